"""The 2048 n-tuple network on the device (csrc/tfe_ntuple.hip: pulse_tfe_nt_rollout, pulse_tfe_nt_learn,
pulse_tfe_nt_apply, pulse_tfe_nt_evaluate) against the host's statement of it (tests/tfe_nt_host.py: the oracle's environment under
greedy_nt_on_host; learn_nt_on_host, apply_nt_on_host) and the environment's own kernels.  Every comparison is exact: keys, bytes and
integers word for word, values and weights as bit patterns.  Every buffer a launch is handed sits between guard words, and the rows of
keys / values / steps at and beyond a game's length must keep what they held.

Shape: 257 games (one full workgroup and one of one lane), max_steps 256, epsilon .25, gamma 1, alpha 1, the tuples (0, 1, 2, 3) and
(4, 5, 6, 8, 9, 10) -- the 6-tuple gives indices above 2^16 and reads cells of the upper word of the board.  Three rounds, played once
and shared: the roll-out of round r runs on the DEVICE's weights after r rounds, read back; the learner and the apply launch are held
to the host's on the device's own recorded games and accumulators.  Rehearsed on the host: every round has games that end (the
`terminal` bit, target 0) and games cut at move 256 (the skipped last move)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD_BYTES, GUARD_FILL = 256, 0x77
KEY_FILL, STEP_FILL, VALUE_FILL = 0x5A5A5A5A5A5A5A5A, 0xEE, -12345.678
GAMES, MAX_STEPS, ROUNDS, EPSILON = 257, 256, 3, .25
TUPLES = ((0, 1, 2, 3), (4, 5, 6, 8, 9, 10))
SEED, BOARD_ID0 = 457, 3000


def _agent(n_games=GAMES, **kw):
    """The agent with every device buffer re-seated between guard words; keys / values / steps pre-filled with a pattern."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    kw = dict(dict(tuples=TUPLES, epsilon=EPSILON, max_steps=MAX_STEPS, seed=SEED, board_id0=BOARD_ID0), **kw)
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), n_games, **kw)
    a._guards = []
    for name, fill in (("weights_dev", 0), ("acc", 0), ("keys", KEY_FILL), ("values", VALUE_FILL), ("steps", STEP_FILL), ("lengths", 0),
                       ("total_score", 0), ("episode_reward", 0), ("counters", 0), ("_eval", 0)):
        t = getattr(a, name)
        g = GUARD_BYTES // t.element_size()
        flat = torch.empty(t.numel() + 2 * g, dtype=t.dtype, device=t.device)
        flat.view(torch.uint8).fill_(GUARD_FILL)
        inner = flat[g:g + t.numel()].view(t.shape)
        inner.fill_(fill)
        setattr(a, name, inner)
        a._guards.append((name, flat, g))
    assert a.acc.data_ptr() % 16 == 0
    return a


def _guards_intact(a):
    import torch
    for name, flat, g in a._guards:
        b = flat.view(torch.uint8)
        gb = g * flat.element_size()
        assert bool((b[:gb] == GUARD_FILL).all()) and bool((b[-gb:] == GUARD_FILL).all()), f"guard words of {name} were written"


def _read(a):
    """the last roll-out's buffers in full (not trimmed to the longest game); values as bit patterns"""
    return dict(keys=a.keys.cpu().numpy().view(np.uint64), values=a.values.cpu().numpy().view(np.uint64), steps=a.steps.cpu().numpy(),
                lengths=a.lengths.cpu().numpy(), total_score=a.total_score.cpu().numpy(), episode_reward=a.episode_reward.cpu().numpy())


def _rollout(a):
    before = _read(a)
    a.rollout()
    return dict(_read(a), **{k + "_before": before[k] for k in ("keys", "values", "steps")})


def _host_rollout(a, weights, **kw):
    from tests.tfe_nt_host import rollout_nt_on_host
    kw = dict(dict(epsilon=a.epsilon, board_id0=a.round_board_id0()), **kw)
    return rollout_nt_on_host(a.n_games, a.max_steps, kw["epsilon"], a.gamma, weights, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                              kw["board_id0"], a.round)


def _assert_rollout(got, want, where):
    """word for word; at and beyond a game's length the rows hold what they held before the launch"""
    L = want["lengths"]
    assert np.array_equal(got["lengths"], L), where
    played = np.arange(got["keys"].shape[0])[:, None] < L[None, :]
    assert np.array_equal(got["keys"][played], want["keys"][played]), where
    assert np.array_equal(got["values"][played], want["values"].view(np.uint64)[played]), where
    assert np.array_equal(got["steps"][played], want["steps"][played]), where
    for k in ("keys", "values", "steps"):
        assert np.array_equal(got[k][~played], got[k + "_before"][~played]), (where, k)
    assert np.array_equal(got["total_score"], want["total_score"]) and np.array_equal(got["episode_reward"], want["episode_reward"]), where


def _play_rounds(symmetric, rounds):
    """`rounds` rounds on the device and on the host: (the agent after them, per round a record).  The big arrays are compared here,
    where they are, and the records keep the verdicts and the counts."""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a = _agent(symmetric=symmetric)
    out, moves, learnt, skipped = [], 0, 0, 0
    for _ in range(rounds):
        policy = a.weights()
        want = _host_rollout(a, policy)
        got = _rollout(a)
        a.learn()
        acc = a.acc.cpu().numpy()
        host_acc = np.zeros_like(acc)
        st = nt.learn_nt_on_host(got["keys"], got["values"].view(np.float64), got["steps"], got["lengths"], a.tuples, a.symmetric, a.gamma, host_acc)
        moves, learnt, skipped = moves + int(got["lengths"].sum()), learnt + st["learnt"], skipped + st["skipped"]
        rec = dict(got=got, want=want, acc_equal=np.array_equal(acc, host_acc), acc_cells=int((acc[:, 1] > 0).sum()), acc_adds=int(acc[:, 1].sum()),
                   acc_max_cnt=int(acc[:, 1].max()), host=st, stats_learn=a.stats(), moves=moves, learnt=learnt, skipped=skipped,
                   board_id0=a.round_board_id0())
        a.apply()
        weights = a.weights()
        host_w = policy.copy()
        rec["moved"] = nt.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features)
        untouched = acc[:, 1] == 0
        rec.update(weights_equal=np.array_equal(weights.view(np.uint32), host_w.view(np.uint32)), acc_zero=not bool(a.acc.any().item()),
                   untouched_kept=np.array_equal(weights.view(np.uint32)[untouched], policy.view(np.uint32)[untouched]),
                   weights_changed=int((weights.view(np.uint32) != policy.view(np.uint32)).sum()), max_index=int(np.flatnonzero(~untouched).max()))
        out.append(rec)
        a.round += 1
    _guards_intact(a)
    return a, out


@functools.lru_cache(maxsize=None)
def _rounds():
    return _play_rounds(True, ROUNDS)


def test_every_round_has_ended_and_cut_games():
    _, rounds = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["want"]["ended"] >= 8 and rec["want"]["truncated"] >= 8, (r, rec["want"]["ended"], rec["want"]["truncated"])
        assert rec["want"]["capped"] == 0


def test_rollout_equals_the_host_word_for_word():
    """round 0 on zero weights, rounds 1 and 2 on the device's own weights read back"""
    a, rounds = _rounds()
    cut = 0
    for r, rec in enumerate(rounds):
        _assert_rollout(rec["got"], rec["want"], r)
        cut += rec["want"]["truncated"]
        assert rec["stats_learn"]["moves"] == rec["moves"] and rec["stats_learn"]["truncated"] == cut
    assert not rounds[0]["want"]["values"].any() and rounds[2]["want"]["values"].any()
    assert int(rounds[2]["want"]["keys"].max()) >= 1 << 36 and 0 < rounds[2]["want"]["greedy"] < rounds[2]["moves"] - rounds[1]["moves"]


def test_rollout_without_symmetry():
    """symmetric = 0: one feature per tuple; the second round runs on weights the first one learnt"""
    _, rounds = _play_rounds(False, 2)
    for r, rec in enumerate(rounds):
        _assert_rollout(rec["got"], rec["want"], r)
        assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["acc_adds"] == 2 * rec["host"]["learnt"], r
    assert rounds[1]["want"]["values"].any()


def test_recorded_actions_replay_through_the_environment():
    """TFEBatch (pulse_tfe_reset / pulse_tfe_step) with the same seed and board ids, stepped by the recorded actions, meets the boards
    whose moved images pack to the recorded keys, with the recorded rewards, terminal bits and final scores."""
    import torch
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from pulselib_amd.environments.TFE.TFE import TFEBatch
    from tests.tfe_mc_host import pack_boards
    a, rounds = _rounds()
    rec = rounds[2]
    got, L = rec["got"], rec["got"]["lengths"]
    actions, rewards, terminal = nt.unpack_steps(got["steps"])
    env = TFEBatch(a.device, GAMES, 4, seed=a.env_seed, board_id0=rec["board_id0"])
    boards, _ = env.reset()
    final, rows = np.zeros(GAMES, dtype=np.int64), np.arange(GAMES)
    for t in range(int(L.max())):
        live = L > t
        after, scores = nt.moves_on_host(pack_boards(boards.cpu().numpy()))
        act = np.where(live, actions[t], 0).astype(np.int64)
        assert np.array_equal(after[rows, act][live], got["keys"][t][live]), t
        assert np.array_equal(nt.rewards_of_scores(scores[rows, act])[live], rewards[t][live]), t
        boards, rew, dones, _, info = env.step(torch.from_numpy(act).to(a.device))
        assert np.array_equal(rew.cpu().numpy()[live], rewards[t][live].astype(np.int32)), t
        assert np.array_equal(dones.cpu().numpy()[live] != 0, terminal[t][live]), t
        ends = L == t + 1
        final[ends] = info["score"].cpu().numpy()[ends]
    assert np.array_equal(final, got["total_score"])


def test_learn_equals_the_host_word_for_word():
    """acc read back before the apply launch, over all W; exact integers: the adds commute.  learnt + skipped = the moves played, the
    skipped moves are the cut games, every learnt move added F times."""
    a, rounds = _rounds()
    for r, rec in enumerate(rounds):
        st = rec["stats_learn"]
        assert rec["acc_equal"], r
        assert st["learnt"] == rec["learnt"] and st["skipped"] == rec["skipped"] and st["learnt"] + st["skipped"] == st["moves"] == rec["moves"], r
        assert rec["host"]["skipped"] == rec["want"]["truncated"] and st["clamped"] == 0
        assert rec["acc_adds"] == a.n_features * rec["host"]["learnt"] and rec["acc_max_cnt"] > GAMES and rec["max_index"] >= 1 << 16, r


def test_apply_equals_the_host_bit_for_bit():
    _, rounds = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["weights_equal"] and rec["acc_zero"] and rec["untouched_kept"], r
        assert rec["moved"] == rec["acc_cells"] and 0 < rec["weights_changed"] <= rec["moved"], r


@pytest.mark.parametrize("epsilon", [0.0, EPSILON])
def test_evaluate_plays_the_rollouts_games(epsilon):
    """the 24 counters and the per-game arrays against the host's games under the weights of three rounds"""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_nt_host import eval_words
    a, _ = _rounds()
    want = _host_rollout(a, a.weights(), epsilon=epsilon)
    ev = a.evaluate(epsilon=epsilon, board_id0=a.round_board_id0(), per_game=True)
    assert np.array_equal(ev["total_score"], want["total_score"]) and np.array_equal(ev["lengths"], want["lengths"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == eval_words(want)
    assert ev["games"] == GAMES and (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0) and sum(ev["max_tile_hist"]) == GAMES
    if epsilon:
        a.epsilon, keep = epsilon, a.epsilon                               # ... and they are the games the roll-out records
        got = _rollout(a)
        a.epsilon = keep
        assert np.array_equal(got["total_score"], ev["total_score"]) and np.array_equal(got["lengths"], ev["lengths"])
    small = a.evaluate(n_games=64)                                         # the defaults: epsilon 0, other boards, no arrays
    assert small["games"] == 64 and "total_score" not in small
    _guards_intact(a)


def test_save_and_load_on_the_device(tmp_path):
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a, _ = _rounds()
    a.save(tmp_path / "net.npz")
    b = NTupleTDAfterstateTFEGPU.load(tmp_path / "net.npz", torch.device("cuda:0"))
    assert np.array_equal(b.weights().view(np.uint32), a.weights().view(np.uint32)) and b.round == a.round and b.tuples == a.tuples
    assert (b.n_games, b.max_steps, b.epsilon, b.gamma, b.alpha, b.seed, b.board_id0, b.symmetric) == \
        (a.n_games, a.max_steps, a.epsilon, a.gamma, a.alpha, a.seed, a.board_id0, a.symmetric)
    assert b.evaluate(n_games=64) == a.evaluate(n_games=64)


def test_it_learns():
    """The default network, 4,096 games per round, max_steps 4,096, epsilon 0, gamma 1, alpha 1, seed 0; the greedy policy evaluated on
    2,048 games from reset.  Two rounds beat the zero weights (greedy on the reward) by at least five standard errors of the
    difference.  Rehearsed on the host with 256 games per round: 1,898 +- 60 on zero weights, 4,426 +- 140 after one round, 5,182 +- 175
    after two.  On an MI355X: 1,993.3 +- 19.9 on zero weights, 6,523.9 +- 66.0 after the two rounds."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0)
    empty = a.evaluate(n_games=2048)
    after = a.learn_batch().learn_batch().evaluate(n_games=2048)
    se = lambda e: e["std_score"] / e["games"] ** .5
    print("greedy mean score on 2,048 games: zero weights", empty["mean_score"], "+-", se(empty), "after two rounds", after["mean_score"], "+-",
          se(after), "mean length", empty["mean_length"], after["mean_length"], "stats", a.stats(), "cut", after["truncated"])
    st = a.stats()
    assert st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not a.acc.any().item()
    assert after["mean_score"] - empty["mean_score"] >= 5.0 * np.hypot(se(after), se(empty)), (after["mean_score"], empty["mean_score"])
