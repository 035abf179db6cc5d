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

from tests.tfe_gpu_support import assert_rollout, guards_intact, replay, rollout
from tests.tfe_nt_support import EPSILON_PLAY as EPSILON
from tests.tfe_nt_support import GAMES, MAX_STEPS, PER_MOVE, ROUNDS, learner_agent, learner_round

pytestmark = pytest.mark.gpu


def _host_rollout(a, weights, **kw):
    from tests.tfe_nt_host import nt_games_on_host
    kw = dict(dict(epsilon=a.epsilon, board_id0=a.round_board_id0()), **kw)
    return nt_games_on_host(a.n_games, a.max_steps, kw["epsilon"], a.gamma, weights, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                            kw["board_id0"], a.round)


def _play_rounds(symmetric, rounds):
    """`rounds` rounds on the device and on the host: (the agent after them, per round learner_round's record with this file's own:
    the roll-out held to the host's, the counters since the first round, and what the apply launch changed)."""
    a = learner_agent(symmetric=symmetric)
    out, total = [], dict(moves=0, learnt=0, skipped=0)

    def after_learn(a, h):
        total.update(moves=total["moves"] + int(h.L.sum()), learnt=total["learnt"] + h.host["learnt"], skipped=total["skipped"] + h.host["skipped"])
        return dict(total, got=h.got, want=_host_rollout(a, h.policy), acc_cells=int(h.visited.sum()), acc_max_cnt=int(h.acc[:, 1].max()),
                    stats_learn=a.stats(), board_id0=a.round_board_id0())

    def after_apply(a, h):
        untouched = ~h.visited
        return dict(untouched_kept=np.array_equal(h.weights.view(np.uint32)[untouched], h.policy.view(np.uint32)[untouched]),
                    weights_changed=int((h.weights.view(np.uint32) != h.policy.view(np.uint32)).sum()), max_index=int(np.flatnonzero(~untouched).max()))
    for _ in range(rounds):
        out.append(learner_round(a, after_learn, after_apply))
    guards_intact(a)
    return a, out


@functools.lru_cache(maxsize=None)
def _rounds():
    return _play_rounds(True, ROUNDS)


@functools.lru_cache(maxsize=None)
def _plain_rounds():
    return _play_rounds(False, 2)


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
        assert_rollout(rec["got"], rec["want"], r, PER_MOVE)
        cut += rec["want"]["truncated"]
        assert rec["stats_learn"]["moves"] == rec["moves"] and rec["stats_learn"]["truncated"] == cut
    assert not rounds[0]["want"]["values"].any() and rounds[2]["want"]["values"].any()
    assert int(rounds[2]["want"]["keys"].max()) >= 1 << 36 and 0 < rounds[2]["want"]["greedy"] < rounds[2]["moves"] - rounds[1]["moves"]


def test_rollout_without_symmetry():
    """symmetric = 0: one feature per tuple; the second round runs on weights the first one learnt"""
    _, rounds = _plain_rounds()
    for r, rec in enumerate(rounds):
        assert_rollout(rec["got"], rec["want"], r, PER_MOVE)
        assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["acc_adds"] == 2 * rec["host"]["learnt"], r
    assert rounds[1]["want"]["values"].any()


def test_evaluate_without_symmetry():
    """symmetric = 0 in the evaluation launch: the per-game arrays and the 24 counters against the host's games under the weights of
    the two rounds without symmetry.  Rehearsed on the host: 242 games end and 15 are cut at epsilon .25, 203 and 54 at 0, none capped."""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, _ = _plain_rounds()
    weights = a.weights()
    for epsilon in (EPSILON, 0.0):
        want = _host_rollout(a, weights, epsilon=epsilon)
        assert want["ended"] >= 8 and want["truncated"] >= 8 and want["capped"] == 0, (epsilon, want["ended"], want["truncated"], want["capped"])
        ev = a.evaluate(epsilon=epsilon, board_id0=a.round_board_id0(), per_game=True)
        assert np.array_equal(ev["total_score"], want["total_score"]) and np.array_equal(ev["lengths"], want["lengths"]), epsilon
        words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
        assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words, epsilon
    guards_intact(a)


def test_recorded_actions_replay_through_the_environment():
    """TFEBatch (pulse_tfe_reset / pulse_tfe_step) with the same seed and board ids, stepped by the recorded actions, meets the boards
    whose moved images pack to the recorded keys, with the recorded rewards, terminal bits and final scores."""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from tests.tfe_host import pack_boards
    a, rounds = _rounds()
    got, L, rows = rounds[2]["got"], rounds[2]["got"]["lengths"], np.arange(GAMES)
    _, rewards, terminal = nt.unpack_steps(got["steps"])

    def recorded_afterstate(t, live, boards, actions):
        after, scores = nt.moves_on_host(pack_boards(boards))
        assert np.array_equal(after[rows, actions][live], got["keys"][t][live]), t
        assert np.array_equal(nt.rewards_of_scores(scores[rows, actions])[live], rewards[t][live]), t
        return actions
    _, _, done = replay(a, got, recorded_afterstate, rounds[2]["board_id0"])
    played = np.arange(MAX_STEPS)[:, None] < L[None, :]                    # the terminal bit: the game's last move, where the environment ended it
    assert np.array_equal(terminal[played], ((np.arange(MAX_STEPS)[:, None] == L[None, :] - 1) & done[None, :])[played])


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
    from tests.tfe_host import eval_words
    a, _ = _rounds()
    want = _host_rollout(a, a.weights(), epsilon=epsilon)
    ev = a.evaluate(epsilon=epsilon, board_id0=a.round_board_id0(), per_game=True)
    assert np.array_equal(ev["total_score"], want["total_score"]) and np.array_equal(ev["lengths"], want["lengths"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words
    assert ev["games"] == GAMES and (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0) and sum(ev["max_tile_hist"]) == GAMES
    if epsilon:
        a.epsilon, keep = epsilon, a.epsilon                               # ... and they are the games the roll-out records
        got = rollout(a, PER_MOVE)
        a.epsilon = keep
        assert np.array_equal(got["total_score"], ev["total_score"]) and np.array_equal(got["lengths"], ev["lengths"])
    small = a.evaluate(n_games=64)                                         # the defaults: epsilon 0, other boards, no arrays
    assert small["games"] == 64 and "total_score" not in small
    guards_intact(a)


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
