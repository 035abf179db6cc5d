"""The 2048 n-tuple network's games continued across rounds on the device (csrc/tfe_ntuple_continue.hip:
pulse_tfe_nt_continue_pick) against the host's statement of them (continue_pick_on_host; tests/tfe_continue_host.py: the host's
roll-out from `start`, then the pick, with the test's own count of every game's moves beside the carries).  Every comparison but the
last is exact: integers word for word, float64 and float32 as bit patterns.  Every buffer a launch is handed sits between guard
words, and the rows of keys / values / steps / backed at and beyond a game's length must keep what they held.

Shapes: one ply 257 games (one full workgroup and one of one lane) in segments of 16 moves at epsilon .25 on the seeded weights of
the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), gamma 1 -- rehearsed on the host: from round 2 or 3 on every round both ends games and
cuts games --; one layer section 13.5's 17 games of at most 192 moves, seed 2312, where the host shows 4 games cut in round 0."""
import numpy as np
import pytest

from tests.tfe_continue_host import WORDS, Carried, pick_on_host
from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guards_intact, read
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import BOARD_ID0, BUFFERS, GAMES, PER_MOVE, TUPLES, bits, learner_agent, learner_round, nt, plain_learner, weights

pytestmark = pytest.mark.gpu

SEGMENT = 16
START_PATTERN, BACKED_PATTERN = 0x3C3C3C3C3C3C3C3C, -4321.125              # what `start` and `backed` hold before the first launch
CONTINUE_STATE = ("start", "restart_stats", "carry_score", "carry_moves", "finished")


def _with_continue(a, backed=False):
    """the agent with `start`, the carries and `finished` (and a `backed`) of its own between guard words: `start` and `backed` hold
    patterns, the carries and `finished` zero"""
    import torch
    a._continue_state()
    names = CONTINUE_STATE
    if backed:
        a.backed, names = torch.zeros_like(a.values), names + ("backed",)
    return guard(a, names, start=START_PATTERN, backed=BACKED_PATTERN)


def _seeded(a):
    import torch
    a.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
    return a


def _start_of(a):
    return a.start.cpu().numpy().view(np.uint64)


def _assert_state(a, c, where):
    """`start`, both carries and the 24 words of `finished` against the host's, and the guard words"""
    assert np.array_equal(_start_of(a), c.start), where
    assert np.array_equal(a.carry_score.cpu().numpy(), c.score) and np.array_equal(a.carry_moves.cpu().numpy(), c.moves), where
    assert a.finished.cpu().tolist() == c.finished, (where, a.finished.cpu().tolist(), c.finished)
    guards_intact(a)


# ------------------------------------------------------------------ the pick
def test_the_pick_is_the_hosts():
    """Four rounds of 257 games of 16 moves at epsilon .25 on the seeded weights, seeds 11 / 12 / 13, round r on the boards 1000 + 257 r:
    after every recording launch the pick on the device's own records against the host's -- `start`, both carries, `finished`, the
    guard words.  The first pick finds `start` full of a pattern and writes every entry; the later ones add to the carries and to
    `finished`.  Rehearsed on the host (tests/test_tfe_nt_continue_cpu.py, the same games): rounds 0 and 1 end no game, round 2 two,
    round 3 ends 17 and cuts 240."""
    a = _seeded(_with_continue(learner_agent(max_steps=SEGMENT, board_id0=1000)))
    a.env_seed, a.agent_seed, a.tie_seed = 11, 12, 13
    c, counts = Carried(GAMES), []
    assert (_start_of(a) == np.uint64(START_PATTERN)).all() and not a.finished.any().item()
    for r in range(4):
        if r:
            a.rollout_from_launch(0)
            assert np.array_equal(_start_of(a), c.start)                    # boards a game moved on: none is zeroed
        else:
            a._launch("pulse_tfe_nt_rollout", a._rollout_struct())
        got = read(a, PER_MOVE)
        words, cut = pick_on_host(c, got, SEGMENT, a.env_seed, a.round_board_id0())
        a.continue_pick_launch()
        _assert_state(a, c, ("round", r))
        after = read(a, PER_MOVE)
        assert all(np.array_equal(after[k], got[k]) for k in got), r      # the records are only read
        counts.append((words[0], words[5]))
        a.round += 1
    print("games finished / continued per round:", counts, "finished:", c.finished)
    assert counts[0] == (0, GAMES) and counts[3][0] >= 10 and counts[3][1] >= 10 and c.score.any() and c.finished[6] == c.finished[0] > 0
    summary = a.finished_summary(clear=False)
    assert summary == nt().finished_summary_on_host(c.finished) and a.finished.cpu().tolist() == c.finished
    assert a.finished_summary()["games"] == c.finished[0] and not a.finished.any().item()
    guards_intact(a)


# ------------------------------------------------------------------ rounds
def _continued_round(a, c, coherence, where):
    """learner_round with the games held to the host's from the `start` the pick of the round before left and, after the apply, the
    pick launch held to the host's"""
    def games(a, h):
        want = nt_games_on_host(a.n_games, a.max_steps, a.epsilon, a.gamma, h.policy, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                                a.round_board_id0(), a.round, start=c.start)
        kept = want["start_left"]
        assert_rollout(h.got, want, where, PER_MOVE)
        assert np.array_equal(_start_of(a), kept) and np.array_equal(kept, c.start), where
        return dict(continued=int(np.count_nonzero(kept)))

    def pick(a, h):
        a.continue_pick_launch()
        words, _ = pick_on_host(c, h.got, a.max_steps, a.env_seed, a.round_board_id0())
        _assert_state(a, c, where)
        return dict(finished=words[0], cut_by_pick=words[5])
    return learner_round(a, after_learn=games, after_apply=pick, coherence=coherence)


def _assert_twins(a, b, more=()):
    """two agents after the same rounds: the weights, the per-game arrays, the counters, `start`, the carries and `finished` whole, the
    per-move rows up to each game's length (beyond it one holds its patterns and the other zeros)"""
    import torch
    for k in ("weights_dev", "lengths", "total_score", "episode_reward", "counters", "start", "carry_score", "carry_moves", "finished"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    played = np.arange(a.max_steps)[:, None] < a.lengths.cpu().numpy()[None, :]
    for k in PER_MOVE + tuple(more):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint64 if x.itemsize == 8 else x.dtype)[played], y.view(np.uint64 if y.itemsize == 8 else y.dtype)[played]), k


@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=0.5, tc=True)], ids=["lambda0", "lambda.5-tc"])
def test_five_continued_rounds_are_the_hosts(kw):
    """From the seeded weights: acc over all W, the counters and the weights as float32 bit patterns per round (learner_round), the
    games from the boards the round before left and the pick itself; then learn_batch() five times on a twin agent leaves the same
    weights, records, start, carries and finished.  Rehearsed on the host: 0 / 0 / 2 / 16 / 42 games end at lambda 0, 0 / 0 / 3 / 11 / 35
    with lambda .5 and tc; every other game is cut, so a round learns 15 moves of each and skips its last."""
    a = _seeded(_with_continue(learner_agent(max_steps=SEGMENT, extra_buffers=("deltas", "acc_abs", "E", "A", "tc_stats"), **kw)))
    a.start.zero_()                                                         # (its own start, guarded: a first round from zeros is a round from reset)
    b = _seeded(plain_learner(max_steps=SEGMENT, **kw))
    a.continue_games = b.continue_games = True
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if a.tc else None
    c, recs = Carried(GAMES), []
    for r in range(5):
        recs.append(_continued_round(a, c, coherence, ("round", r)))
        guards_intact(a)
    print([{k: rec[k] for k in ("ended", "cut", "moves", "continued", "finished", "cut_by_pick", "host", "stats")} for rec in recs])
    for rec in recs:
        assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["stats"] == {k: rec["host"][k] for k in rec["stats"]}, rec
        assert rec["finished"] + rec["cut_by_pick"] == GAMES and rec["cut_by_pick"] == rec["host"]["skipped"] >= 1, rec
        assert rec["host"]["learnt"] == rec["moves"] - rec["cut_by_pick"], rec     # every move but a cut game's last: learnt once
    assert recs[0]["continued"] == 0 and [rec["continued"] for rec in recs[1:]] == [rec["cut_by_pick"] for rec in recs[:4]]
    assert sum(rec["finished"] for rec in recs) == c.finished[0] >= 1
    if a.tc:
        E, A = a.coherence()
        assert np.array_equal(bits(E), bits(coherence[0])) and np.array_equal(bits(A), bits(coherence[1]))
    assert b.start is None and b.carry_score is None and b.finished is None
    for _ in range(5):
        b.learn_batch()
    assert a.round == b.round == 5 and b.finished_summary(clear=False) == nt().finished_summary_on_host(c.finished)
    _assert_twins(a, b)


def test_three_continued_rounds_under_search_with_backed_targets_are_the_hosts():
    """rollout_layers = 1, backed_targets, lambda .5: section 13.5's 17 games of at most 192 moves at epsilon .25, the first round from the
    seeded weights.  Rehearsed on the host: 4 / 4 / 1 games are cut at move 192 and 13 / 13 / 16 end.  Per round the games and backed
    values from the boards the round before left, acc, the counters, the weights as bit patterns and the pick; then learn_batch()
    three times on a twin agent.  The backed walk ends at a segment's cut: the host's learner on the segment's records is the statement."""
    n, games, max_steps, seed = nt(), 17, 192, 2312
    make = lambda: _seeded(plain_learner(games, max_steps=max_steps, seed=seed, lam=0.5))
    a, b = make(), make()
    a = _with_continue(guard(a, BUFFERS + ("deltas",), **PATTERNS), backed=True)
    _seeded(a).start.zero_()
    for agent in (a, b):
        agent.rollout_layers, agent.backed_targets, agent.continue_games = 1, True, True
    c, counts = Carried(games), []
    for r in range(3):
        policy, before_rows, st0 = a.weights(), bits(a.backed.cpu().numpy()), a.stats()
        before = read(a, PER_MOVE)
        a.rollout()
        got = dict(read(a, PER_MOVE), **{k + "_before": v for k, v in before.items() if k in PER_MOVE})
        want = nt_games_on_host(games, max_steps, a.epsilon, a.gamma, policy, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                                a.round_board_id0(), a.round, depth=1, backed=True, start=c.start)
        kept = want["start_left"]
        assert_rollout(got, want, ("round", r), PER_MOVE)
        L = got["lengths"].astype(np.int64)
        played, backed = np.arange(max_steps)[:, None] < L[None, :], bits(a.backed.cpu().numpy())
        assert np.array_equal(backed[played], bits(want["backed"])[played]) and np.array_equal(backed[~played], before_rows[~played])
        assert np.array_equal(_start_of(a), kept) and np.array_equal(kept, c.start)
        a.learn()
        st, acc = a.stats(), a.acc.cpu().numpy()
        host_acc = np.zeros_like(acc)
        host = n.learn_backed_nt_on_host(got["keys"], got["values"].view(np.float64), backed.view(np.float64), got["steps"], L, a.tuples, a.symmetric,
                                         a.gamma, a.lam, host_acc)
        assert np.array_equal(acc, host_acc) and {k: st[k] - st0[k] for k in ("learnt", "skipped", "clamped")} == {k: host[k] for k in ("learnt", "skipped", "clamped")}
        a.apply()
        host_w = policy.copy()
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0
        assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)) and not a.acc.any().item()
        a.continue_pick_launch()
        words, _ = pick_on_host(c, got, max_steps, a.env_seed, a.round_board_id0())
        _assert_state(a, c, ("round", r))
        assert host["skipped"] == words[5] == want["truncated"] and host["learnt"] + host["skipped"] == int(L.sum())
        counts.append((words[0], words[5]))
        a.round += 1
    print("games finished / continued per round:", counts)
    assert counts[0][1] >= 1 and all(done >= 1 for done, _ in counts) and c.finished[6] >= 1, counts     # a game is cut, and a continued game ends
    for _ in range(3):
        b.learn_batch()
    _assert_twins(a, b, ("backed", "deltas"))


def test_continued_rounds_on_stages_keep_start():
    """stage_tiles: the staged launch from `start`, which rollout() must not zero while continuing: three rounds of learn_batch() on a
    staged agent whose slices are all the seeded weights against the pick's state of an unstaged twin after its first round -- the two
    play the same first round -- and `start` still holds the cut games' boards after the second round's launch."""
    import torch
    a = _seeded(plain_learner(33, max_steps=SEGMENT))
    s = plain_learner(33, max_steps=SEGMENT, stage_tiles=(64, 512))
    s.weights_dev.copy_(a.weights_dev.repeat(s.n_stages))
    a.continue_games = s.continue_games = True
    a.rollout()
    s.rollout()
    for k in ("keys", "values", "steps", "lengths", "total_score"):
        assert torch.equal(getattr(a, k), getattr(s, k)), k
    a.continue_pick_launch()
    s.continue_pick_launch()
    assert torch.equal(a.start, s.start) and int((s.start != 0).sum().item()) == 33      # no game of 2048 ends within 16 moves
    s.round += 1
    picked = s.start.clone()
    s.rollout()
    assert torch.equal(s.start, picked)                                     # not zeroed, and every board usable
    s.continue_games = False
    s.rollout()
    assert not s.start.any().item()                                         # off: the staged launch plays from reset again


def test_without_the_attribute_three_rounds_are_todays():
    import torch
    from pulselib_amd import _native
    a, b = plain_learner(33, max_steps=SEGMENT), plain_learner(33, max_steps=SEGMENT)
    assert a.continue_games is False and a.eval_max_steps is None and a.start is None
    for _ in range(3):
        a.learn_batch()
        b._launch("pulse_tfe_nt_rollout", b._rollout_struct())._launch("pulse_tfe_nt_learn", b._moves(_native.TfeNtLearn())).apply()
        b.round += 1
    for k in ("weights_dev", "keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.round == 3 and a.weights().any() and a.stats()["truncated"] == 3 * 33      # every game cut at 16 moves, and reset
    assert a.start is None and a.restart_stats is None and a.carry_score is None and a.carry_moves is None and a.finished is None
    with pytest.raises(ValueError, match="holds no finished"):
        a.finished_summary()


# ------------------------------------------------------------------ the evaluations' own cap
def _host_whole_games(a, max_steps):
    return nt_games_on_host(a.n_games, max_steps, 0.0, a.gamma, a.weights(), a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                            a.eval_board_id0(), a.round)


@pytest.mark.parametrize("cap", [None, 4096], ids=["agents_max_steps", "4096"])
def test_eval_max_steps(cap):
    """An agent with max_steps 16 on the seeded weights: with eval_max_steps None the evaluation is today's -- the 24 counters and the
    per-game arrays of the host's games cut at 16 moves --; with 4,096 they are the host's whole games, under search as well as one
    ply deep (evaluate_search goes through the same launch).  33 games: two workgroups' worth of nothing, so the whole games take a
    second on the host."""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a = _seeded(learner_agent(33, max_steps=SEGMENT))
    a.eval_max_steps = cap
    want = _host_whole_games(a, SEGMENT if cap is None else cap)
    assert (want["truncated"], want["ended"]) == ((33, 0) if cap is None else (0, 33)) and (cap is None or int(want["lengths"].max()) > 4 * SEGMENT)
    ev = a.evaluate(per_game=True)
    assert np.array_equal(ev["total_score"], want["total_score"]) and np.array_equal(ev["lengths"], want["lengths"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"],
                                                                            want["greedy"], want["capped"])
    searched = a.evaluate_search(per_game=True)
    assert searched["games"] == 33 and searched["truncated"] == (33 if cap is None else 0)
    assert int(searched["lengths"].max()) == SEGMENT if cap is None else int(searched["lengths"].max()) > 4 * SEGMENT
    guards_intact(a)


# ------------------------------------------------------------------ the score
def test_it_learns():
    """The default network, 1,024 games per round, epsilon 0, seed 0, from zero weights.  A: max_steps 64 with continue_games, eight
    rounds; B: max_steps 4,096, two rounds of whole games.  Then 1,024 one-ply evaluation games from the default evaluation boards,
    capped at 4,096 moves, on A, on B and on zero weights, paired by board.  Asserted: A learnt from fewer moves than B; A beats zero
    weights by at least five standard errors of the paired difference; A beats B by at least five standard errors of the paired
    difference.  On an MI355X (one run): A learnt 500,590 moves and B 564,024; zero weights 2,025.6 +- 29.0, B 6,046.0 +- 92.6,
    A 9,803.8 +- 159.3; A minus zero +7,778.2 +- 160.8 (48 standard errors), A minus B +3,757.8 +- 187.3 (20); while training, 585 whole
    games of A finished with a mean score of 4,806.1.  The host chain of A's eight rounds (tests/tfe_continue_host.py, learn_nt_on_host,
    apply_nt_on_host) gives the same 500,590 moves, 585 games and 4,806.1.  The rehearsal before the unit was written had reported
    508,197 moves for A and, with the evaluation's tie coins of round 99, zero weights 1,954.2 +- 28.7, B 6,126.6 +- 90.5, A 10,446.9
    +- 169.7 (+8,492.7 +- 172.4 and +4,320.3 +- 190.2): B's moves are reproduced, A's are not."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    dev = torch.device("cuda:0")
    a = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=64, seed=0)
    a.continue_games, a.eval_max_steps = True, 4096
    for _ in range(8):
        a.learn_batch()
    b = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=4096, seed=0)
    for _ in range(2):
        b.learn_batch()
    sa, sb, done = a.stats(), b.stats(), a.finished_summary()
    for st in (sa, sb):
        assert st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"]
    assert a.round == 8 and b.round == 2 and not a.acc.any().item() and done["games"] + int((a.start != 0).sum().item()) >= 1024
    zero = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=4096, seed=0)
    ev = {name: agent.evaluate(n_games=1024, per_game=True) for name, agent in (("a", a), ("b", b), ("zero", zero))}
    se = lambda e: e["std_score"] / e["games"] ** .5

    def paired(x, y):
        d = (ev[x]["total_score"] - ev[y]["total_score"]).astype(np.float64)
        return d.mean(), d.std(ddof=1) / np.sqrt(d.size)
    (gain, gain_se), (over, over_se) = paired("a", "zero"), paired("a", "b")
    print("moves learnt: continued", sa["learnt"], "whole games", sb["learnt"], "whole games finished while training A:", done["games"], "mean score",
          done["mean_score"], "mean length", done["mean_length"], "one-ply evaluation: zero", ev["zero"]["mean_score"], "+-", se(ev["zero"]), "B",
          ev["b"]["mean_score"], "+-", se(ev["b"]), "A", ev["a"]["mean_score"], "+-", se(ev["a"]), "A minus zero", gain, "+-", gain_se, "A minus B", over, "+-",
          over_se, "clamped", sa["clamped"], sb["clamped"])
    assert all(e["games"] == 1024 for e in ev.values()) and ev["a"]["truncated"] == 0
    assert sa["learnt"] < sb["learnt"], (sa["learnt"], sb["learnt"])
    assert gain >= 5.0 * gain_se, (ev["a"]["mean_score"], ev["zero"]["mean_score"], gain_se)
    assert over >= 5.0 * over_se, (ev["a"]["mean_score"], ev["b"]["mean_score"], over_se)
