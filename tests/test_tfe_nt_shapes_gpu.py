"""The 2048 n-tuple network's device code at the network shapes and on the boards the other GPU files never reach (csrc/tfe_ntuple*.hip),
against the host's statement of it.  Every comparison is exact: integers word for word, float64 and float32 as bit patterns.  Every
buffer a launch is handed sits between guard words.  Where a test rests on counts it asserts the HOST's counts first, so that a changed
seed cannot hide a failure.

Shapes (tests/tfe_nt_support.py: SHAPES): "eight", the ABI's limit of 8 tuples, of lengths 1 to 5 on descending, scattered and
overlapping cells, 1,188,368 weights (the apply launches' last workgroup is ragged); "one6", the other limit, one tuple of length 6,
descending, in the board's upper word; "default", the shipping network of four tuples and 33,685,504 weights.  They reach the `shifts`
table of check_net, feature_index with its mask and offset, the tuple loops of values4 and add_features, step = alpha / n_features,
the one-lane-per-weight grids of the apply launches and the per-workgroup rho sums of pulse_tfe_nt_apply_tc.

Boards: late_start -- nibbles 6..14, a quarter of the boards one move from the 32,768 tile -- as search boards and as the `start` of
pulse_tfe_nt_rollout_from, so that nibbles up to 15 enter feature indices in play and in learning and the cap at the 32,768 tile
(the game is CUT, its last move skipped by the learners) runs inside device games.

Out of scope: the evaluation launches take no `start`, so the cap inside pulse_tfe_nt_evaluate* is reachable only through play_game's
one shared text, which the restarted roll-outs below run with Record; two-layer roll-outs from late boards have no host statement
(nt_games_on_host: `start` needs depth in (0, 1)); no test here reads kernel assembly."""
import functools
import time

import numpy as np
import pytest

from tests.test_tfe_nt_restart_gpu import MODES, START_PATTERN, _assert_games, _launched, _set_start, _start_of, _with_restart
from tests.tfe_gpu_support import PER_GAME, assert_rollout, guard, guarded, guards_intact, read
from tests.tfe_nt_host import nibbles as _nibbles
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import (BOARD_ID0, CRAFTED, MORE, PER_MOVE, ROUNDS, SEED, SHAPES, bits, late_start, learner_agent, learner_round, nt,
                                  search_agent, search_outputs, weights)

pytestmark = pytest.mark.gpu

SYMMETRIC = pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
SETTINGS = {"td0": dict(lam=0.0), "lambda.5": dict(lam=0.5), "lambda.5-tc": dict(lam=0.5, tc=True)}
TC_STATE = ("deltas", "acc_abs", "E", "A", "tc_stats")
# "one6" without symmetry learns games that end early: at seed 457 its later rounds cut 3 to 11 games, and of the seeds 458 to 547 none
# has 8 cut games in every round of every setting.  613 has, found on the host alone (the rounds' docstring).
LEARNER_SEED = {("one6", False): 613}
LATE = (65, 96, 4242)                                                      # games, max_steps, seed of the late-game and the evaluation cases
LATE_EPSILON, ROUND = {0: .05, 1: .25}, 0                                  # by layers, as tests/test_tfe_nt_restart_gpu.py plays them


def _seeds(seed):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return seed, seed ^ AGENT_KEY, seed ^ TIE_KEY


@functools.lru_cache(maxsize=None)
def _small_weights(shape):
    """the seeded weights of the shape divided by 64 (exact): play is led by the rewards and V breaks their ties"""
    w = weights("seeded", SHAPES[shape]) / np.float32(64)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------ 1. search at every shape
@functools.lru_cache(maxsize=None)
def _boards():
    """uint64[9 + 64]: the crafted boards, then the first 64 boards of late_start(86, 3) that are not 0"""
    from tests.tfe_search_host import key_of
    late = late_start(86, 3)
    keys = np.concatenate([np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64), late[late != 0][:64]])
    assert keys.shape == (len(CRAFTED) + len(MORE) + 64,)
    keys.setflags(write=False)
    return keys


@SYMMETRIC
@pytest.mark.parametrize("shape", ["eight", "one6"])
def test_search_equals_the_mirror_at_every_shape(shape, symmetric):
    """pulse_tfe_nt_search and pulse_tfe_nt_search_deep on the crafted boards and 64 late boards under the seeded weights of the shape:
    q as bit patterns, actions and candidates.  On the host first: the second layer changes some q, and some board holds a nibble of
    12 or more in a cell a tuple reads (62 of the 64 late boards do; 50 where "one6" reads its one image)."""
    import torch
    n, tuples, keys = nt(), SHAPES[shape], _boards()
    w = weights("seeded", tuples)
    a = search_agent(7, 16, LATE[2], "seeded", symmetric, tuples=tuples)
    a.round = 3
    want = {layers: n.search_nt_on_host(keys, w, tuples, symmetric, a.gamma, a.tie_seed, a.round, layers=layers) for layers in (1, 2)}
    assert (want[1]["q"] != want[2]["q"]).any(axis=1).sum() >= 8 and (want[2]["action"] >= 0).sum() >= len(keys) - 2
    cells = np.unique(np.concatenate([c.ravel() for c in n.feature_cells_on_host(tuples, symmetric)]))
    assert (_nibbles(keys)[:, cells] >= 12).any(axis=1).sum() >= 8 and np.unique(want[1]["q"]).size > len(keys)
    dev = torch.device("cuda:0")
    boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    for layers in (1, 2):
        q, action, cand, guards = search_outputs(len(keys), dev)
        a.search_launch(boards, q, action, cand, layers=layers)
        assert np.array_equal(cand.cpu().numpy(), want[layers]["candidates"]), layers
        assert np.array_equal(action.cpu().numpy().astype(np.int64), want[layers]["action"]), layers
        assert np.array_equal(q.cpu().numpy().view(np.uint64), want[layers]["q"].view(np.uint64)), layers
        assert np.array_equal(boards.cpu().numpy().view(np.uint64), keys)
        guards_intact(a, [("boards", gb, nb)] + guards)


# ------------------------------------------------------------------ 2. three learner rounds at every shape
def _round(a, coherence, where, least=8):
    """learner_round with the roll-out held to nt_games_on_host on the weights the round played on -- the host's counts asserted
    before the device's records are compared: at least `least` games end and as many are cut -- and, with tc, the third accumulator,
    tc_stats' differences, E and A"""
    def after_learn(a, h):
        want = nt_games_on_host(a.n_games, a.max_steps, a.epsilon, a.gamma, h.policy, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                                a.round_board_id0(), a.round)
        out = dict(want_ended=want["ended"], want_cut=want["truncated"], want_capped=want["capped"])
        assert want["ended"] >= least and want["truncated"] >= least and want["ended"] + want["truncated"] == a.n_games, (where, out)
        assert_rollout(h.got, want, where, PER_MOVE)
        if a.tc:
            h.tc_before = a.tc_stats.cpu().numpy().copy()
            out.update(abs_equal=np.array_equal(h.acc_abs, h.host_abs), abs_any=bool(h.acc_abs.any()))
        return out

    def after_apply(a, h):
        if not a.tc:
            return {}
        E, A = a.coherence()
        return dict(host_tc=h.host_tc, tc=tuple((a.tc_stats.cpu().numpy() - h.tc_before).tolist()), E_equal=np.array_equal(bits(E), bits(coherence[0])),
                    A_equal=np.array_equal(bits(A), bits(coherence[1])))
    return learner_round(a, after_learn, after_apply, coherence=coherence)


def _assert_round(a, rec, where):
    assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["stats"] == rec["host"], (where, rec["stats"], rec["host"])
    assert rec["acc_adds"] == a.n_features * rec["host"]["learnt"] and rec["stats"]["skipped"] == rec["cut"] == rec["want_cut"], where
    assert rec["stats"]["learnt"] + rec["stats"]["skipped"] == rec["moves"] and rec["moved"] == rec["visited"] > 0, where
    if a.tc:
        assert rec["abs_equal"] and rec["abs_any"] and rec["E_equal"] and rec["A_equal"] and rec["tc"] == rec["host_tc"] + (0, 0), (where, rec["tc"], rec["host_tc"])


@functools.lru_cache(maxsize=None)
def _rounds(shape, symmetric, setting):
    a = learner_agent(extra_buffers=TC_STATE, tuples=SHAPES[shape], symmetric=symmetric, seed=LEARNER_SEED.get((shape, symmetric), SEED), **SETTINGS[setting])
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if a.tc else None
    recs = [_round(a, coherence, (shape, symmetric, setting, r)) for r in range(ROUNDS)]
    guards_intact(a)
    return a, recs


@pytest.mark.parametrize("setting", list(SETTINGS))
@SYMMETRIC
@pytest.mark.parametrize("shape", ["eight", "one6"])
def test_three_rounds_equal_the_host_at_every_shape(shape, symmetric, setting):
    """The learners' regime (257 games of at most 256 moves, epsilon .25, from zero weights) on "eight" and "one6": per round the
    roll-out, acc over all W, the counters and the weights as float32 bit patterns, and with tc acc_abs, E, A and tc_stats.
    Rehearsed on the host, games ended / cut per round (none capped; round 0 is the same games in every setting of a seed):
      eight, symmetric, seed 457: TD(0) 241/16 160/97 135/122 (40,212, 57,863 and 58,281 moves); lambda .5, with tc or without,
        241/16 157/100 115/142 (40,212, 57,525, 60,898)
      eight, one image, seed 457: TD(0) 241/16 225/32 220/37 (40,212, 47,208, 47,954); lambda .5 241/16 233/24 225/32 (40,212, 43,635, 45,799)
      one6, symmetric, seed 457: TD(0) 241/16 206/51 182/75 (40,212, 52,368, 55,034); lambda .5 241/16 211/46 205/52 (40,212, 50,832, 52,956)
      one6, one image, seed 613: TD(0) 242/15 245/12 245/12 (40,196, 40,947, 39,982); lambda .5 242/15 245/12 248/9 (40,196, 37,616, 36,397)"""
    a, recs = _rounds(shape, symmetric, setting)
    print([{k: rec[k] for k in ("ended", "cut", "moves", "host", "visited")} for rec in recs])
    for r, rec in enumerate(recs):
        assert rec["ended"] >= 8 and rec["cut"] >= 8 and rec["want_capped"] == 0, (r, rec["ended"], rec["cut"])
        _assert_round(a, rec, (shape, symmetric, setting, r))
    assert recs[2]["values_any"] and not recs[0]["values_any"]


def test_one_round_of_the_default_network_equals_the_host():
    """The shipping network's learn and apply launches held to the host once: TD(0), symmetric, one round of 65 games of at most 256
    moves at seed 457.  acc is 539 MB on each side; on an MI355X the case took 0.54 s (one run).  Rehearsed on the host: 58 games end and
    7 are cut in 10,302 moves, none capped."""
    start = time.perf_counter()
    a = learner_agent(65, tuples=SHAPES["default"])
    assert a.n_weights == 33685504 and a.n_features == 32
    rec = _round(a, None, "default", least=1)
    print("default network, one round:", {k: rec[k] for k in ("ended", "cut", "moves", "host", "visited")}, "wall s", time.perf_counter() - start)
    _assert_round(a, rec, "default")
    guards_intact(a)


# ------------------------------------------------------------------ 3. the evaluations at every shape
def _late_agent(shape, symmetric, epsilon, **kw):
    """an agent of LATE's shape on the shape's tuples, every buffer between guard words; the caller uploads its weights"""
    games, max_steps, seed = LATE
    return search_agent(games, max_steps, seed, "seeded", symmetric, tuples=SHAPES[shape], epsilon=epsilon, **kw)


@pytest.mark.parametrize("epsilon", [0.0, .25])
@pytest.mark.parametrize("shape", ["eight", "default"])
def test_the_evaluations_play_the_hosts_games_at_every_shape(shape, epsilon):
    """pulse_tfe_nt_evaluate and pulse_tfe_nt_evaluate_search, 65 games of at most 96 moves from reset: the per-game scores and
    lengths, the 8 summary words and the 16 bins.  "eight" on the weights its three symmetric TD(0) rounds left, "default" on its
    seeded weights / 64.  Rehearsed on the host, games ended / cut (moves), none capped -- 96 moves from reset end few games:
      eight, epsilon 0: one ply 1/64 (6,232), search 0/65 (6,240); epsilon .25: 0/65 and 0/65 (6,240 each)
      default, epsilon 0: one ply 4/61 (6,184), search 0/65 (6,240); epsilon .25: 8/57 (6,152) and 0/65 (6,240)"""
    import torch
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    (games, max_steps, seed), tuples = LATE, SHAPES[shape]
    w = _rounds("eight", True, "td0")[0].weights() if shape == "eight" else _small_weights(shape)
    assert w.any()
    args = (games, max_steps, epsilon, 1.0, w, tuples, True, *_seeds(seed), BOARD_ID0, ROUND)
    a = _late_agent(shape, True, epsilon)
    a.weights_dev.copy_(torch.from_numpy(w.copy()))
    for name, want, play in (("one ply", nt_games_on_host(*args), a.evaluate), ("search", nt_games_on_host(*args, depth=1, record=False), a.evaluate_search)):
        assert want["ended"] + want["truncated"] == games and int(want["lengths"].sum()) > 32 * games, name
        ev = play(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
        assert np.array_equal(ev["total_score"], want["total_score"]) and np.array_equal(ev["lengths"], want["lengths"]), name
        words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
        assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words, name
        assert (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0), name
    guards_intact(a)


# ------------------------------------------------------------------ 4. late-game boards and the cap, in games
LATE_CASES = [(shape, mode, True) for shape in ("eight", "default") for mode in MODES] + [("one6", "one_ply", False)]
LEARN_CASES = [case + ("td0",) for case in LATE_CASES] + [("eight", mode, True, "lambda.5-tc") for mode in MODES]


@functools.lru_cache(maxsize=None)
def _late_games(shape, mode, symmetric):
    """The host's games from late_start(65, 3), with what they are asserted to hold: at least 8 capped games, 8 ended ones and 8 cut at
    max_steps without a 32,768 tile; nibble 15 in recorded afterstates; a capped game whose last byte has no terminal bit.  Returns
    (the games, the `start` the launch is to leave, bool[B]: the capped games)."""
    (games, max_steps, seed), (layers, backed) = LATE, MODES[mode]
    start = late_start(games, 3)
    want = nt_games_on_host(games, max_steps, LATE_EPSILON[layers], 1.0, _small_weights(shape), SHAPES[shape], symmetric, *_seeds(seed), BOARD_ID0, ROUND,
                            depth=layers, backed=backed, start=start)
    left = want["start_left"]
    L, rows = want["lengths"].astype(np.int64), np.arange(games)
    played = np.arange(max_steps)[:, None] < L[None, :]
    fifteen = (_nibbles(want["keys"]) == 15).any(axis=2) & played
    capped = fifteen[L - 1, rows]                                          # a game stops at its first 32,768 tile: only its last afterstate holds one
    last = want["steps"][L - 1, rows]
    where = (shape, mode, symmetric, want["ended"], want["truncated"], want["capped"])
    assert int(capped.sum()) == want["capped"] == int(fifteen.sum()) >= 8 and want["ended"] >= 8 and want["ended"] + want["truncated"] == games, where
    assert int(((L == max_steps) & ~capped & (last >> 7 == 0)).sum()) >= 8 and (capped & (last >> 7 == 0)).any() and (L[capped] < max_steps).any(), where
    assert int(np.count_nonzero(left)) == 49 and np.array_equal(left, start) and int((L >= 3).sum()) >= 32, where
    return want, left, capped


@pytest.mark.parametrize("shape,mode,symmetric,learner", LEARN_CASES, ids=["-".join((s, m, l)) for s, m, _, l in LEARN_CASES])
def test_late_games_and_the_cap_are_the_hosts(shape, mode, symmetric, learner):
    """pulse_tfe_nt_rollout_from on late_start(65, 3) (49 usable boards, 16 zeros) at 96 moves, seed 4242, on the seeded weights / 64:
    keys, values, steps, lengths, scores, backed, the counters, the `start` left behind and the rows beyond a game's length; then one
    learn and one apply launch on those records -- pulse_tfe_nt_learn, with "lambda.5-tc" pulse_tfe_nt_learn_tc and pulse_tfe_nt_apply_tc,
    and in the backed mode pulse_tfe_nt_learn_backed -- with two values of a game that is at least three moves long replaced by 10 and
    20,000 (tests/tfe_nt_support.py: worked_games), so that the clamp and the cap meet in one launch.
    Rehearsed on the host, games ended / cut / capped (moves; cut at move 96 without a 32,768 tile):
      eight: one ply 23/42/27 (1,933; 15), search and backed 19/46/30 (2,108; 16)
      default: one ply 27/38/26 (1,952; 12), search and backed 18/47/31 (2,223; 16)
      one6, one image, one ply: 24/41/25 (1,974; 16)"""
    import torch
    n, (layers, backed) = nt(), MODES[mode]
    want, left, capped = _late_games(shape, mode, symmetric)
    a = _late_agent(shape, symmetric, LATE_EPSILON[layers], **SETTINGS[learner])
    if backed and a.deltas is None:
        a.deltas = torch.zeros_like(a.values)                              # (what pulse_tfe_nt_learn_backed would allocate: here between guard words)
    guard(a, tuple(k for k in TC_STATE if getattr(a, k) is not None))
    a = _with_restart(a, backed)
    a.weights_dev.copy_(torch.from_numpy(_small_weights(shape).copy()))
    _set_start(a, late_start(LATE[0], 3))
    got = _launched(a, lambda: a.rollout_from_launch(layers, backed=backed))
    _assert_games(a, got, want, left, (shape, mode, symmetric), backed)
    # one learn and one apply launch on these records
    g = int(np.flatnonzero(want["lengths"] >= 3)[0])
    a.values[0, g], a.values[1, g] = 10.0, 20000.0
    if backed:
        a.backed[1, g] = 20000.0
    rec, policy, before = read(a, PER_MOVE), a.weights(), a.stats()
    a.backed_targets = backed
    a.learn()
    acc, st = a.acc.cpu().numpy(), a.stats()
    host_acc, host_abs = np.zeros_like(acc), np.zeros(a.n_weights, dtype=np.int64) if a.tc else None
    records = (rec["keys"], rec["values"].view(np.float64), rec["steps"], rec["lengths"].astype(np.int64), a.tuples, a.symmetric, a.gamma)
    if backed:
        host = n.learn_backed_nt_on_host(*records[:2], a.backed.cpu().numpy(), *records[2:], a.lam, host_acc, host_abs)
    elif a.tc:
        host = n.learn_tc_nt_on_host(*records, a.lam, host_acc, host_abs)
    else:
        host = n.learn_nt_on_host(*records, host_acc)
    stats = {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")}
    print((shape, mode, symmetric, learner), "ended / cut / capped", want["ended"], want["truncated"], want["capped"], "learn", stats)
    assert host["skipped"] == want["truncated"] >= int(capped.sum()) >= 8 and host["clamped"] >= 2 and host["learnt"] + host["skipped"] == got["moves"]
    assert stats == {k: host[k] for k in stats} and np.array_equal(acc, host_acc) and acc[:, 1].sum() == a.n_features * host["learnt"]
    if a.tc:
        assert np.array_equal(a.acc_abs.cpu().numpy(), host_abs) and host_abs.any()
    if a.deltas is not None:
        played = np.arange(a.max_steps)[:, None] < rec["lengths"][None, :]
        assert np.array_equal(bits(a.deltas.cpu().numpy())[played], bits(host["deltas"])[played])
    a.apply()
    host_w = policy.copy()
    if a.tc:
        E, A = np.zeros(a.n_weights), np.zeros(a.n_weights)
        moved = n.apply_tc_nt_on_host(host_w, host_acc, host_abs, E, A, a.alpha / a.n_features)
        got_E, got_A = a.coherence()
        assert np.array_equal(bits(got_E), bits(E)) and np.array_equal(bits(got_A), bits(A)) and tuple(a.tc_stats.cpu().tolist()) == moved + (0, 0)
        assert moved[1] == moved[0] << 32 and not a.acc_abs.any().item()
    else:
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0
    assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)) and not a.acc.any().item()
    assert (a.weights().view(np.uint32) != policy.view(np.uint32)).any()
    after = read(a, PER_MOVE)
    assert all(np.array_equal(after[k], rec[k]) for k in PER_MOVE + PER_GAME)                  # the learners only read the records
    guards_intact(a)


# ------------------------------------------------------------------ 5. the default network's sibling check
def test_with_a_start_of_zeros_the_default_network_plays_its_sibling():
    """pulse_tfe_nt_rollout_from with `start` all zero and pulse_tfe_nt_rollout on the same struct of the default network: every output,
    byte for byte (tests/test_tfe_nt_restart_gpu.py has the check on its own network).  65 games of at most 96 moves at epsilon .05, seed
    4242, on the seeded weights / 64; rehearsed on the host: 8 games end and 57 are cut in 6,113 moves."""
    import torch
    a, b = (_with_restart(_late_agent("default", True, LATE_EPSILON[0])) for _ in range(2))
    for agent in (a, b):
        agent.weights_dev.copy_(torch.from_numpy(_small_weights("default").copy()))
    a.start.zero_()
    a.rollout_from_launch(0)
    b._launch("pulse_tfe_nt_rollout", b._rollout_struct())
    for k in ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters"):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k
    assert not a.start.any().item() and (_start_of(b) == np.uint64(START_PATTERN)).all()
    assert int(a.lengths.min().item()) < LATE[1] == int(a.lengths.max().item()) and a.stats()["moves"] == int(a.lengths.sum().item()) > 0
    guards_intact(a, b)
