"""The 2048 n-tuple network's expectimax play at a depth the board's empty cells choose, on the device (DESIGN.md section 13.11;
csrc/tfe_ntuple_search.hip: pulse_tfe_nt_search_adaptive, pulse_tfe_nt_evaluate_search_adaptive) against the host's statement
of it (search_adaptive_nt_on_host; tests/tfe_nt_host.py: the oracle's environment under it) and against the two searches it
chooses between.  Every comparison is exact: integers word for word, float64 as bit patterns.  Every buffer a launch is handed sits
between guard words, the two depth counters too.

Shape (tests/tfe_nt_adaptive_support.py, where the rehearsal is written down): the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), weights all
zero or a seeded normal array of scale 4, gamma 1, 7 games of at most 256 moves, E = 3.  The kernels take one board or game per
workgroup, so no batch size leaves a workgroup partly filled.  The host's games are played once per case and shared (about 2 s per
case: most moves are one layer deep)."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import guard, guarded, guards_intact
from tests.tfe_nt_adaptive_support import CASES, DEEP_EMPTY_MAX, EPSILON, GAMES, MAX_STEPS, SEED, host_games
from tests.tfe_nt_support import BOARD_ID0, CRAFTED, MORE, TUPLES, search_agent, search_outputs, weights
from tests.tfe_search_host import key_of

pytestmark = pytest.mark.gpu
E = DEEP_EMPTY_MAX
SEARCH, EVALUATE = "pulse_tfe_nt_search_adaptive", "pulse_tfe_nt_evaluate_search_adaptive"
DEPTHS = ("moves_deep", "moves_shallow")


def _agent(name, symmetric=True, **kw):
    """the agent of the shape, every device buffer between guard words: the depth counters too, which the agent would allocate itself"""
    import torch
    a = search_agent(GAMES, MAX_STEPS, SEED, name, symmetric, **kw)
    a.depth_stats = torch.zeros(2, dtype=torch.int64, device=a.device)
    a = guard(a, ("depth_stats",))
    assert a.depth_stats.data_ptr() % 8 == 0
    return a


@functools.lru_cache(maxsize=None)
def _boards():
    """uint64[9 + 3 * GAMES]: the crafted boards, then move 2, the middle move and the last move of every host game on the seeded
    weights at epsilon .25"""
    from tests.tfe_host import pack_boards
    games = host_games("seeded", EPSILON, True)
    L, rows = games["lengths"], np.arange(GAMES)
    middle = np.stack([games["boards"][int(L[g]) // 2][g] for g in rows])
    late = np.stack([games["boards"][int(L[g]) - 1][g] for g in rows])
    keys = np.concatenate([np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64),
                           pack_boards(games["boards"][2]), pack_boards(middle), pack_boards(late)])
    assert keys.shape == (len(CRAFTED) + len(MORE) + 3 * GAMES,) and L.min() > 4
    keys.setflags(write=False)
    return keys


def _launch_boards(a, keys, entry, *args):
    """(q, action, candidates) on the host after one launch of `entry` on `keys`, with all four buffers' guard words checked"""
    import torch
    dev = torch.device("cuda:0")
    boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    q, action, cand, guards = search_outputs(len(keys), dev)
    a._launch(entry, a._search_struct(boards, q, action, cand), *args)
    out = q.cpu().numpy(), action.cpu().numpy().astype(np.int64), cand.cpu().numpy()
    assert np.array_equal(boards.cpu().numpy().view(np.uint64), keys)
    guards_intact(a, [("boards", gb, nb)] + guards)
    return out


def _same(got, want, skip=()):
    assert sorted(k for k in got if k not in skip) == sorted(k for k in want if k not in skip)
    for k in want:
        if k not in skip:
            assert np.array_equal(got[k], want[k]) if k in ("total_score", "lengths") else got[k] == want[k], k


# ------------------------------------------------------------------ boards, bit for bit
@pytest.mark.parametrize("name,symmetric", [("zero", True), ("seeded", True), ("seeded", False)])
def test_search_equals_the_mirror_bit_for_bit(name, symmetric):
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a, keys = _agent(name, symmetric), _boards()
    a.round = 3                                                            # (the coins of another round than the games')
    want = nt.search_adaptive_nt_on_host(keys, weights(name), TUPLES, symmetric, a.gamma, a.tie_seed, a.round, E)
    got_q, got_action, got_cand = _launch_boards(a, keys, SEARCH, E)
    assert np.array_equal(got_cand, want["candidates"]) and np.array_equal(got_action, want["action"])
    assert np.array_equal(got_q.view(np.uint64), want["q"].view(np.uint64))
    # what the comparison exercised: both depths, the shallow boards bit for bit the one-layer search's, the deep ones not
    deep = want["deep"]
    assert np.array_equal(deep, nt.count_empty_on_host(keys) <= E) and deep.sum() >= 5 and (~deep).sum() >= 5
    one = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, a.gamma, a.tie_seed, a.round)
    assert np.array_equal(got_q[~deep].view(np.uint64), one["q"][~deep].view(np.uint64)) and np.array_equal(got_action[~deep], one["action"][~deep])
    assert (got_q[deep] != one["q"][deep]).any()
    names = list(CRAFTED) + list(MORE)
    assert int(want["action"][names.index("dead")]) == -1 and int(want["candidates"][names.index("over_after_spawn")]) == 0
    assert (want["action"] >= 0).sum() >= len(keys) - 2 and len(set(want["candidates"].tolist())) >= 6
    # the public method: the same launch on tensors of its own
    out = a.search(keys, layers=2, deep_empty_max=E)
    assert np.array_equal(out["q"].view(np.uint64), want["q"].view(np.uint64)) and out["action"].dtype == np.int8 and out["candidates"].dtype == np.uint8
    assert np.array_equal(out["action"], want["action"]) and np.array_equal(out["candidates"], want["candidates"])
    guards_intact(a)


def test_sixteen_is_the_two_layer_search_and_zero_is_the_mirror():
    """E = 16: device against device on the same boards, pulse_tfe_nt_search_deep at layers = 2; E = 0: two layers on the full boards
    alone, against the mirror"""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a, keys = _agent("seeded"), _boards()
    q16, action16, cand16 = _launch_boards(a, keys, SEARCH, 16)
    q2, action2, cand2 = _launch_boards(a, keys, "pulse_tfe_nt_search_deep", 2)
    assert np.array_equal(q16.view(np.uint64), q2.view(np.uint64)) and np.array_equal(action16, action2) and np.array_equal(cand16, cand2)
    assert (action2 >= 0).sum() >= len(keys) - 2 and np.abs(q2).sum() > 0
    want = nt.search_adaptive_nt_on_host(keys, weights("seeded"), TUPLES, True, a.gamma, a.tie_seed, a.round, 0)
    q0, action0, cand0 = _launch_boards(a, keys, SEARCH, 0)
    assert np.array_equal(q0.view(np.uint64), want["q"].view(np.uint64)) and np.array_equal(action0, want["action"]) and np.array_equal(cand0, want["candidates"])
    assert want["deep"].sum() >= 3 and (q0 != q2).any()


# ------------------------------------------------------------------ games, word for word
@pytest.mark.parametrize("name,epsilon,symmetric", CASES)
def test_games_equal_the_hosts_word_for_word(name, epsilon, symmetric):
    """lengths, scores, the 24 counters (the largest-tile histogram among them) and the moves at each depth"""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, want = _agent(name, symmetric), host_games(name, epsilon, symmetric)
    ev = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True, layers=2, deep_empty_max=E)
    assert np.array_equal(ev["lengths"], want["lengths"]) and np.array_equal(ev["total_score"], want["total_score"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words
    assert (ev["moves_deep"], ev["moves_shallow"]) == (want["deep"], want["shallow"]) and ev["moves_deep"] + ev["moves_shallow"] == ev["moves"]
    assert ev["games"] == GAMES and (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0) and sum(ev["max_tile_hist"]) == GAMES
    guards_intact(a)


def test_a_null_depth_stats_leaves_everything_else_equal():
    """one direct launch with depth_stats = NULL beside the agent's own call"""
    a = _agent("seeded")
    mine = a.evaluate_search(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True, layers=2, deep_empty_max=E)
    counted = a.depth_stats.cpu().tolist()
    null = a._evaluate_with(a._entry(EVALUATE, E, None), None, EPSILON, BOARD_ID0, True)
    _same(null, mine, skip=DEPTHS)
    assert a.depth_stats.cpu().tolist() == counted == [mine[k] for k in DEPTHS] and mine["moves"] > GAMES and not set(DEPTHS) & set(null)
    # the launch alone only adds
    a.evaluate_search_launch(epsilon=EPSILON, board_id0=BOARD_ID0, layers=2, deep_empty_max=E)
    assert a.depth_stats.cpu().tolist() == [2 * c for c in counted]
    guards_intact(a)


def test_sixteen_is_the_two_layer_evaluation():
    """device against device, every key: 7 games capped at 96 moves, where two layers on every board stay affordable"""
    a = _agent("seeded")
    a.eval_max_steps = 96
    two = a.evaluate_search(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True, layers=2)
    all_deep = a.evaluate_search(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True, layers=2, deep_empty_max=16)
    _same(all_deep, two, skip=DEPTHS)
    assert (all_deep["moves_deep"], all_deep["moves_shallow"]) == (two["moves"], 0) and two["moves"] > GAMES
    guards_intact(a)


@pytest.mark.parametrize("epsilon", [0.0, EPSILON])
def test_gamma_zero_is_the_one_ply_evaluation(epsilon):
    a = _agent("seeded", gamma=0.0)
    one = a.evaluate(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
    mine = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True, layers=2, deep_empty_max=E)
    _same(mine, one, skip=DEPTHS)
    assert one["moves"] > GAMES and mine["moves_deep"] > 0 and mine["moves_shallow"] > 0 and mine["moves_deep"] + mine["moves_shallow"] == one["moves"]
    guards_intact(a)


# ------------------------------------------------------------------ the score
def test_the_adaptive_search_plays_no_worse_than_one_layer():
    """The default network after two rounds of 4,096 games (as test_two_layers_play_no_worse trains it), then 256 games from the default
    evaluation boards under one layer, under E = 3 and under two layers, paired by board: the mean of (E = 3 - one layer) is at least -3
    standard errors of that difference.  It catches a search that plays worse; it is no claim of a gain.  The three means, the deep
    share and the launch times between HIP events are printed for DESIGN.md section 13.11.  On an MI355X (one run): one layer
    13,499.2 +- 347.3 in 61.6 ms, E = 3 18,245.9 +- 463.4 in 74.1 ms with 20.6 % of 261,991 moves two layers deep, two layers
    19,693.9 +- 518.2 in 317.7 ms; E = 3 - one layer +4,746.8 +- 575.8, E = 3 - two layers -1,448.0 +- 696.1."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0)
    a.learn_batch().learn_batch()

    def timed(**kw):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.eval_counters(clear=True)
        start.record()
        arrays = a.evaluate_search_launch(n_games=256, per_game=True, **kw)
        stop.record()
        stop.synchronize()
        return dict(a.eval_counters(), total_score=arrays[0].cpu().numpy().astype(np.float64), ms=start.elapsed_time(stop))

    one, two = timed(layers=1), timed(layers=2)
    mine = timed(layers=2, deep_empty_max=E)
    deep, shallow = a.depth_stats.cpu().tolist()
    se = lambda e: e["std_score"] / e["games"] ** .5
    diff, diff2 = mine["total_score"] - one["total_score"], mine["total_score"] - two["total_score"]
    se_diff, se_diff2 = diff.std(ddof=1) / np.sqrt(diff.size), diff2.std(ddof=1) / np.sqrt(diff2.size)
    print("256 games after two rounds: one layer", one["mean_score"], "+-", se(one), "E = 3", mine["mean_score"], "+-", se(mine), "two layers",
          two["mean_score"], "+-", se(two), "E = 3 - one", diff.mean(), "+-", se_diff, "E = 3 - two", diff2.mean(), "+-", se_diff2, "deep share",
          deep / (deep + shallow), "of", deep + shallow, "moves; launch ms: one layer", one["ms"], "E = 3", mine["ms"], "two layers", two["ms"])
    assert one["games"] == mine["games"] == two["games"] == 256 and deep + shallow == mine["moves"] and deep > 0 and shallow > 0
    assert diff.mean() >= -3.0 * se_diff, (one["mean_score"], mine["mean_score"], se_diff)
