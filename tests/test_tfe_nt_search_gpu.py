"""The 2048 n-tuple network's expectimax play on the device (csrc/tfe_ntuple_search.hip: pulse_tfe_nt_search,
pulse_tfe_nt_evaluate_search) against the host's statement of it (search_nt_on_host; tests/tfe_nt_host.py: the oracle's environment
under it).  Every comparison is exact: integers word for word, float64 as bit patterns.  Every buffer a launch is handed sits between
guard words.

Shape: the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), weights all zero or a seeded normal array of scale 4 (V of the order of the
rewards), gamma 1.  73 boards = nine workgroups of eight groups and one group.  17 games of at most 192 moves = two workgroups and one
group.  Chosen on the host (seed SEED): on the seeded weights, at epsilon 0 and .25, and on zero weights at epsilon .25 the 17 games
hold at least two that end and at least two that are cut, and no two games that end are equally long (the games of a wavefront leave
their loop at different moves); the cut games are all as long as max_steps by definition.  On zero weights at epsilon 0 the search
plays too well for 192 moves to end two games under any of 350 seeds tried (one game ends under this one): that case checks the cut games and whatever ends."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import guarded, guards_intact
from tests.tfe_nt_support import BOARD_ID0, CRAFTED, TUPLES, search_agent, search_outputs, weights
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_search_host import key_of

pytestmark = pytest.mark.gpu

GAMES, MAX_STEPS, BOARDS, EPSILON = 17, 192, 73, .25
SEED, ROUND = 2312, 0
_agent = functools.partial(search_agent, GAMES, MAX_STEPS, SEED)


@functools.lru_cache(maxsize=None)
def _host_games(name, epsilon, symmetric=True, keep_boards=None):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return nt_games_on_host(GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0, ROUND,
                            depth=1, record=False, keep_boards=keep_boards)


@functools.lru_cache(maxsize=None)
def _boards():
    """uint64[73]: the crafted boards, then boards of the host's games on the seeded
    weights at epsilon .25 (move 1, the middle move and the last move of every game), and move 150 of the 14 longest games on zero weights"""
    from tests.tfe_host import pack_boards
    games = _host_games("seeded", EPSILON, True, "before")
    L, rows = games["lengths"], np.arange(GAMES)
    middle = np.stack([games["boards"][int(L[g]) // 2][g] for g in rows])
    late = np.stack([games["boards"][int(L[g]) - 1][g] for g in rows])
    zero = _host_games("zero", 0.0, True, "before")
    longest = np.argsort(-zero["lengths"], kind="stable")[:14]
    assert (zero["lengths"][longest] > 150).all() and L.min() > 2
    keys = np.concatenate([np.array([key_of(c) for c in CRAFTED.values()], dtype=np.uint64), pack_boards(games["boards"][1]), pack_boards(middle),
                           pack_boards(late), pack_boards(zero["boards"][150][longest])])
    assert keys.shape == (BOARDS,)
    keys.setflags(write=False)
    return keys


@pytest.mark.parametrize("name,symmetric", [("zero", True), ("seeded", True), ("seeded", False)])
def test_search_equals_the_mirror_bit_for_bit(name, symmetric):
    import torch
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a, keys = _agent(name, symmetric), _boards()
    a.round = 3                                                            # (the coins of another round than the games')
    want = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, a.gamma, a.tie_seed, a.round)
    dev = torch.device("cuda:0")
    boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    q, action, cand, guards = search_outputs(BOARDS, dev)
    a.search_launch(boards, q, action, cand)
    got_q = q.cpu().numpy()
    assert np.array_equal(cand.cpu().numpy(), want["candidates"]) and np.array_equal(action.cpu().numpy().astype(np.int64), want["action"])
    assert np.array_equal(got_q.view(np.uint64), want["q"].view(np.uint64))
    assert np.array_equal(boards.cpu().numpy().view(np.uint64), keys)
    guards_intact(a, [("boards", gb, nb)] + guards)
    # what the comparison exercised
    names = list(CRAFTED)
    assert int(want["action"][names.index("dead")]) == -1 and int(want["candidates"][names.index("over_after_spawn")]) == 0
    assert (want["action"] >= 0).sum() >= BOARDS - 2 and len(set(want["candidates"].tolist())) >= 6
    best = np.where(want["candidates"][:, None] >> np.arange(4) & 1, want["q"], -np.inf)
    ties = ((best == best.max(axis=1, keepdims=True)) & np.isfinite(best)).sum(axis=1) >= 2
    if name == "zero":
        assert ties[names.index("corner")] and ties.sum() >= 2              # the coins decide there
        coins = nt.philox_many_on_host(a.tie_seed, keys[ties], a.round)
        assert len({int(w) >> 31 for w in coins[:, :3].ravel()}) == 2       # ... both ways
    else:
        assert np.unique(want["q"]).size > 2 * BOARDS and (want["q"] < 0).any()
    # the public method: the same launch on tensors of its own
    out = a.search(keys)
    assert np.array_equal(out["q"].view(np.uint64), want["q"].view(np.uint64)) and out["action"].dtype == np.int8 and out["candidates"].dtype == np.uint8
    assert np.array_equal(out["action"], want["action"]) and np.array_equal(out["candidates"], want["candidates"])


def test_the_hosts_games_end_and_are_cut():
    """no GPU work: what the games below exercise (module docstring)"""
    for name, epsilon in (("seeded", 0.0), ("seeded", EPSILON), ("zero", EPSILON), ("zero", 0.0)):
        want = _host_games(name, epsilon)
        L = want["lengths"]
        ended = L[L < MAX_STEPS]
        assert want["truncated"] >= 2 and want["capped"] == 0 and want["ended"] + want["truncated"] == GAMES, (name, epsilon)
        assert len(set(ended.tolist())) == len(ended), (name, epsilon, sorted(L.tolist()))
        if (name, epsilon) != ("zero", 0.0):
            assert want["ended"] >= 2 and want["ended"] == len(ended), (name, epsilon, want["ended"])


@pytest.mark.parametrize("epsilon", [0.0, EPSILON])
@pytest.mark.parametrize("name", ["seeded", "zero"])
def test_games_equal_the_hosts_word_for_word(name, epsilon):
    """scores, lengths and the 24 counters"""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, want = _agent(name), _host_games(name, epsilon)
    ev = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
    assert np.array_equal(ev["lengths"], want["lengths"]) and np.array_equal(ev["total_score"], want["total_score"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words
    assert ev["games"] == GAMES and (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0) and sum(ev["max_tile_hist"]) == GAMES
    guards_intact(a)


def test_games_without_symmetry():
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, want = _agent("seeded", False), _host_games("seeded", EPSILON, False)
    ev = a.evaluate_search(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True)
    assert np.array_equal(ev["lengths"], want["lengths"]) and np.array_equal(ev["total_score"], want["total_score"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == eval_words(want["total_score"], want["lengths"], want["final_boards"],
                                                                             want["truncated"], want["greedy"], want["capped"])
    guards_intact(a)


@pytest.mark.parametrize("epsilon", [0.0, EPSILON])
def test_gamma_zero_is_the_one_ply_evaluation(epsilon):
    a = _agent("seeded", gamma=0.0)
    one = a.evaluate(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
    two = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
    assert sorted(one) == sorted(two) and one["moves"] > GAMES
    for k in one:
        assert np.array_equal(one[k], two[k]) if k in ("total_score", "lengths") else one[k] == two[k], k
    assert a.evaluate_search(n_games=9) == a.evaluate(n_games=9)            # the defaults: the same boards for both policies
    guards_intact(a)


def test_search_plays_no_worse():
    """The default network after two rounds of 4,096 games (as test_it_learns trains it), then 1,024 games from the default evaluation
    boards under both policies, paired by board: the mean of (search - one-ply) is at least -3 standard errors of that difference.  It
    catches a search that plays worse; it is no claim about the gain.  Rehearsed on the host (256 games per round, 128 evaluation
    games): one-ply 4,804 +- 211, search 11,228 +- 461, difference +6,424 +- 483.  On an MI355X: one-ply 6,640.7 +- 96.6, search 13,483.7 +- 174.3,
    difference +6,843.0 +- 197.3; the search evaluation took 65 ms with its read-back, so the 1,024 games were not halved."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0)
    a.learn_batch().learn_batch()
    one = a.evaluate(n_games=1024, per_game=True)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    two = a.evaluate_search(n_games=1024, per_game=True)
    stop.record()
    stop.synchronize()
    se = lambda e: e["std_score"] / e["games"] ** .5
    diff = (two["total_score"] - one["total_score"]).astype(np.float64)
    se_diff = diff.std(ddof=1) / np.sqrt(diff.size)
    print("1,024 games after two rounds: one-ply", one["mean_score"], "+-", se(one), "search", two["mean_score"], "+-", se(two), "difference", diff.mean(),
          "+-", se_diff, "mean lengths", one["mean_length"], two["mean_length"], "search evaluation with its read-back, ms", start.elapsed_time(stop))
    assert one["games"] == two["games"] == 1024
    assert diff.mean() >= -3.0 * se_diff, (one["mean_score"], two["mean_score"], se_diff)
