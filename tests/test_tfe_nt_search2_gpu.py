"""The 2048 n-tuple network's expectimax play two chance layers deep on the device (DESIGN.md section 13.4;
csrc/tfe_ntuple_search.hip: pulse_tfe_nt_search_deep, pulse_tfe_nt_evaluate_search_deep) against the host's statement of it
(search_nt_on_host(layers=2); tests/tfe_nt_host.py: the oracle's environment under it).  Every comparison is exact: integers word
for word, float64 as bit patterns.  Every buffer a launch is handed sits between guard words.

Shape: the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), weights all zero or a seeded normal array of scale 4, gamma 1.  The kernels
take one board or game per workgroup, so no batch size leaves a workgroup partly filled: every board and game below is a workgroup of
its own.  7 games of at most 160 moves, chosen on the host from 7 games of 96 moves upwards (at 96 moves at most one game ended under
any of 15 seeds; seed 5 is the first of those tried that holds at 160): on the seeded weights at epsilon 0 (games end at moves 139,
146, 158), at epsilon .25 (75, 78, 79, 130, 158) and without symmetry at epsilon .25 (78, 108, 128, 129) at least two games end, no
two of them equally long, and at least two are cut at move 160.  On ZERO weights the two-layer search plays too well for that, at
epsilon .25 as at epsilon 0: no game of the 7 ended within 192 moves under any of five seeds tried, the mirror already takes half a
minute per such case at 160 moves, and the games' mean length under this policy is several hundred moves.  Those two cases check the
cut games and whatever ends.  The host's games are played once per case and shared (about 10 s per case on seeded weights)."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import guarded, guards_intact
from tests.tfe_nt_support import BOARD_ID0, CRAFTED, MORE, TUPLES, search_agent, search_outputs, weights
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_search_host import key_of

pytestmark = pytest.mark.gpu
GAMES, MAX_STEPS, EPSILON = 7, 160, .25
SEED, ROUND = 5, 0
CASES = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("zero", EPSILON, True), ("zero", 0.0, True), ("seeded", EPSILON, False))
_agent = functools.partial(search_agent, GAMES, MAX_STEPS, SEED)


@functools.lru_cache(maxsize=None)
def _host_games(name, epsilon, symmetric=True):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return nt_games_on_host(GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0,
                            ROUND, depth=2, record=False, keep_boards="before")


@functools.lru_cache(maxsize=None)
def _boards():
    """uint64[9 + 3 * GAMES]: the crafted boards, then move 2, the middle move and the last move of every host game on the seeded
    weights at epsilon .25"""
    from tests.tfe_host import pack_boards
    games = _host_games("seeded", EPSILON)
    L, rows = games["lengths"], np.arange(GAMES)
    middle = np.stack([games["boards"][int(L[g]) // 2][g] for g in rows])
    late = np.stack([games["boards"][int(L[g]) - 1][g] for g in rows])
    keys = np.concatenate([np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64),
                           pack_boards(games["boards"][2]), pack_boards(middle), pack_boards(late)])
    assert keys.shape == (len(CRAFTED) + len(MORE) + 3 * GAMES,) and L.min() > 4
    keys.setflags(write=False)
    return keys


def _n_empty(keys):
    return ((keys[:, None] >> (np.uint64(4) * np.arange(16, dtype=np.uint64))) & np.uint64(15) == 0).sum(axis=1)


# ------------------------------------------------------------------ boards, bit for bit
@pytest.mark.parametrize("name,symmetric", [("zero", True), ("seeded", True), ("seeded", False)])
def test_search_equals_the_mirror_bit_for_bit(name, symmetric):
    import torch
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a, keys = _agent(name, symmetric), _boards()
    a.round = 3                                                            # (the coins of another round than the games')
    want = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, a.gamma, a.tie_seed, a.round, layers=2)
    dev = torch.device("cuda:0")
    boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    q, action, cand, guards = search_outputs(len(keys), dev)
    a.search_launch(boards, q, action, cand, layers=2)
    got_q = q.cpu().numpy()
    assert np.array_equal(cand.cpu().numpy(), want["candidates"]) and np.array_equal(action.cpu().numpy().astype(np.int64), want["action"])
    assert np.array_equal(got_q.view(np.uint64), want["q"].view(np.uint64))
    assert np.array_equal(boards.cpu().numpy().view(np.uint64), keys)
    guards_intact(a, [("boards", gb, nb)] + guards)
    # what the comparison exercised
    names = list(CRAFTED) + list(MORE)
    assert int(want["action"][names.index("dead")]) == -1 and int(want["candidates"][names.index("over_after_spawn")]) == 0
    empty = _n_empty(keys)
    assert empty[names.index("fourteen_empty")] == 14 and empty[names.index("one_empty")] == 1 and empty.max() == 15 and (empty == 0).sum() >= 3
    assert (want["action"] >= 0).sum() >= len(keys) - 2 and len(set(want["candidates"].tolist())) >= 6
    one = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, a.gamma, a.tie_seed, a.round)
    assert (want["q"] != one["q"]).any(axis=1).sum() >= len(keys) - 4       # the second layer enters
    best = np.where(want["candidates"][:, None] >> np.arange(4) & 1, want["q"], -np.inf)
    ties = ((best == best.max(axis=1, keepdims=True)) & np.isfinite(best)).sum(axis=1) >= 2
    if name == "zero":
        assert ties[names.index("corner")] and ties.sum() >= 2              # the coins decide there
        coins = nt.philox_many_on_host(a.tie_seed, keys[ties], a.round)
        assert len({int(w) >> 31 for w in coins[:, :3].ravel()}) == 2       # ... both ways
    else:
        assert np.unique(want["q"]).size > 2 * len(keys)
    # the public method: the same launch on tensors of its own
    out = a.search(keys, layers=2)
    assert np.array_equal(out["q"].view(np.uint64), want["q"].view(np.uint64)) and out["action"].dtype == np.int8 and out["candidates"].dtype == np.uint8
    assert np.array_equal(out["action"], want["action"]) and np.array_equal(out["candidates"], want["candidates"])


def test_one_layer_through_the_deep_entry_point_is_the_search():
    """device against device, the same boards: pulse_tfe_nt_search_deep at layers = 1 and pulse_tfe_nt_search"""
    import torch
    a, keys, dev = _agent("seeded"), _boards(), torch.device("cuda:0")
    boards = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    q0, action0, cand0, guards0 = search_outputs(len(keys), dev)
    q1, action1, cand1, guards1 = search_outputs(len(keys), dev)
    a.search_launch(boards, q0, action0, cand0)
    a._launch("pulse_tfe_nt_search_deep", a._search_struct(boards, q1, action1, cand1), 1)
    assert torch.equal(q0.view(torch.int64), q1.view(torch.int64)) and torch.equal(action0, action1) and torch.equal(cand0, cand1)
    assert int((action0 >= 0).sum()) >= len(keys) - 2 and q0.abs().sum() > 0
    guards_intact(a, guards0, guards1)


# ------------------------------------------------------------------ games, word for word
def test_the_hosts_games_end_and_are_cut():
    """no GPU work: what the games below exercise (module docstring)"""
    for name, epsilon, symmetric in CASES:
        want = _host_games(name, epsilon, symmetric)
        L = want["lengths"]
        ended = L[L < MAX_STEPS]
        assert want["truncated"] >= 2 and want["capped"] == 0 and want["ended"] + want["truncated"] == GAMES, (name, epsilon)
        assert len(set(ended.tolist())) == len(ended), (name, epsilon, sorted(L.tolist()))
        if name != "zero":
            assert want["ended"] >= 2 and want["ended"] == len(ended), (name, epsilon, want["ended"])


@pytest.mark.parametrize("name,epsilon,symmetric", CASES)
def test_games_equal_the_hosts_word_for_word(name, epsilon, symmetric):
    """lengths, scores, the 24 counters (the largest-tile histogram among them)"""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, want = _agent(name, symmetric), _host_games(name, epsilon, symmetric)
    ev = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True, layers=2)
    assert np.array_equal(ev["lengths"], want["lengths"]) and np.array_equal(ev["total_score"], want["total_score"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words
    assert ev["games"] == GAMES and (ev["moves_greedy"] == ev["moves"]) == (epsilon == 0.0) and sum(ev["max_tile_hist"]) == GAMES
    guards_intact(a)


def test_one_layer_through_the_deep_entry_point_is_the_search_evaluation():
    """the same board_id0, every key: pulse_tfe_nt_evaluate_search_deep at layers = 1 and pulse_tfe_nt_evaluate_search"""
    a = _agent("seeded")
    one = a.evaluate_search(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True)
    deep = a._evaluate_with(a._entry("pulse_tfe_nt_evaluate_search_deep", 1), None, EPSILON, BOARD_ID0, True)
    assert sorted(one) == sorted(deep) and one["moves"] > GAMES
    for k in one:
        assert np.array_equal(one[k], deep[k]) if k in ("total_score", "lengths") else one[k] == deep[k], k
    guards_intact(a)


@pytest.mark.parametrize("epsilon", [0.0, EPSILON])
def test_gamma_zero_is_the_one_ply_evaluation(epsilon):
    a = _agent("seeded", gamma=0.0)
    one = a.evaluate(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True)
    two = a.evaluate_search(epsilon=epsilon, board_id0=BOARD_ID0, per_game=True, layers=2)
    assert sorted(one) == sorted(two) and one["moves"] > GAMES
    for k in one:
        assert np.array_equal(one[k], two[k]) if k in ("total_score", "lengths") else one[k] == two[k], k
    guards_intact(a)


# ------------------------------------------------------------------ the score
def test_two_layers_play_no_worse():
    """The default network after two rounds of 4,096 games (as test_search_plays_no_worse trains it), then 256 games from the default
    evaluation boards under one and under two chance layers, paired by board: the mean of (two - one) is at least -3 standard errors of
    that difference.  It catches a deeper search that plays worse; it is no claim about the gain.  On an MI355X (one run): one layer
    13,499.2 +- 347.3 (mean length 797.3), two layers 19,693.9 +- 518.2 (1,088.2), difference +6,194.8 +- 620.1; the two-layer
    evaluation took 317 ms with its read-back, far below 10 s, so the 256 games were not halved."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0)
    a.learn_batch().learn_batch()
    one = a.evaluate_search(n_games=256, per_game=True)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    two = a.evaluate_search(n_games=256, per_game=True, layers=2)
    stop.record()
    stop.synchronize()
    se = lambda e: e["std_score"] / e["games"] ** .5
    diff = (two["total_score"] - one["total_score"]).astype(np.float64)
    se_diff = diff.std(ddof=1) / np.sqrt(diff.size)
    print("256 games after two rounds: one layer", one["mean_score"], "+-", se(one), "two layers", two["mean_score"], "+-", se(two), "difference",
          diff.mean(), "+-", se_diff, "mean lengths", one["mean_length"], two["mean_length"], "two-layer evaluation with its read-back, ms",
          start.elapsed_time(stop))
    assert one["games"] == two["games"] == 256
    assert diff.mean() >= -3.0 * se_diff, (one["mean_score"], two["mean_score"], se_diff)
