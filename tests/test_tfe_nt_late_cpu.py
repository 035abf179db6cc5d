"""The premises of tests/test_tfe_nt_late_gpu.py, computed with the host mirrors alone: the games of the late
regime on four stages, the search boards, the five continued rounds and the adaptive search's boards are made by
tests/tfe_nt_late_support.py, which asserts every floor where it makes them; the tests here call each case, assert what is derived from
them, and print the counts the GPU file's docstrings quote.  No GPU: a change of seeds, of late_start or of the staged weights that
empties a GPU test fails here first."""
import numpy as np
import pytest

from tests import tfe_nt_late_support as late
from tests.tfe_nt_staged_support import adds_per_stage, staged
from tests.tfe_nt_support import SHAPES, nt

# the GPU file's cases, "one6" with 8 images for the rehearsal's table, and the shipping network times four stages (its 134,742,016
# seeded weights take about 5 s to draw: the one slow case here)
HOST_CASES = sorted({(shape, symmetric, late.MODES[mode][0]) for shape, symmetric, mode in late.ROLLOUT_CASES} | {("one6", True, 0), ("default", True, 0)})
SEARCH_CASES = [("eight", True), ("eight", False), ("one6", True), ("one6", False)]


def _host_acc(shape, symmetric, g, steps):
    n, tuples = nt(), staged(SHAPES[shape], late.LATE_TILES)
    acc = np.zeros((late.S * n.tuple_offsets(tuples)[1], 2), dtype=np.int64)
    host = n.learn_nt_on_host(g.want["keys"], g.want["values"], steps, g.L, tuples, symmetric, 1.0, acc)
    return host, adds_per_stage(acc, late.S)


@pytest.mark.parametrize("shape,symmetric,layers", HOST_CASES)
def test_the_late_games_reach_every_stage_and_every_end(shape, symmetric, layers):
    g = late.late_games(shape, symmetric, layers)
    print("late games", (shape, symmetric, layers), "seed", g.seed, g.counts)
    assert sum(g.per_stage) == g.counts["moves"] and int((g.capped | g.dead | g.cut).sum()) == late.GAMES      # (a game can be capped and dead at once)
    assert late.late_games(shape, symmetric, layers) is g                   # made once per session


@pytest.mark.parametrize("shape,symmetric", [("eight", True), ("eight", False), ("one6", False)])
def test_stage_three_learns_only_where_a_capped_game_is_dead(shape, symmetric):
    """On the roll-out's own records the top slice gets no add: every capped game's last move is cut.  With the terminal bit set in
    every second of those bytes (with_dead_caps) each slice has adds, and the other capped games stay skipped."""
    g = late.late_games(shape, symmetric, 0)
    F = len(SHAPES[shape]) * (8 if symmetric else 1)
    host, per_stage = _host_acc(shape, symmetric, g, g.want["steps"])
    assert per_stage[3] == 0 and all(x > 0 for x in per_stage[:3]) and host["skipped"] == g.counts["capped"] + g.counts["cut"]
    steps, marked = late.with_dead_caps(g.want["steps"], g)
    host, marked_per_stage = _host_acc(shape, symmetric, g, steps)
    print("adds per stage", (shape, symmetric), per_stage, "->", marked_per_stage, "capped games learnt", len(marked))
    assert len(marked) >= 4 and marked_per_stage[3] == F * len(marked) and marked_per_stage[:3] == per_stage[:3]
    assert host["skipped"] == g.counts["capped"] + g.counts["cut"] - len(marked) >= late.FLOOR["capped"] + 4


def test_under_the_low_tiles_stage_zero_is_empty():
    g = late.late_games("eight", True, 0, late.LOW_TILES)
    print("late games under", late.LOW_TILES, g.counts)
    assert g.per_stage[0] == 0 and g.counts["capped"] >= 8


@pytest.mark.parametrize("tiles", [late.LATE_TILES, late.LOW_TILES], ids=["late_tiles", "low_tiles"])
@pytest.mark.parametrize("shape,symmetric", SEARCH_CASES)
def test_the_search_boards_straddle_the_thresholds(shape, symmetric, tiles):
    want, split = late.staged_search(shape, symmetric, tiles)
    print("search", (shape, symmetric, tiles), "boards with candidate afterstates in two stages", split)
    assert len(want["q"]) == 123 and (want["action"] >= 0).sum() >= 120 and np.unique(want["q"]).size > 123


@pytest.mark.parametrize("case", list(late.CONTINUE_CASES))
def test_the_continued_rounds_reach_the_picks_three_branches(case):
    rounds, counts = late.continued_rounds(case)
    games, K, layers, seed = late.CONTINUE_CASES[case]
    print("continued rounds", case, "seed", seed, counts, "capped per round", [int(r.capped.sum()) for r in rounds], "finished per round", [r.words[0] for r in rounds])
    assert sum(r.words[0] for r in rounds) == counts["finished"] and all(r.words[0] + r.words[5] == games for r in rounds)
    last = rounds[-1]
    assert int(last.cut.sum()) >= 8 and int(np.count_nonzero(last.start)) >= 8       # the learners' round: games taken up again, and cut again


@pytest.mark.parametrize("shape,symmetric", SEARCH_CASES)
def test_the_adaptive_search_takes_both_depths_on_the_late_boards(shape, symmetric):
    counts = late.adaptive_premises(shape, symmetric)
    print("adaptive", (shape, symmetric), counts)
    assert counts["deep"] + counts["shallow"] == 123 and counts["full"] <= counts["deep_at_2"] <= counts["deep"] and min(counts["empty_cells"][:13]) >= 1
