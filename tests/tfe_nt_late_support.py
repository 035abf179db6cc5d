"""What the late-game tests of the 2048 n-tuple network's three newest units share (tests/test_tfe_nt_late_cpu.py,
tests/test_tfe_nt_late_gpu.py): weight sets by tile stage at the ABI's four stages and at thresholds on the
nibbles 1, 14 and 15, games continued across rounds at the pick's three-way branch, and the search whose depth the empty cells choose
at the limit shapes -- all of them on late_start's boards.  Here are the stage tiles, the regimes, the host's games of every case with
the PREMISES a case rests on asserted where the games are made (so a changed seed or a changed late_start cannot empty a test
unnoticed), and the seeds chosen on the host where a floor was missed at the regime's own.  Everything is played once per session and
handed out read-only.  A helper, not a test."""
import functools
from types import SimpleNamespace

import numpy as np

from tests.tfe_continue_host import Carried, round_on_host
from tests.tfe_nt_host import nibbles, nt_games_on_host
from tests.tfe_nt_staged_support import staged, staged_weights
from tests.tfe_nt_support import BOARD_ID0, CRAFTED, MORE, SEED, SHAPES, late_start, nt, seeds, weights
from tests.tfe_search_host import key_of

# Four stages, the ABI's limit.  Stage 0: boards below the 8 tile (late_start's games with g % 4 == 3 begin at reset); stage 1: nibbles
# 3 to 13; stage 2: boards whose largest tile is 16,384; stage 3: boards with the 32,768 tile, where the game is also capped.
LATE_TILES = (8, 16384, 32768)
# A threshold at nibble 1: every board with a tile is in stage 1 or above, so stage 0 holds no afterstate at all.
LOW_TILES = (2, 256, 16384)
S = 4
GAMES, MAX_STEPS, EPSILON, ROUND = 65, 96, .25, 0                          # section 13.8's late regime at the learners' seed (SEED = 457), gamma 1
MODES = {"one_ply": (0, False), "search": (1, False), "backed": (1, True)}  # (layers, backed)
DIVISOR = {0: 64, 1: 1}                                                     # layers: what divides the seeded weights (tests/test_tfe_nt_staged_gpu.py)
ROLLOUT_CASES = [("eight", symmetric, mode) for symmetric in (True, False) for mode in MODES] + [("one6", False, "one_ply")]
# "eight" with 8 images under the search cuts 7 games at move 96 without the cap at seed 457, one short of the floor; of the seeds
# 458.. the first that holds every floor of the case was taken, on the host alone (tests/test_tfe_nt_late_cpu.py prints the counts).
LATE_SEED = {("eight", True, 1): 459}
FLOOR = dict(per_stage=20, capped=8, dead=8, cut=8)

CONTINUE_GAMES, CONTINUE_ROUNDS = 257, 5
# max_steps: (games, layers, seed).  At max_steps = 2 a game makes one kept move per round, so few finished games had been continued:
# 8 to 17 at the seeds 457 to 463; 561 is the first seed from 457 on with 20, found on the host alone.
CONTINUE_CASES = {"K2": (257, 2, 0, 561), "K7": (257, 7, 0, SEED), "K16": (257, 16, 0, SEED), "K16_backed": (65, 16, 1, SEED)}
CONTINUE_FLOOR = dict(capped=50, capped_at_k=3, dead_at_k=5, resumed=20, continued=100)

DEPTHS = (0, 2, 4, 16)                                                     # the adaptive search's E
ADAPTIVE_FLOOR = dict(deep=25, shallow=25, q_differs=20, action_differs=3)
SEARCH_ROUND = 3                                                           # the coins of another round than the games'


def late_weights(shape, layers):
    """float32[4 W] of the shape, read-only: a slice of its own per stage, / 64 one ply deep so that play is led by the rewards"""
    return staged_weights(SHAPES[shape], S, DIVISOR[layers])


def late_seed(shape, symmetric, layers):
    return LATE_SEED.get((shape, symmetric, layers), SEED)


# ------------------------------------------------------------------ 1. the games from late_start(65, 3) on four stages
@functools.lru_cache(maxsize=None)
def late_games(shape, symmetric, layers, tiles=LATE_TILES):
    """The host's games of the late regime under `tiles` (at one layer with the backed values: recording them does not change play),
    with what the regime rests on asserted.  Under LATE_TILES: every stage holds at least 20 recorded afterstates; at least 8 games are
    capped, 8 end on a dead board and 8 are cut at move 96 without a 32,768 tile; every recorded afterstate of stage 3 is a capped
    game's last move, and at least 8 of their bytes have no terminal bit.  Under LOW_TILES: stage 0 holds nothing, every other stage
    at least 20.  Returns a namespace: want (the games), left (the `start` the launch is to leave), L, played, stage [T, B], per_stage,
    capped / dead / cut bool[B], seed."""
    seed = late_seed(shape, symmetric, layers)
    start = late_start(GAMES, 3)
    want = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, 1.0, late_weights(shape, layers), staged(SHAPES[shape], tiles), symmetric, *seeds(seed, BOARD_ID0, ROUND),
                            depth=layers, backed=bool(layers), start=start)
    left = want["start_left"]
    L, rows = want["lengths"].astype(np.int64), np.arange(GAMES)
    played = np.arange(MAX_STEPS)[:, None] < L[None, :]
    stage = nt().stage_of_keys_on_host(want["keys"].reshape(-1), tiles).reshape(MAX_STEPS, GAMES)
    per_stage = np.bincount(stage[played], minlength=S)
    fifteen = (nibbles(want["keys"]) == 15).any(axis=2) & played
    capped, dead = fifteen[L - 1, rows], want["steps"][L - 1, rows] >> 7 != 0     # a game stops at its first 32,768 tile: only its last afterstate holds one
    cut = (L == MAX_STEPS) & ~capped & ~dead
    g = SimpleNamespace(want=want, left=left, L=L, played=played, stage=stage, per_stage=per_stage.tolist(), capped=capped, dead=dead, cut=cut, seed=seed,
                        counts=dict(per_stage=per_stage.tolist(), capped=int(capped.sum()), dead=int(dead.sum()), cut=int(cut.sum()), moves=int(L.sum())))
    where = (shape, symmetric, layers, tiles, g.counts)
    assert int(capped.sum()) == want["capped"] == int(fifteen.sum()) and int(dead.sum()) == want["ended"] and want["ended"] + want["truncated"] == GAMES, where
    assert g.counts["capped"] >= FLOOR["capped"] and g.counts["dead"] >= FLOOR["dead"] and g.counts["cut"] >= FLOOR["cut"], where
    assert np.array_equal(left, start) and int(np.count_nonzero(left)) == GAMES - len(start[3::4]), where
    if tiles == LATE_TILES:
        assert min(g.per_stage) >= FLOOR["per_stage"], where
        top = played & (stage == 3)
        assert np.array_equal(top, fifteen) and int((capped & ~dead).sum()) >= FLOOR["capped"], where    # the capping move, without a terminal bit
    else:
        assert g.per_stage[0] == 0 and min(g.per_stage[1:]) >= FLOOR["per_stage"], where
    return g


def with_dead_caps(steps, g):
    """The step bytes with the terminal bit set in the last byte of every second capped game.  A capped game's last move is CUT: the
    learners skip it, so no roll-out's own records add to stage 3's slice (a spawn that leaves a board with the 32,768 tile dead would:
    no game of the regime has one).  A learner reads the records as data: with the bit set the move is learnt, with target 0, in the top
    slice, as the records of such a game would be.  The other capped games keep their cut."""
    out = np.array(steps)
    marked = np.flatnonzero(g.capped & ~g.dead)[::2]
    out[g.L[marked] - 1, marked] |= 0x80
    return out, marked


# ------------------------------------------------------------------ the search boards
@functools.lru_cache(maxsize=None)
def late_boards():
    """uint64[9 + 49 + 65], read-only: the crafted boards, the boards of late_start(65, 3) that are not 0, and the afterstate 12 moves
    into each of the 65 games of "eight", 8 images, one ply (the last afterstate of a game that is shorter)"""
    g = late_games("eight", True, 0)
    late = late_start(GAMES, 3)
    crafted = np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64)
    keys = np.concatenate([crafted, late[late != 0], g.want["keys"][np.minimum(12, g.L - 1), np.arange(GAMES)]])
    assert keys.shape == (123,)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def staged_search(shape, symmetric, tiles):
    """search_nt_on_host of late_boards() on the shape's four slices, with its premise.  Under LATE_TILES: the boards' own stages and
    their afterstates' cover all four, and at least 8 boards have two candidate afterstates in different stages -- the case values4
    forms four bases for (24 have: late_start's boards with two adjacent 14s, whose merge is in stage 3).  Under LOW_TILES no board with
    a tile is in stage 0, so the stages are 1 to 3, and that merge crosses no threshold: a pair needs two 13s or two 7s to merge, which
    late_start leaves to chance -- 6 boards have one, and the floor is 4.  Returns (the mirror's rows, the boards with such a pair)."""
    n, keys = nt(), late_boards()
    want = n.search_nt_on_host(keys, late_weights(shape, 1), staged(SHAPES[shape], tiles), symmetric, 1.0, seeds(SEED)[2], SEARCH_ROUND)
    cand = want["after"] != keys[:, None]
    stage = n.stage_of_keys_on_host(want["after"].reshape(-1), tiles).reshape(-1, 4)
    own = n.stage_of_keys_on_host(keys, tiles)
    lo, hi = np.where(cand, stage, S).min(axis=1), np.where(cand, stage, -1).max(axis=1)
    split = int((cand.any(axis=1) & (lo != hi)).sum())
    reached = set(own.tolist()) | set(stage[cand].tolist())
    assert (reached, split >= 8) == ({0, 1, 2, 3}, True) if tiles == LATE_TILES else (reached, split >= 4) == ({1, 2, 3}, True), (shape, symmetric, tiles, reached, split)
    return want, split


@functools.lru_cache(maxsize=None)
def adaptive_search(shape, symmetric, E):
    """search_adaptive_nt_on_host of late_boards() on the shape's seeded weights (one stage)"""
    return nt().search_adaptive_nt_on_host(late_boards(), weights("seeded", SHAPES[shape]), SHAPES[shape], symmetric, 1.0, seeds(SEED)[2], SEARCH_ROUND, E)


@functools.lru_cache(maxsize=None)
def adaptive_premises(shape, symmetric):
    """At E = 4: at least 25 boards are deep and 25 shallow, the shallow rows are bit for bit the one-layer search's, and at least 20
    deep rows differ from it in q, 3 in the action.  Returns the counts."""
    n, keys, tuples = nt(), late_boards(), SHAPES[shape]
    want = adaptive_search(shape, symmetric, 4)
    one = n.search_nt_on_host(keys, weights("seeded", tuples), tuples, symmetric, 1.0, seeds(SEED)[2], SEARCH_ROUND)
    deep = want["deep"]
    assert np.array_equal(deep, n.count_empty_on_host(keys) <= 4)
    assert np.array_equal(want["q"][~deep].view(np.uint64), one["q"][~deep].view(np.uint64)) and np.array_equal(want["action"][~deep], one["action"][~deep])
    counts = dict(deep=int(deep.sum()), shallow=int((~deep).sum()), q_differs=int((want["q"][deep] != one["q"][deep]).any(axis=1).sum()),
                  action_differs=int((want["action"][deep] != one["action"][deep]).sum()), deep_at_2=int(adaptive_search(shape, symmetric, 2)["deep"].sum()),
                  full=int(adaptive_search(shape, symmetric, 0)["deep"].sum()), empty_cells=np.bincount(n.count_empty_on_host(keys), minlength=17).tolist())
    assert all(counts[k] >= v for k, v in ADAPTIVE_FLOOR.items()) and counts["full"] >= 3 and int((nibbles(keys) == 15).any(axis=1).sum()) >= 2, (shape, symmetric, counts)
    return counts


# ------------------------------------------------------------------ 2. five continued rounds from late_start, under fixed weights
@functools.lru_cache(maxsize=None)
def continued_rounds(case):
    """Five rounds of continued games on the host (tests/tfe_continue_host.py: round_on_host) from a `start` of late_start(games, 3), on
    "eight" with 8 images and LATE_TILES, weights fixed, round r on the boards BOARD_ID0 + games * r.  Returns (per round a namespace of
    start -- the `start` the round played from --, games, words, cut, carried -- start, score, moves and finished after its pick --, and
    the counts over the rounds), the premises of the case asserted."""
    games, K, layers, seed = CONTINUE_CASES[case]
    tuples, w = staged(SHAPES["eight"], LATE_TILES), late_weights("eight", layers)
    c, rounds = Carried(games), []
    c.start = np.array(late_start(games, 3))
    counts = dict(capped=0, capped_at_k=0, dead_at_k=0, resumed=0, finished=0, continued=[])
    for r in range(CONTINUE_ROUNDS):
        start = c.start.copy()
        g, words, cut = round_on_host(c, games, K, EPSILON, 1.0, w, tuples, True, *seeds(seed, BOARD_ID0 + games * r, r), depth=layers, backed=bool(layers))
        L, rows = g["lengths"].astype(np.int64), np.arange(games)
        capped, dead = (nibbles(g["keys"][L - 1, rows]) == 15).any(axis=1), g["steps"][L - 1, rows] >> 7 != 0
        assert words[7] == int(capped.sum()) and not (cut & (capped | dead)).any()
        counts["capped_at_k"] += int((capped & (L == K)).sum())
        counts["dead_at_k"] += int((dead & (L == K)).sum())
        counts["continued"].append(words[5])
        rounds.append(SimpleNamespace(start=start, games=g, words=words, cut=cut, capped=capped,
                                      carried=SimpleNamespace(start=c.start.copy(), score=c.score.copy(), moves=c.moves.copy(), finished=list(c.finished))))
    counts.update(capped=c.finished[7], resumed=c.finished[6], finished=c.finished[0])
    if games == CONTINUE_GAMES:
        floor = CONTINUE_FLOOR
        assert counts["capped"] >= floor["capped"] and counts["resumed"] >= floor["resumed"] and min(counts["continued"]) >= floor["continued"], (case, counts)
        assert K != 2 or counts["capped_at_k"] >= floor["capped_at_k"], (case, counts)
        assert K != 7 or counts["dead_at_k"] >= floor["dead_at_k"], (case, counts)
    else:                                                                   # 65 games: the floors of a quarter of the games, as the late regime's
        assert counts["capped"] >= 8 and counts["resumed"] >= 8 and min(counts["continued"]) >= 25, (case, counts)
    return rounds, counts
