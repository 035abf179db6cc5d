"""What the test files of the 2048 n-tuple network's search at the depth the board chooses share (tests/test_tfe_nt_adaptive_*.py,
tests/test_tfe_nt_adaptive_rollout_*.py; DESIGN.md sections 13.11 and 13.13): the shape and its cases, the start boards of the games
from `start`, and the host's games of every case (tests/tfe_nt_host.py), played once per session and handed out read-only.  A helper,
not a test."""
import functools

from tests.tfe_host import pack_boards
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import CRAFTED, TUPLES, seeds, weights
from tests.tfe_search_host import key_of

# The shape of tests/test_tfe_nt_adaptive_*.py: 7 games (one workgroup each, so no batch leaves one partly filled) of at most 256 moves
# on tfe_nt_support's TUPLES, gamma 1, E = 3, round 0.  Rehearsed on the host for exactly these values (about 2 s per case):
#   weights  epsilon  symmetric   games ended (lengths)       cut at 256   moves two layers / one layer deep
#   seeded   0        True        2 (213, 244)                5            1,043 / 694
#   seeded   .25      True        4 (101, 132, 178, 209)      3            762 / 626
#   seeded   .25      False       4 (143, 155, 157, 244)      3            593 / 874
#   zero     .25      True        none                        7            330 / 1,462
# and no game is capped.
GAMES, MAX_STEPS, SEED, ROUND, DEEP_EMPTY_MAX, EPSILON = 7, 256, 7, 0, 3, .25
CASES = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("seeded", EPSILON, False), ("zero", EPSILON, True))

# The shape of the recording games is the same: 7 games (one workgroup each) of at most 256 moves on tfe_nt_support's TUPLES, gamma 1, seed 7,
# E = 3, round 0, and its four CASES.  Recording does not change the games a policy plays, so the header above lists what the cases
# contain: seeded, 2, 4 and 4 of 7 games end at distinct moves and 5, 3 and 3 are cut, 593 to 1,043 moves are deep and 626 to 874 shallow;
# zero weights, all 7 are cut, 330 moves are deep and 1,462 shallow; no game is capped.
#
# The games from `start` (start_boards below): per game the board before move FROM_MOVE = 100 of the ("seeded", .25, True) case's games,
# with entry 0 set to 0, entry 2 to a dead full board and entry 5 to a board holding nibble 15 -- the three ways a start is unusable -- so
# games 0, 2 and 5 begin at their resets and games 1, 3, 4 and 6 on the late boards (3, 5, 2 and 1 empty cells; largest tile 128, 128,
# 64 and 128).  Rehearsed on the host for exactly these values (seeded weights, epsilon .25, symmetric, about 2 s):
#   lengths of games 0..6                 games ended   cut at 256   moves two layers / one layer deep   capped
#   132, 134, 256, 61, 177, 209, 19       6             1 (game 2)   695 / 293                           none
# Games 0, 2 and 5 are the case's own games 0, 2 and 5 (lengths 132, 256, 209): they begin at their resets and share no draw with the others.
FROM_MOVE, FROM_CASE = 100, ("seeded", EPSILON, True)
FROM_REHEARSED = dict(lengths=[132, 134, 256, 61, 177, 209, 19], ended=6, truncated=1, capped=0, deep=695, shallow=293)
UNUSABLE = {0: "zero", 2: "dead", 5: "tile_32768"}                         # game: which unusable start it gets


def _games(name, epsilon, symmetric, **options):
    return nt_games_on_host(GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, *seeds(SEED, round=ROUND), deep_empty_max=DEEP_EMPTY_MAX, **options)


@functools.lru_cache(maxsize=None)
def host_games(name, epsilon, symmetric=True):
    """the host's games of one of CASES, boards before every move kept; played once per session and shared, not to be written to"""
    return _games(name, epsilon, symmetric, record=False, keep_boards="before")


@functools.lru_cache(maxsize=None)
def host_rollout(name, epsilon, symmetric=True):
    """the host's recorded games of one of CASES, with `backed`; played once per session and shared, not to be written to"""
    return _games(name, epsilon, symmetric, backed=True)


@functools.lru_cache(maxsize=None)
def start_boards():
    """uint64[GAMES], read-only: the `start` of the From tests (the header says what it holds)"""
    start = pack_boards(host_games(*FROM_CASE)["boards"][FROM_MOVE]).astype("uint64")
    for g, which in UNUSABLE.items():
        start[g] = 0 if which == "zero" else key_of(CRAFTED[which])
    start.setflags(write=False)
    return start


@functools.lru_cache(maxsize=None)
def host_rollout_from():
    """the host's recorded games from start_boards() under FROM_CASE, with `backed` and `start_left`, the `start` left behind; shared,
    read-only"""
    return _games(*FROM_CASE, backed=True, start=start_boards())
