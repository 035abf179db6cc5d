"""The host's side of the n-tuple network's training roll-out at the adaptive search depth (csrc/tfe_ntuple_search_rollout.hip;
DESIGN.md section 13.13), for the tests: tests/tfe_adaptive_host.py's policy -- the live boards of a move searched at the depth their
empty cells choose -- which also hands the game loop the value a move records, the NETWORK's V of the chosen afterstate, and keeps per
move the value the search backed up at that depth.  One search per move (search_adaptive_nt_on_host gives the q, the action and
search_backed_on_host of the q at once); tests/test_tfe_nt_adaptive_rollout_cpu.py holds its games to _NTupleAdaptive's.  A helper, not
a test."""
import functools

import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host
from tests.tfe_adaptive_host import CASES, DEEP_EMPTY_MAX, EPSILON, GAMES, MAX_STEPS, ROUND, SEED, _NTupleAdaptive  # noqa: F401 (the shape, re-exported)
from tests.tfe_restart_host import boards_of_keys, usable_on_host

# The shape is tests/tfe_adaptive_host.py's: 7 games (one workgroup each) of at most 256 moves on tfe_nt_support's TUPLES, gamma 1, seed 7,
# E = 3, round 0, and its four CASES.  Recording does not change the games a policy plays, so that file's header lists what the cases
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


class _NTupleAdaptiveRecord(_NTupleAdaptive):
    """pulse_tfe_nt_rollout_adaptive at `deep_empty_max`: _NTupleAdaptive's choice -- the same boards at the same depths, the same
    counters -- from search_adaptive_nt_on_host, with value_on_host of the chosen afterstates as the recorded values and `backed`
    float64[max_steps, B], search_backed_on_host of the q at the depth the board chose, filled as the games go: zero at and beyond a
    game's length"""
    def __init__(self, n_games, *args, max_steps, **rest):
        super().__init__(n_games, *args, **rest)
        self.backed = np.zeros((int(max_steps), int(n_games)), dtype=np.float64)

    def choose(self, t, ids, live, boards):
        look = nt.search_adaptive_nt_on_host(tfe_host.pack_boards(boards), self.weights, self.tuples, self.symmetric, self.gamma, self.tie_seed,
                                             self.round, self.deep_empty_max)
        assert (look["action"] >= 0).all()                                 # a board that is not over has a candidate
        self.counts["deep"] += int(look["deep"].sum())
        self.counts["shallow"] += int((~look["deep"]).sum())
        greedy, uniform = self.branch(t, ids)
        a, rows = np.where(greedy, look["action"], uniform), np.arange(live.size)
        keys = look["after"][rows, a]
        self.backed[t, live] = look["backed"]
        return keys, a, a, look["rewards"][rows, a], nt.value_on_host(keys, self.weights, self.tuples, self.symmetric)


def adaptive_rollout_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                             deep_empty_max, backed=False, boards0=None):
    """pulse_tfe_nt_rollout_adaptive on the host: search_rollout_on_host's records of adaptive_games_on_host's games; the dict has
    `values`, `deep` and `shallow`, and with `backed` also `backed` float64[max_steps, B]."""
    policy = _NTupleAdaptiveRecord(n_games, epsilon, agent_seed, tie_seed, round, max_steps=max_steps, weights=weights, tuples=tuples,
                                   symmetric=symmetric, gamma=gamma, deep_empty_max=nt.check_deep_empty_max(deep_empty_max))
    out = tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, boards0=boards0, tile_cap=32768)
    return dict(out, backed=policy.backed) if backed else out


def adaptive_rollout_from_on_host(start, n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0,
                                  round, deep_empty_max, backed=False):
    """pulse_tfe_nt_rollout_adaptive with `start` on the host: (the games, the `start` the launch leaves behind), as
    tfe_restart_host.rollout_from_on_host gives them: boards0 = the usable boards of `start` and the reset boards of the other games."""
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    assert len(start) == n_games
    ok = usable_on_host(start)
    boards0, score = np.zeros((n_games, 4, 4), dtype=np.int32), np.zeros(n_games, dtype=np.int64)
    orc.tfe_reset(boards0, score, 4, env_seed, board_id0)
    boards0[ok] = boards_of_keys(start[ok])
    games = adaptive_rollout_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                                     deep_empty_max, backed=backed, boards0=boards0)
    return games, np.where(ok, start, np.uint64(0))


def _seeds():
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_support import BOARD_ID0
    return SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0, ROUND


@functools.lru_cache(maxsize=None)
def host_rollout(name, epsilon, symmetric=True):
    """the host's recorded games of one of CASES, with `backed`; played once per session and shared, not to be written to"""
    from tests.tfe_nt_support import TUPLES, weights
    return adaptive_rollout_on_host(GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, *_seeds(), DEEP_EMPTY_MAX, backed=True)


@functools.lru_cache(maxsize=None)
def start_boards():
    """uint64[GAMES], read-only: the `start` of the From tests (the header says what it holds)"""
    from tests.tfe_adaptive_host import host_games
    from tests.tfe_nt_support import CRAFTED
    from tests.tfe_search_host import key_of
    start = tfe_host.pack_boards(host_games(*FROM_CASE)["boards"][FROM_MOVE]).astype(np.uint64)
    for g, which in UNUSABLE.items():
        start[g] = 0 if which == "zero" else key_of(CRAFTED[which])
    start.setflags(write=False)
    return start


@functools.lru_cache(maxsize=None)
def host_rollout_from():
    """(the host's recorded games from start_boards() under FROM_CASE, with `backed`; the `start` left behind); shared, read-only"""
    from tests.tfe_nt_support import TUPLES, weights
    name, epsilon, symmetric = FROM_CASE
    return adaptive_rollout_from_on_host(start_boards(), GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, *_seeds(), DEEP_EMPTY_MAX,
                                         backed=True)
