"""The host's side of the n-tuple network's play under the search whose depth the board chooses (csrc/tfe_ntuple_search.hip;
DESIGN.md section 13.11), for the tests: tests/tfe_host.py's game loop on the oracle's environment, the live boards of a move split by
their empty cells and searched by search_nt_on_host once per depth.  A helper, not a test."""
import functools

import numpy as np

from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host
from tests.tfe_search_host import _NTupleSearch

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


class _NTupleAdaptive(_NTupleSearch):
    """pulse_tfe_nt_evaluate_search_adaptive at `deep_empty_max`: a live board with at most that many empty cells is searched two
    layers deep, every other one layer deep; `deep` / `shallow` count the moves at each depth, the epsilon branch's too"""
    counters = ("greedy", "deep", "shallow")

    def choose(self, t, ids, live, boards):
        keys = tfe_host.pack_boards(boards)
        deep = nt.count_empty_on_host(keys) <= self.deep_empty_max
        action, rewards = np.zeros(live.size, dtype=np.int64), np.zeros((live.size, 4), dtype=np.int64)
        after = np.zeros((live.size, 4), dtype=np.uint64)
        for rows, layers in ((~deep, 1), (deep, 2)):
            if rows.any():
                look = nt.search_nt_on_host(keys[rows], self.weights, self.tuples, self.symmetric, self.gamma, self.tie_seed, self.round, layers=layers)
                action[rows], after[rows], rewards[rows] = look["action"], look["after"], look["rewards"]
        assert (action >= 0).all()                                         # a board that is not over has a candidate
        self.counts["deep"] += int(deep.sum())
        self.counts["shallow"] += int((~deep).sum())
        greedy, uniform = self.branch(t, ids)
        a, rows = np.where(greedy, action, uniform), np.arange(live.size)
        return after[rows, a], a, a, rewards[rows, a], None


def adaptive_games_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                           deep_empty_max, keep_boards=None):
    """pulse_tfe_nt_evaluate_search_adaptive on the host: tests/tfe_search_host.py's games with q at the depth the board chooses; the
    dict also has `deep` and `shallow`, the moves at each depth."""
    policy = _NTupleAdaptive(n_games, epsilon, agent_seed, tie_seed, round, weights=weights, tuples=tuples, symmetric=symmetric, gamma=gamma,
                             deep_empty_max=nt.check_deep_empty_max(deep_empty_max))
    return tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, keep_boards=keep_boards, tile_cap=32768)


@functools.lru_cache(maxsize=None)
def host_games(name, epsilon, symmetric=True):
    """the host's games of one of CASES, boards before every move kept; played once per session and shared, not to be written to"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_support import BOARD_ID0, TUPLES, weights
    return adaptive_games_on_host(GAMES, MAX_STEPS, epsilon, 1.0, weights(name), TUPLES, symmetric, SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0,
                                  ROUND, DEEP_EMPTY_MAX, keep_boards="before")
