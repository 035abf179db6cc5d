"""The host's side of the n-tuple network's expectimax play (csrc/tfe_ntuple_search.hip), for the tests: tests/tfe_host.py's game loop on
the oracle's environment under search_nt_on_host, and packed boards from lists of nibbles.  A helper, not a test."""
import numpy as np

from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host


def key_of(nibbles) -> int:
    """the packed board of 16 nibbles (log2 tiles, 0 = empty), row-major"""
    assert len(nibbles) == 16 and all(0 <= int(x) <= 15 for x in nibbles)
    return sum(int(x) << (4 * i) for i, x in enumerate(nibbles))


class _NTupleSearch(tfe_host._Policy):
    """pulse_tfe_nt_evaluate_search: search_nt_on_host over all live games at once; bit 7 is game over"""
    philox_many, counters = staticmethod(nt.philox_many_on_host), ("greedy",)

    def choose(self, t, ids, live, boards):
        look = nt.search_nt_on_host(tfe_host.pack_boards(boards), self.weights, self.tuples, self.symmetric, self.gamma, self.tie_seed, self.round)
        assert (look["action"] >= 0).all()                                 # a board that is not over has a candidate
        greedy, uniform = self.branch(t, ids)
        a, rows = np.where(greedy, look["action"], uniform), np.arange(live.size)
        return look["after"][rows, a], a, a, look["rewards"][rows, a], None

    def flag(self, live, keys, actions, over):
        return over


def search_games_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                         keep_boards=None):
    """pulse_tfe_nt_evaluate_search on the host: tfe_host.rollout_nt_on_host's games with q from the search."""
    policy = _NTupleSearch(n_games, epsilon, agent_seed, tie_seed, round, weights=weights, tuples=tuples, symmetric=symmetric, gamma=gamma)
    return tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, keep_boards=keep_boards, tile_cap=32768)
