"""The host's side of the n-tuple network's search-backed targets (csrc/tfe_ntuple_backed.hip), for the tests:
tests/tfe_search_rollout_host.py's recording policy, which also keeps per move the value the search backed up for the board the move
was made on -- search_nt_on_host's `backed`, the largest q over the candidate moves, whatever the action taken.  A helper, not a test."""
import numpy as np

from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host
from tests.tfe_search_rollout_host import _NTupleSearchRecord


class _NTupleSearchBacked(_NTupleSearchRecord):
    """pulse_tfe_nt_rollout_backed at `layers`: _NTupleSearchRecord's choice and records from ONE search per move (at two layers the
    host's search is the cost of a test), and `backed` float64[max_steps, B] filled as the games go: zero at and beyond a game's length"""
    def __init__(self, n_games, *args, max_steps, **rest):
        super().__init__(n_games, *args, **rest)
        self.backed = np.zeros((int(max_steps), int(n_games)), dtype=np.float64)

    def choose(self, t, ids, live, boards):
        look = nt.search_nt_on_host(tfe_host.pack_boards(boards), self.weights, self.tuples, self.symmetric, self.gamma, self.tie_seed, self.round,
                                    layers=self.layers)
        assert (look["action"] >= 0).all()                                 # a board that is not over has a candidate
        greedy, uniform = self.branch(t, ids)
        a, rows = np.where(greedy, look["action"], uniform), np.arange(live.size)
        keys = look["after"][rows, a]
        self.backed[t, live] = look["backed"]
        return keys, a, a, look["rewards"][rows, a], nt.value_on_host(keys, self.weights, self.tuples, self.symmetric)


def backed_rollout_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round, layers=1,
                           boards0=None):
    """pulse_tfe_nt_rollout_backed on the host: search_rollout_on_host's games and records, with `backed` float64[max_steps, B] among them."""
    policy = _NTupleSearchBacked(n_games, epsilon, agent_seed, tie_seed, round, max_steps=max_steps, weights=weights, tuples=tuples, symmetric=symmetric,
                                 gamma=gamma, layers=layers)
    out = tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, boards0=boards0, tile_cap=32768)
    return dict(out, backed=policy.backed)
