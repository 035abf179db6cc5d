"""The host's side of the n-tuple network's training roll-out under expectimax search (csrc/tfe_ntuple_search_rollout.hip; DESIGN.md
section 13.5), for the tests: tests/tfe_search_host.py's policy, which also hands the game loop the value a move records -- the
NETWORK's V of the chosen afterstate (value_on_host), not the search's q.  A helper, not a test."""
from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host
from tests.tfe_search_host import _NTupleSearch


class _NTupleSearchRecord(_NTupleSearch):
    """pulse_tfe_nt_rollout_search at `layers`: _NTupleSearch's choice, and value_on_host of the chosen afterstates as the recorded values"""
    def choose(self, t, ids, live, boards):
        keys, recorded, moved, rewards, _ = super().choose(t, ids, live, boards)
        return keys, recorded, moved, rewards, nt.value_on_host(keys, self.weights, self.tuples, self.symmetric)


def search_rollout_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round, layers=1,
                           boards0=None):
    """pulse_tfe_nt_rollout_search on the host: tfe_host.rollout_nt_on_host's games, draws and records with the greedy action from
    search_nt_on_host at `layers` chance layers; `values` float64[max_steps, B] among the records."""
    policy = _NTupleSearchRecord(n_games, epsilon, agent_seed, tie_seed, round, weights=weights, tuples=tuples, symmetric=symmetric, gamma=gamma,
                                 layers=layers)
    return tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, boards0=boards0, tile_cap=32768)
