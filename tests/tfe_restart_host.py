"""The host's side of the n-tuple network's restarted roll-outs (csrc/tfe_ntuple_restart.hip), for the tests:
which boards of a `start` a game may begin on, those boards as the oracle's environment holds them, and the three host roll-outs
(tests/tfe_host.py, tests/tfe_search_rollout_host.py, tests/tfe_backed_host.py) begun on them through `boards0` -- the unusable entries
replaced by the reset boards -- with the `start` the device is to leave behind.  A helper, not a test."""
import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host
from tests.tfe_backed_host import backed_rollout_on_host
from tests.tfe_search_rollout_host import search_rollout_on_host


def usable_on_host(start) -> np.ndarray:
    """bool[B]: the packed board is not 0, at least one of its four moves changes it (moves_on_host) and it holds no nibble 15"""
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    nib = np.stack([(start >> np.uint64(4 * c)) & np.uint64(15) for c in range(16)], axis=1)
    after, _ = nt.moves_on_host(start)
    return (start != 0) & (after != start[:, None]).any(axis=1) & ~(nib == 15).any(axis=1)


def boards_of_keys(keys) -> np.ndarray:
    """int32[B, 4, 4]: the tiles of packed boards (nibble k > 0 is the tile 2^k)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    nib = np.stack([(keys >> np.uint64(4 * c)) & np.uint64(15) for c in range(16)], axis=1).astype(np.int64)
    return np.where(nib > 0, 1 << nib, 0).astype(np.int32).reshape(-1, 4, 4)


def rollout_from_on_host(start, n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                         layers=0, backed=False):
    """pulse_tfe_nt_rollout_from on the host: (the games, the `start` the launch leaves behind).  layers = 0: rollout_nt_on_host; 1:
    search_rollout_on_host, or with `backed` backed_rollout_on_host -- each from boards0 = the usable boards of `start` and the reset
    boards of the other games."""
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    assert len(start) == n_games and layers in (0, 1) and not (backed and not layers)
    ok = usable_on_host(start)
    boards0, score = np.zeros((n_games, 4, 4), dtype=np.int32), np.zeros(n_games, dtype=np.int64)
    orc.tfe_reset(boards0, score, 4, env_seed, board_id0)
    boards0[ok] = boards_of_keys(start[ok])
    args = (n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round)
    if not layers:
        games = tfe_host.rollout_nt_on_host(*args, boards0=boards0)
    elif backed:
        games = backed_rollout_on_host(*args, layers=1, boards0=boards0)
    else:
        games = search_rollout_on_host(*args, layers=1, boards0=boards0)
    return games, np.where(ok, start, np.uint64(0))
