"""The host's side of the 2048 n-tuple network's games (csrc/tfe_ntuple*.hip), for the tests, in the shape the
device has: ONE policy and ONE roll-out on tests/tfe_host.py's game loop and the oracle's environment, with the options of the device's
one game kernel -- the depth of the search the greedy action comes from (none, one or two chance layers, or the depth the board's
empty cells choose), whether a move records the network's V of the chosen afterstate, whether it keeps the value the search backed
up, and the boards the games start from.  The look-up of a move comes from exactly one of the package's mirrors (greedy_nt_on_host,
search_nt_on_host, search_adaptive_nt_on_host).  Staged networks travel on `tuples` (with_stages) and need nothing here.  Also which
boards of a `start` a game may begin on, and those boards as the oracle's environment holds them.  A helper, not a test."""
import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests import tfe_host


def nibbles(keys) -> np.ndarray:
    """uint64[..., 16]: the 16 nibbles of packed boards, on a new last axis"""
    return (np.asarray(keys, dtype=np.uint64)[..., None] >> (np.uint64(4) * np.arange(16, dtype=np.uint64))) & np.uint64(15)


def usable_on_host(start) -> np.ndarray:
    """bool[B]: the packed board is not 0, at least one of its four moves changes it (moves_on_host) and it holds no nibble 15"""
    start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
    after, _ = nt.moves_on_host(start)
    return (start != 0) & (after != start[:, None]).any(axis=1) & ~(nibbles(start) == 15).any(axis=1)


def boards_of_keys(keys) -> np.ndarray:
    """int32[B, 4, 4]: the tiles of packed boards (nibble k > 0 is the tile 2^k)"""
    nib = nibbles(np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)).astype(np.int64)
    return np.where(nib > 0, 1 << nib, 0).astype(np.int32).reshape(-1, 4, 4)


class _NTuple(tfe_host._Policy):
    """tfe_nt_play_kernel's policy over all live games at once, draws from the package's vectorised Philox; bit 7 is game over.
    depth: 0 is the one-ply rule (greedy_nt_on_host), 1 or 2 the search that many chance layers deep (search_nt_on_host); with
    deep_empty_max a live board with at most that many empty cells is searched two layers deep, every other one layer deep
    (search_adaptive_nt_on_host), and `deep` / `shallow` count the moves at each depth, the epsilon branch's too.  record: a move
    hands the game loop a value -- one ply deep the look-up's own, under a search the NETWORK's V of the chosen afterstate
    (value_on_host), not the search's q.  backed: None, or float64[max_steps, B] of zeros that takes the look-up's `backed` of the
    board each move was made on, whatever the action taken: zero at and beyond a game's length.  One look-up per move serves the
    action, the record and the backed value (at two layers the host's search is the cost of a test)."""
    philox_many, depth, deep_empty_max, record, backed = staticmethod(nt.philox_many_on_host), 0, None, True, None

    @property
    def counters(self):
        return ("greedy",) if self.deep_empty_max is None else ("greedy", "deep", "shallow")

    def choose(self, t, ids, live, boards):
        net, coins = (self.weights, self.tuples, self.symmetric), (self.tie_seed, self.round)
        if self.deep_empty_max is not None:
            look = nt.search_adaptive_nt_on_host(tfe_host.pack_boards(boards), *net, self.gamma, *coins, self.deep_empty_max)
            self.counts["deep"] += int(look["deep"].sum())
            self.counts["shallow"] += int((~look["deep"]).sum())
        elif self.depth:
            look = nt.search_nt_on_host(tfe_host.pack_boards(boards), *net, self.gamma, *coins, layers=self.depth)
        else:
            look = nt.greedy_nt_on_host(tfe_host.pack_boards(boards), *net, self.gamma, *coins)
        assert (look["action"] >= 0).all()                                 # a board that is not over has a candidate
        greedy, uniform = self.branch(t, ids)
        a, rows = np.where(greedy, look["action"], uniform), np.arange(live.size)
        keys = look["after"][rows, a]
        if self.backed is not None:
            self.backed[t, live] = look["backed"]
        values = None if not self.record else look["values"][rows, a] if "values" in look else nt.value_on_host(keys, *net)
        return keys, a, a, look["rewards"][rows, a], values

    def flag(self, live, keys, actions, over):
        return over


def nt_games_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round, *,
                     depth=0, deep_empty_max=None, record=True, backed=False, start=None, boards0=None, keep_boards=None) -> dict:
    """The games of one launch of tfe_nt_play_kernel on the host: 4 x 4, a game stops where it is over or holds a 32,768 tile.  Returns
    tfe_host._play's dict: `greedy` counts the moves not decided by the epsilon branch; `values` float64[max_steps, B] is there with
    `record`, `deep` and `shallow` with `deep_empty_max`, `backed` float64[max_steps, B] with `backed`.  start: uint64[B] packed
    boards; the games begin on its usable boards and on the reset boards of the other games, and `start_left`, the `start` the launch
    leaves behind, is among the results.  boards0: int32[B, 4, 4] to begin on as they are.  The options are those the device offers."""
    deep_empty_max = nt.check_deep_empty_max(deep_empty_max)
    adaptive = deep_empty_max is not None
    assert depth in (0, 1, 2) and not (adaptive and depth) and not (backed and not depth and not adaptive)
    assert start is None or (boards0 is None and (adaptive or depth in (0, 1)))
    extra = {}
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.uint64).reshape(-1)
        assert len(start) == n_games
        ok = usable_on_host(start)
        boards0 = np.zeros((n_games, 4, 4), dtype=np.int32)
        orc.tfe_reset(boards0, np.zeros(n_games, dtype=np.int64), 4, env_seed, board_id0)
        boards0[ok] = boards_of_keys(start[ok])
        extra["start_left"] = np.where(ok, start, np.uint64(0))
    if backed:
        extra["backed"] = np.zeros((int(max_steps), int(n_games)), dtype=np.float64)
    policy = _NTuple(n_games, epsilon, agent_seed, tie_seed, round, weights=weights, tuples=tuples, symmetric=symmetric, gamma=gamma, depth=depth,
                     deep_empty_max=deep_empty_max, record=record, backed=extra.get("backed"))
    return dict(tfe_host._play(policy, n_games, 4, max_steps, env_seed, board_id0, boards0=boards0, keep_boards=keep_boards, tile_cap=32768), **extra)
