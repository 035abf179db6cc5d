"""2048 on 4 x 4: an n-tuple network trained by batch TD(0) -- or, with `lam`, TD(lambda) -- on afterstates, on the device (DESIGN.md
sections 13 and 13.2; csrc/tfe_ntuple.hip, csrc/tfe_ntuple_lambda.hip).

The value of an afterstate -- the board after the move and before the spawn -- is the sum of a few lookup tables.  Each table is
indexed by the tiles (4-bit log2, the state key's nibbles) on a fixed set of cells, read on the board's eight images under the
symmetries of the square, which share the table.  A round is three launches and nothing read back in between:
`pulse_tfe_nt_rollout` plays `n_games` whole games, one lane each, greedily (or epsilon-greedily) on reward + gamma * V among the
moves that change the board, and records per move the afterstate's key, its V and one byte; `pulse_tfe_nt_learn` runs one lane per
recorded move and adds the temporal difference reward' + gamma * V' - V (0 - V at a terminal move) as a fixed-point integer into
{sum, cnt} of every weight the afterstate reads; `pulse_tfe_nt_apply` moves every visited weight by alpha / F of the MEAN of its
adds and zeroes the accumulators.  `pulse_tfe_nt_evaluate` plays games without a trajectory and reduces the scores in the launch; `pulse_tfe_nt_search` and
`pulse_tfe_nt_evaluate_search` play under expectimax search one chance layer deep (section 13.1), 32 lanes per board; with `layers=2`
`pulse_tfe_nt_search_deep` and `pulse_tfe_nt_evaluate_search_deep` search two (section 13.4), 256 lanes per board; with `layers=2, deep_empty_max=E`
`pulse_tfe_nt_search_adaptive` and `pulse_tfe_nt_evaluate_search_adaptive` search two on the boards with at most E empty cells and one on the others (section 13.11); with the attribute `rollout_layers` = 1 or 2 the
round's games themselves are played under that search, `pulse_tfe_nt_rollout_search` (section 13.5), and recorded alike.  With `lam > 0`
the learn launch is `pulse_tfe_nt_learn_lambda` (section 13.2): one lane per game walks the recorded game backwards and leaves the
lambda-differences D_t = delta_t + gamma * lam * D_{t+1} in `deltas`, and the same one-lane-per-move adds follow with D_t for delta_t.

The policy of a round is frozen (the weights are only read by the roll-out) and the adds are integers, so a round's result does not
depend on scheduling: `feature_cells_on_host`, `value_on_host`, `greedy_nt_on_host`, `search_nt_on_host`, `learn_nt_on_host`,
`lambda_deltas_on_host`, `learn_lambda_nt_on_host` and `apply_nt_on_host` are the host's statement of the same arithmetic in numpy, vectorised over boards, and the device is held to them word for word.

With `tc=True` (section 13.3; csrc/tfe_ntuple_tc.hip) every weight has a step size of its own, rho = |E| / A, from the running sums of
its rounds' mean errors and mean absolute errors: `learn` is `pulse_tfe_nt_learn_tc`, which also adds |d| into a third accumulator,
and `apply` is `pulse_tfe_nt_apply_tc`; `learn_tc_nt_on_host` and `apply_tc_nt_on_host` state them on the host.

With the attribute `backed_targets` (section 13.6; csrc/tfe_ntuple_backed.hip) a round under search also records, per move, the value
the search backed up for the board the move was made on (`pulse_tfe_nt_rollout_backed`), and `learn` is `pulse_tfe_nt_learn_backed`:
the difference of a move is backed[t + 1] - V_t in place of r' + gamma * V' - V.  `search_backed_on_host`, `backed_deltas_on_host`
and `learn_backed_nt_on_host` state them on the host.

With the attribute `restart_fraction` > 0 (section 13.7; csrc/tfe_ntuple_restart.hip) `learn_batch` ends with a fourth launch,
`pulse_tfe_nt_restart_pick`, which writes into `start` the board every long enough game of the round stood on at that fraction of its
length, and the next round's games begin there (`pulse_tfe_nt_rollout_from`) instead of at their reset boards: the "restart" strategy
of the n-tuple 2048 literature.  `spawn_on_host` and `restart_pick_on_host` state the pick on the host.

With `stage_tiles` (section 13.9; csrc/tfe_ntuple_staged.hip) the network is S = len(stage_tiles) + 1 copies of its tables, and a board
reads -- a recorded move adds to -- the copy of its stage, the number of those tiles its largest tile has reached: multi-stage TD.
Every launch of a round then goes through the four `pulse_tfe_nt_*_staged` entry points and one apply launch per stage; `add_stage`
splits a stage in two at a tile, the new one starting as a copy (weight promotion).  On the host the stages travel on `tuples`
(`with_stages`), so every mirror above reads and adds by stage; `stage_of_keys_on_host` states the stage.

With the attribute `continue_games` (section 13.10; csrc/tfe_ntuple_continue.hip) an agent built with a small `max_steps` = K plays K
moves of every game per round: `learn_batch` ends with `pulse_tfe_nt_continue_pick`, which puts into `start` the board the last move
of every cut game was made on -- the next round decides that move again under the new weights, so every transition is learnt once --
keeps the score and moves of the game so far in `carry_score` / `carry_moves` and adds the games that ended, whole, to `finished`.
`continue_pick_on_host` states the pick on the host; `eval_max_steps` gives the evaluations a cap of their own."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from .. import _native
from .tfe_common import (AGENT_KEY, EVAL_BINS, TIE_KEY, _TFEGamesGPU, greedy_scan_many_on_host, philox_many_on_host,  # noqa: F401 (re-exported)
                         rewards_of_scores, transforms_on_host, unpack_steps)
from .tfe_common import eval_summary_on_host as _eval_summary_on_host

MAX_TUPLES, MAX_LEN, FRAC_BITS, DELTA_MAX = _native.TFE_NT_MAX_TUPLES, _native.TFE_NT_MAX_LEN, _native.TFE_NT_FRAC_BITS, _native.TFE_NT_DELTA_MAX
MAX_STAGES = _native.TFE_NT_MAX_STAGES
DEFAULT_TUPLES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))       # two rows and two 2 x 3 rectangles
STATS = ("moves", "learnt", "skipped", "truncated", "clamped")                                # words 0..4 of the stats buffer
EVAL_SUMMARY = ("games", "moves", "score_sum", "score_sq_sum", "max_score", "truncated", "moves_greedy", "tile_capped")
CHECKPOINT_VERSION = 1                                                                        # what an agent with lam == 0 writes
CHECKPOINT_VERSION_LAMBDA = 2                                                                 # ... and with lam != 0: version 1's arrays and `lam`
CHECKPOINT_VERSION_TC = 4                                                                     # ... and with tc: version 2's and tc_index / tc_e / tc_a (3 is not a format)
CHECKPOINT_VERSION_STAGED = 5                                                                 # ... and with stage_tiles: version 2's or 4's arrays over S * W weights and `stage_tiles`
TC_RHO_BITS = 32                                                                              # rho is summed as llrint(rho * 2^32)
CHECKPOINT_SCALARS = ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")
_U64 = np.uint64


# ------------------------------------------------------------------ the network's shape
def check_tuples(tuples) -> tuple:
    """The tuples as a tuple of tuples of ints, after the library's own checks (ValueError)."""
    stage_tiles = stage_tiles_of(tuples)
    tuples = tuple(tuple(int(c) for c in t) for t in tuples)
    if not 1 <= len(tuples) <= MAX_TUPLES:
        raise ValueError(f"n_tuples must be in 1..{MAX_TUPLES}")
    for t in tuples:
        if not 1 <= len(t) <= MAX_LEN:
            raise ValueError(f"a tuple's length must be in 1..{MAX_LEN}")
        if any(not 0 <= c <= 15 for c in t) or len(set(t)) != len(t):
            raise ValueError("a tuple's cells must be distinct and in 0..15")
    return StagedTuples(tuples, stage_tiles) if stage_tiles else tuples


# ------------------------------------------------------------------ weight sets by tile stage
def check_stage_tiles(stage_tiles) -> tuple:
    """The tiles at which the stages 1, 2, ... begin, as a tuple of ints: at most MAX_STAGES - 1 powers of two in 2..32,768, strictly
    increasing (ValueError otherwise; a bool is no tile).  () is the one-stage network."""
    tiles = tuple(stage_tiles)
    if any(isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) for t in tiles):
        raise ValueError("a stage tile must be an int")
    tiles = tuple(int(t) for t in tiles)
    if len(tiles) > MAX_STAGES - 1:
        raise ValueError(f"at most {MAX_STAGES - 1} stage tiles ({MAX_STAGES} stages)")
    if any(not 2 <= t <= 32768 or t & (t - 1) for t in tiles):
        raise ValueError("a stage tile must be a power of two in 2..32768")
    if any(b <= a for a, b in zip(tiles, tiles[1:])):
        raise ValueError("the stage tiles must be strictly increasing")
    return tiles


class StagedTuples(tuple):
    """The tuples of a network with weight sets by stage: a tuple of tuples like any other, with the tiles at which its stages begin
    as `stage_tiles`.  Every host mirror takes `tuples`; handed these, it reads and adds by stage."""
    def __new__(cls, tuples, stage_tiles):
        self = super().__new__(cls, tuples)
        self.stage_tiles = check_stage_tiles(stage_tiles)
        return self


def with_stages(tuples, stage_tiles):
    """`tuples` (checked) carrying `stage_tiles`; with () the plain tuples of the one-stage network."""
    plain = check_tuples(tuple(tuple(t) for t in tuples))
    tiles = check_stage_tiles(stage_tiles)
    return StagedTuples(plain, tiles) if tiles else plain


def stage_tiles_of(tuples) -> tuple:
    """The stage tiles `tuples` carries: () unless they are StagedTuples."""
    return tuple(getattr(tuples, "stage_tiles", ()))


def stage_of_keys_on_host(keys, stage_tiles) -> np.ndarray:
    """int64[len(keys)]: the stage of packed boards = the number of `stage_tiles` whose nibble (log2 of the tile) is at most the board's
    largest nibble.  The empty board is in stage 0; () puts every board there."""
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    top = np.zeros(len(keys), dtype=np.int64)
    for c in range(16):
        top = np.maximum(top, ((keys >> _U64(4 * c)) & _U64(15)).astype(np.int64))
    stage = np.zeros(len(keys), dtype=np.int64)
    for tile in check_stage_tiles(stage_tiles):
        stage += top >= tile.bit_length() - 1
    return stage


def check_lam(lam) -> float:
    """lambda as a float, after the library's own check (ValueError outside [0, 1]; NaN is outside)."""
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam must be in [0, 1]")
    return lam


def tuple_offsets(tuples):
    """(offsets, n_weights): tuple t's table of 16^len weights starts at the sum of the earlier tables' sizes.  n_weights is ONE stage's."""
    sizes = [16 ** len(t) for t in tuples]
    return [sum(sizes[:i]) for i in range(len(sizes))], sum(sizes)


def add_stage_on_host(arrays, tuples, tile, copy=True):
    """add_stage on the host: (the arrays grown by one stage, `tuples` carrying the stage tiles with `tile` among them).  Every array of
    `arrays` holds n_stages slices of equal length along its first axis; the stage that holds `tile` is split at it and the new, upper
    stage's slice is a copy of the slice it is split from (copy: the weights, E and A) or zero (the accumulators).  ValueError if a
    stage begins at `tile` already or MAX_STAGES stages exist."""
    (tile,), old = check_stage_tiles((tile,)), stage_tiles_of(tuples)
    if tile in old:
        raise ValueError(f"a stage begins at tile {tile} already")
    if len(old) + 1 >= MAX_STAGES:
        raise ValueError(f"the network has {MAX_STAGES} stages already")
    tiles = tuple(sorted(old + (tile,)))
    new = tiles.index(tile) + 1                                             # the new stage; it is split from stage new - 1
    grown = []
    for x in arrays:
        rows = np.asarray(x).reshape((len(old) + 1, -1) + np.asarray(x).shape[1:])
        rows = np.insert(rows, new, rows[new - 1] if copy else 0, axis=0)
        grown.append(np.ascontiguousarray(rows.reshape((-1,) + rows.shape[2:])))
    return grown, with_stages(tuples, tiles)


def feature_cells_on_host(tuples, symmetric=True) -> list:
    """Per tuple int64[images, len]: the board cells that feature (tuple, image j) reads, in the tuple's order.  Image j reads the
    cells T_j(board) shows at the tuple's positions: transforms_on_host(4)[j][cell].  images = 8, or 1 (T_0) without `symmetric`."""
    tf = transforms_on_host(4)[:8 if symmetric else 1]
    return [tf[:, list(t)] for t in tuples]


def _nibbles(keys) -> np.ndarray:
    """int64[len(keys), 16]: the nibbles of packed boards uint64[N], cell c in column c."""
    return np.stack([(keys >> _U64(4 * c)) & _U64(15) for c in range(16)], axis=1).astype(np.int64)


def feature_indices_on_host(keys, tuples, symmetric=True) -> np.ndarray:
    """int64[len(keys), F]: the weights an afterstate reads, tuple-major and image j within a tuple (the order V is summed in).  Where
    `tuples` carry stage tiles (with_stages) every index is in the slice of the afterstate's own stage: + stage * n_weights."""
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    nib = _nibbles(keys)
    offsets, n_weights = tuple_offsets(tuples)
    cols = []
    for off, cells in zip(offsets, feature_cells_on_host(tuples, symmetric)):
        for image in cells:
            cols.append(off + sum(nib[:, int(c)] << (4 * i) for i, c in enumerate(image)))
    idx = np.stack(cols, axis=1)
    stage_tiles = stage_tiles_of(tuples)
    return idx + (stage_of_keys_on_host(keys, stage_tiles) * n_weights)[:, None] if stage_tiles else idx


def value_on_host(keys, weights, tuples, symmetric=True) -> np.ndarray:
    """float64[len(keys)]: V = the sum of (double)weights[index] over the features, from 0.0 in the order of feature_indices_on_host,
    one rounding per add."""
    w = np.asarray(weights, dtype=np.float32)[feature_indices_on_host(keys, tuples, symmetric)].astype(np.float64)
    v = np.zeros(w.shape[0], dtype=np.float64)
    for f in range(w.shape[1]):
        v = v + w[:, f]
    return v


# ------------------------------------------------------------------ the environment's move, over many boards
@functools.lru_cache(maxsize=None)
def row_table_on_host():
    """(row after the squash to the left uint16[65536], merge score int64[65536]) of every row of four nibbles (TFE.py:85-101: a
    tile merges with an equal neighbour once): the host's copy of the device's row table (csrc/tfe_device.h)."""
    rows, ar = np.arange(65536, dtype=np.int64), np.arange(65536)
    res, w = np.zeros((65536, 4), dtype=np.int64), np.zeros(65536, dtype=np.int64)
    merged, score = np.zeros(65536, dtype=bool), np.zeros(65536, dtype=np.int64)
    for c in range(4):
        val = (rows >> (4 * c)) & 15
        cur = res[ar, w]
        put = (val != 0) & (cur == 0)
        mrg = (val != 0) & (cur != 0) & (cur == val) & ~merged
        adv = (val != 0) & (cur != 0) & ~mrg
        res[ar[put], w[put]] = val[put]
        res[ar[mrg], w[mrg]] = np.minimum(val[mrg] + 1, 15)
        score[mrg] += np.int64(2) << val[mrg]
        merged[mrg] = True
        w[adv] += 1
        res[ar[adv], w[adv]] = val[adv]
        merged[adv] = False
    return (res[:, 0] | res[:, 1] << 4 | res[:, 2] << 8 | res[:, 3] << 12).astype(np.uint16), score


def moves_on_host(keys):
    """(afterstate keys uint64[N, 4], merge scores int64[N, 4]) of the four moves of packed 4 x 4 boards, without the spawn
    (TFE.py:154-178: the board rotated `a` times, every row squashed to the left, rotated back)."""
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    nib = _nibbles(keys)
    table, table_score = row_table_on_host()
    after, score = np.zeros((len(keys), 4), dtype=_U64), np.zeros((len(keys), 4), dtype=np.int64)
    for a, src in enumerate(transforms_on_host(4)[:4].tolist()):
        for r in range(0, 16, 4):
            row = nib[:, src[r]] | nib[:, src[r + 1]] << 4 | nib[:, src[r + 2]] << 8 | nib[:, src[r + 3]] << 12
            out = table[row].astype(np.int64)
            score[:, a] += table_score[row]
            for c in range(4):
                after[:, a] |= ((out >> (4 * c)) & 15).astype(_U64) << _U64(4 * src[r + c])
    return after, score


def greedy_nt_on_host(keys, weights, tuples, symmetric, gamma: float, tie_seed: int, round: int) -> dict:
    """The roll-out's greedy rule on packed boards: q_a = r_a + gamma * V(B_a) in float64 for the four moves; the candidates are the
    moves with B_a != B, scanned in the order a = 0..3 -- the first is the best so far, a larger q replaces it, an equal q replaces
    it iff bit 31 of word a - 1 of Philox(tie_seed, key of B, round) is set.  Returns action int64[N] (-1: no candidate: the board is
    over), after uint64[N, 4], scores / rewards int64[N, 4], values / q float64[N, 4]."""
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    after, scores = moves_on_host(keys)
    rewards = rewards_of_scores(scores)
    values = value_on_host(after.reshape(-1), weights, tuples, symmetric).reshape(-1, 4)
    q = rewards.astype(np.float64) + float(gamma) * values
    best = greedy_scan_many_on_host(q, philox_many_on_host(tie_seed, keys, int(round)), after != keys[:, None])
    return dict(action=best, after=after, scores=scores, rewards=rewards, values=values, q=q)


# ------------------------------------------------------------------ expectimax search, one chance layer deep
TILE_ODDS = (15099495.0 / 16777216.0, 1677721.0 / 16777216.0)                                 # a 2-tile, a 4-tile (csrc/tfe_device.h: tfe_spawn_packed)


def check_layers(layers) -> int:
    """The search's depth in chance layers as an int: 1 or 2 (ValueError otherwise), as the library checks it."""
    if isinstance(layers, bool) or layers not in (1, 2):
        raise ValueError("layers must be 1 or 2")
    return int(layers)


def check_rollout_layers(layers) -> int:
    """The depth of the search a training roll-out plays under, as an int: 0 (none: the one-ply roll-out, pulse_tfe_nt_rollout), 1 or 2
    chance layers (pulse_tfe_nt_rollout_search).  ValueError otherwise; a bool is no depth."""
    if isinstance(layers, bool) or layers not in (0, 1, 2):
        raise ValueError("rollout_layers must be 0, 1 or 2")
    return int(layers)


def search_backed_on_host(q, candidates) -> np.ndarray:
    """float64[N]: the value the search backs up for a board, from its q float64[N, 4] and candidates bool[N, 4]:
    the largest q over the candidate moves, scanned in the order a = 0..3 -- the first candidate starts, a strictly larger q replaces
    it; +0.0 without a candidate (the board is over).  A maximum: no tie coin, and nothing of the action taken."""
    q, candidates = np.asarray(q, dtype=np.float64).reshape(-1, 4), np.asarray(candidates, dtype=bool).reshape(-1, 4)
    best, found = np.zeros(len(q), dtype=np.float64), np.zeros(len(q), dtype=bool)
    for a in range(4):
        take = candidates[:, a] & (~found | (q[:, a] > best))
        best, found = np.where(take, q[:, a], best), found | candidates[:, a]
    return best


def search_nt_on_host(keys, weights, tuples, symmetric, gamma: float, tie_seed: int, round: int, *, layers: int = 1) -> dict:
    """pulse_tfe_nt_search on the host, word for word.  For a candidate move a of board B (B_a != B) the chance boards of B_a are B_a
    with nibble k = 1, 2 at an empty cell c, slot s = 2 c + (k - 1); m = the best r + gamma * V over the candidate moves of a chance board
    (scanned in the order 0..3, a larger one replaces; 0.0 without a candidate); term_s = P_k * m, +0.0 at a filled cell; S = the pairwise
    tree over the 32 terms (x[0::2] + x[1::2], five times); E_a = S / n_empty(B_a); q_a = r_a + gamma * E_a, +0.0 for a move that is no
    candidate.  The action is greedy_nt_on_host's scan on these q.  Returns q float64[N, 4], action int64[N] (-1: no candidate),
    candidates uint8[N] (bit a), E float64[N, 4] (0.0 for a non-candidate), terms float64[N, 4, 32], and the moves themselves: after
    uint64[N, 4], rewards int64[N, 4]; and backed float64[N], search_backed_on_host of these q and candidates (what
    pulse_tfe_nt_rollout_backed records per move).

    layers = 2 (pulse_tfe_nt_search_deep): m of a chance board C is W2(C), the best over C's candidate moves
    of the q this function gives board C at one layer (the same scan: the first candidate starts, a strictly larger q replaces it;
    +0.0 without a candidate; no tie coins inside the tree); everything else is as above, and `terms` are these outer terms.  The
    one-layer search runs once per distinct chance board.  ValueError for any other `layers`."""
    layers = check_layers(layers)
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    gamma = float(gamma)
    after, scores = moves_on_host(keys)
    cand = after != keys[:, None]
    slot = np.arange(32)
    shift, tile = (_U64(4) * (slot >> 1).astype(_U64)), ((slot & 1) + 1).astype(_U64)
    empty = ((after[:, :, None] >> shift) & _U64(15)) == 0                                     # [N, 4, 32]: the slot's cell is empty in B_a
    live = cand[:, :, None] & empty
    chance = (after[:, :, None] | (tile << shift))[live]
    terms = np.zeros(live.shape, dtype=np.float64)
    if len(chance):
        if layers == 2:
            distinct, at = np.unique(chance, return_inverse=True)
            inner = search_nt_on_host(distinct, weights, tuples, symmetric, gamma, tie_seed, round)
            x, cand2 = inner["q"][at], (inner["after"] != distinct[:, None])[at]
        else:
            after2, scores2 = moves_on_host(chance)
            x = rewards_of_scores(scores2).astype(np.float64) + gamma * value_on_host(after2.reshape(-1), weights, tuples, symmetric).reshape(-1, 4)
            cand2 = after2 != chance[:, None]
        terms[live] = np.broadcast_to(np.array(TILE_ODDS, dtype=np.float64)[slot & 1], live.shape)[live] * search_backed_on_host(x, cand2)
    total = terms
    for _ in range(5):
        total = total[..., 0::2] + total[..., 1::2]
    n_empty = empty[:, :, 0::2].sum(axis=2)
    E = np.where(cand, total[..., 0] / np.maximum(n_empty, 1), 0.0)
    rewards = rewards_of_scores(scores)
    q = np.where(cand, rewards.astype(np.float64) + gamma * E, 0.0)
    action = greedy_scan_many_on_host(q, philox_many_on_host(tie_seed, keys, int(round)), cand)
    return dict(q=q, action=action, candidates=(cand << np.arange(4)).sum(axis=1).astype(np.uint8), E=E, terms=terms, after=after,
                rewards=rewards, backed=search_backed_on_host(q, cand))


# ------------------------------------------------------------------ search depth chosen by the board's empty cells
def check_deep_empty_max(x):
    """The threshold of the adaptive search: None (no adaptive search: the call is what it was) or an int in 0..16, returned as it is
    meant.  ValueError otherwise; a bool is no threshold."""
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) <= 16:
        raise ValueError("deep_empty_max must be None or an int in 0..16")
    return int(x)


def count_empty_on_host(keys) -> np.ndarray:
    """int64[N]: the empty cells (nibbles 0) of packed 4 x 4 boards"""
    return (_nibbles(np.ascontiguousarray(keys, dtype=_U64).reshape(-1)) == 0).sum(axis=1).astype(np.int64)


def search_adaptive_nt_on_host(keys, weights, tuples, symmetric, gamma: float, tie_seed: int, round: int, deep_empty_max: int) -> dict:
    """pulse_tfe_nt_search_adaptive on the host, word for word: a board with at most `deep_empty_max` empty cells gets every row of
    search_nt_on_host(layers=2), every other board those of search_nt_on_host(layers=1); the boards of a depth are searched in one
    call.  Returns search_nt_on_host's dict and deep bool[N]: the board was searched two layers deep."""
    E = check_deep_empty_max(deep_empty_max)
    if E is None:
        raise ValueError("deep_empty_max must be None or an int in 0..16")
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    deep = count_empty_on_host(keys) <= E
    out = search_nt_on_host(keys[:0], weights, tuples, symmetric, gamma, tie_seed, round)       # (the rows' shapes and types)
    out = {k: np.zeros((len(keys),) + v.shape[1:], dtype=v.dtype) for k, v in out.items()}
    for rows, layers in ((~deep, 1), (deep, 2)):
        if rows.any():
            look = search_nt_on_host(keys[rows], weights, tuples, symmetric, gamma, tie_seed, round, layers=layers)
            for k, v in look.items():
                out[k][rows] = v
    return dict(out, deep=deep)


# ------------------------------------------------------------------ restarted roll-outs
def check_restart_fraction(fraction) -> float:
    """The fraction of a game's length its successor starts at, as a float: 0 (off) or inside the open interval (0, 1).  ValueError
    otherwise; NaN is outside."""
    fraction = float(fraction)
    if not 0.0 <= fraction < 1.0:
        raise ValueError("restart_fraction must be 0 (off) or in (0, 1)")
    return fraction


def spawn_on_host(keys, r_cell, r_val) -> np.ndarray:
    """uint64[N]: the environment's spawn (csrc/tfe_device.h: tfe_spawn_packed) on packed 4 x 4 boards, from the two Philox words it
    reads: the tile goes to the k-th empty cell in cell order, k = (r_cell * empty) >> 32, and is nibble 2 (a 4-tile) iff
    (r_val >> 8) > 15099494, else nibble 1.  A full board comes back as it is."""
    keys = np.ascontiguousarray(keys, dtype=_U64).reshape(-1)
    r_cell, r_val = np.asarray(r_cell, dtype=_U64).reshape(-1), np.asarray(r_val, dtype=_U64).reshape(-1)
    free = _nibbles(keys) == 0
    empty = free.sum(axis=1).astype(_U64)
    k = ((r_cell * empty) >> _U64(32)).astype(np.int64)
    cell = (free & (np.cumsum(free, axis=1) - 1 == k[:, None])).argmax(axis=1).astype(_U64)
    tile = np.where((r_val >> _U64(8)) > _U64(15099494), _U64(2), _U64(1))
    return keys | np.where(empty > 0, tile << (_U64(4) * cell), _U64(0))


def restart_pick_on_host(keys, lengths, max_steps, env_seed, board_id0, fraction, min_length):
    """pulse_tfe_nt_restart_pick on the host.  keys uint64[T, B] and lengths int[B] of a recorded round (T at least the longest game),
    env_seed and board_id0 those it was recorded under.  L = min(lengths[g], max_steps), t* = floor(float64(L) * fraction); where
    L >= min_length and 1 <= t* <= L - 1, start[g] = the board move t* was made on: spawn_on_host of keys[t* - 1, g] under words x and
    y of Philox(env_seed, board_id0 + g, t*); 0 elsewhere.  Returns (start uint64[B], picked (the boards picked, the sum of their t*))."""
    keys = np.asarray(keys, dtype=_U64)
    L = np.minimum(np.asarray(lengths, dtype=np.int64).reshape(-1), int(max_steps))
    at = np.floor(L.astype(np.float64) * np.float64(fraction)).astype(np.int64)
    g = np.flatnonzero((L >= int(min_length)) & (at >= 1) & (at <= L - 1))
    start = np.zeros(len(L), dtype=_U64)
    if len(g):
        ids = np.array([(int(board_id0) + int(i)) & 0xFFFFFFFFFFFFFFFF for i in g], dtype=_U64)
        draws = philox_many_on_host(int(env_seed), ids, at[g].astype(_U64))
        start[g] = spawn_on_host(keys[at[g] - 1, g], draws[:, 0], draws[:, 1])
    return start, (len(g), int(at[g].sum()))


def restart_summary_on_host(words, start) -> dict:
    """restart_stats' two words and `start` as {"picked", "mean_depth", "started"}: mean_depth = words[1] / words[0] (0.0 where nothing
    was picked), started = the non-zero entries of start."""
    picked, total = int(words[0]), int(words[1])
    return dict(picked=picked, mean_depth=total / picked if picked else 0.0, started=int(np.count_nonzero(start)))


# ------------------------------------------------------------------ games continued across rounds
FINISHED_SUMMARY = ("games", "moves", "score_sum", "score_sq_sum", "max_score", "continued", "resumed", "tile_capped")     # words 0..7 of `finished`


def continue_pick_on_host(keys, steps, lengths, total_score, max_steps, env_seed, board_id0, carry_score, carry_moves):
    """pulse_tfe_nt_continue_pick on the host.  keys uint64[T, B], steps uint8[T, B], lengths int[B] and total_score int64[B] of a
    recorded round (T at least the longest game), env_seed and board_id0 those it was recorded under, carry_score int64[B] and
    carry_moves int[B] as the launch finds them (not written).  L = min(lengths[g], max_steps), b = steps[L - 1, g], A = keys[L - 1, g].
    A game is CUT where b has no terminal bit, A holds no nibble 15 and L == max_steps: start[g] = spawn_on_host of keys[L - 2, g] under
    words x and y of Philox(env_seed, board_id0 + g, L - 1), the board move L - 1 was made on; carry_score[g] += total_score[g] - sc, sc
    the merge score of that board's move b & 3 (moves_on_host), carry_moves[g] += L - 1.  AssertionError if that move does not give A:
    the device does not check it.  Every other game is FINISHED: its score carry_score[g] + total_score[g], its length carry_moves[g] +
    L and the largest tile of A with the spawn of Philox(env_seed, board_id0 + g, L) go into the 24 words (FINISHED_SUMMARY, then the
    histogram), and start[g] and both carries are 0.  Returns (start uint64[B], carry_score int64[B], carry_moves int32[B], the 24 words
    this launch adds as Python ints; word 4 is a maximum)."""
    keys, steps = np.asarray(keys, dtype=_U64), np.asarray(steps, dtype=np.uint8)
    max_steps = int(max_steps)
    if not 2 <= max_steps <= 65535:
        raise ValueError("max_steps must be in 2..65535")
    L = np.minimum(np.asarray(lengths, dtype=np.int64).reshape(-1), max_steps)
    assert (L >= 1).all(), "a recorded game has a move"
    B = len(L)
    g = np.arange(B)
    total = np.asarray(total_score, dtype=np.int64).reshape(-1)
    score, moves = np.array(carry_score, dtype=np.int64).reshape(-1), np.array(carry_moves, dtype=np.int64).reshape(-1)
    b, A = steps[L - 1, g], keys[L - 1, g]
    capped = (_nibbles(A) == 15).any(axis=1)
    cut = (b >> 7 == 0) & ~capped & (L == max_steps)
    ids = np.array([(int(board_id0) + int(i)) & 0xFFFFFFFFFFFFFFFF for i in g], dtype=_U64)
    draws = philox_many_on_host(int(env_seed), ids, np.where(cut, L - 1, L).astype(_U64))
    start, words = np.zeros(B, dtype=_U64), [0] * (len(FINISHED_SUMMARY) + EVAL_BINS)
    c, f = np.flatnonzero(cut), np.flatnonzero(~cut)
    if len(c):
        start[c] = spawn_on_host(keys[L[c] - 2, c], draws[c, 0], draws[c, 1])
        after, scores = moves_on_host(start[c])
        a = (b[c] & 3).astype(np.int64)
        assert np.array_equal(after[np.arange(len(c)), a], A[c]), "the cut move made again does not give the recorded afterstate"
        score[c] += total[c] - scores[np.arange(len(c)), a]
        moves[c] += L[c] - 1
        words[5] = len(c)
    if len(f):
        s = (score[f] + total[f]).astype(object)                           # (Python ints: the sum of squares is exact)
        top = _nibbles(spawn_on_host(A[f], draws[f, 0], draws[f, 1])).max(axis=1)
        words[:5] = [len(f), int((moves[f] + L[f]).sum()), int(s.sum()), int((s * s).sum()), int(s.max())]
        words[6], words[7] = int((moves[f] > 0).sum()), int(capped[f].sum())
        words[len(FINISHED_SUMMARY):] = np.bincount(top, minlength=EVAL_BINS).tolist()
        score[f], moves[f] = 0, 0
    return start, score, moves.astype(np.int32), words


def add_finished_on_host(words, more) -> list:
    """`finished` after a launch that adds `more` to `words`: every word a sum but word 4, the largest score."""
    return [max(int(x), int(y)) if i == 4 else int(x) + int(y) for i, (x, y) in enumerate(zip(words, more))]


def finished_summary_on_host(words) -> dict:
    """`finished`'s 8 + 16 words as a dict (tfe_common.eval_summary_on_host with FINISHED_SUMMARY): the whole games that ended since the
    words were zeroed -- mean_score, std_score and mean_length are theirs -- `continued` the games the pick launches took on into
    another round, `resumed` the finished games that had been continued at least once."""
    return _eval_summary_on_host(words, FINISHED_SUMMARY)


# ------------------------------------------------------------------ the learner and the apply launch
def _add_moves_on_host(keys, steps, lengths, deltas, tuples, symmetric, acc, acc_abs=None) -> dict:
    """The learners' tail.  A game has L = min(lengths[g], T) moves; its last is skipped without its terminal bit; any other move (t, g),
    t < L, has deltas[t, g] clamped to +-DELTA_MAX, d = round-half-even(that * 2^16), and sum += d, cnt += 1 at every feature of
    keys[t, g] (a weight two images meet gets both).  acc int64[W, 2] = {sum, cnt}, in place; with acc_abs int64[W] also
    acc_abs += |d| at the same features.  Returns dict(learnt, skipped, clamped)."""
    L = np.minimum(np.asarray(lengths, dtype=np.int64).reshape(-1), keys.shape[0])
    t = np.arange(keys.shape[0], dtype=np.int64)[:, None]
    played = t < L[None, :]
    skipped = played & (t == L[None, :] - 1) & (steps >> 7 == 0)
    learn = played & ~skipped
    delta = deltas[learn]
    clamped = np.abs(delta) > DELTA_MAX
    d = np.rint(np.ldexp(np.clip(delta, -DELTA_MAX, DELTA_MAX), FRAC_BITS)).astype(np.int64)
    idx = feature_indices_on_host(keys[learn], tuples, symmetric)
    np.add.at(acc[:, 0], idx.reshape(-1), np.repeat(d, idx.shape[1]))
    np.add.at(acc[:, 1], idx.reshape(-1), 1)
    if acc_abs is not None:
        np.add.at(acc_abs, idx.reshape(-1), np.repeat(np.abs(d), idx.shape[1]))
    return dict(learnt=int(learn.sum()), skipped=int(skipped.sum()), clamped=int(clamped.sum()))


def learn_nt_on_host(keys, values, steps, lengths, tuples, symmetric, gamma: float, acc, acc_abs=None):
    """pulse_tfe_nt_learn on the host.  keys uint64[T, B], values float64[T, B], steps uint8[T, B], lengths int[B] (a game has
    min(lengths[g], T) moves); acc int64[W, 2] = {sum, cnt}, added to in place.  The last move of a game has target 0; any other has
    target = reward(steps[t + 1]) + gamma * values[t + 1]; delta = target - values[t], added by _add_moves_on_host (to acc_abs too,
    where one is given).  Returns dict(learnt, skipped, clamped)."""
    keys, values, steps = np.asarray(keys, dtype=_U64), np.asarray(values, dtype=np.float64), np.asarray(steps, dtype=np.uint8)
    T = keys.shape[0]
    last = np.arange(T, dtype=np.int64)[:, None] == np.minimum(np.asarray(lengths, dtype=np.int64).reshape(-1), T)[None, :] - 1
    nxt_r, nxt_v = np.zeros_like(values), np.zeros_like(values)
    nxt_r[:-1], nxt_v[:-1] = ((steps[1:] >> 2) & 31).astype(np.float64), values[1:]
    target = np.where(last, 0.0, nxt_r + float(gamma) * nxt_v)
    return _add_moves_on_host(keys, steps, lengths, target - values, tuples, symmetric, acc, acc_abs)


def _walk_deltas_on_host(values, steps, lengths, gamma, lam, backed=None) -> np.ndarray:
    """The learners' backward walk, operation for operation: gl = gamma * lam (one multiply); at a game's last move D = 0 - values[t] with
    its terminal bit and +0.0 without (the move is skipped); at any other D_t = (target - values[t]) + gl * D_{t+1}, unclamped, where
    target = reward(steps[t + 1]) + gamma * values[t + 1], or with `backed` backed[t + 1].  Rows at or beyond a game's length are 0."""
    values, steps = np.asarray(values, dtype=np.float64), np.asarray(steps, dtype=np.uint8)
    T = values.shape[0]
    L = np.minimum(np.asarray(lengths, dtype=np.int64).reshape(-1), T)
    gamma, gl = np.float64(gamma), np.float64(gamma) * np.float64(lam)
    out, carried = np.zeros(values.shape, dtype=np.float64), np.zeros(values.shape[1], dtype=np.float64)
    for t in range(int(L.max()) - 1 if L.size else -1, -1, -1):
        last, played = t == L - 1, t < L
        nxt = t + 1 if t + 1 < T else t                                    # (row T does not exist; a move at T - 1 is a last move)
        with np.errstate(all="ignore"):                                    # (what a lane computes on rows beyond its game is not used)
            target = backed[nxt] if backed is not None else ((steps[nxt] >> 2) & 31).astype(np.float64) + gamma * values[nxt]
            delta = np.where(last, 0.0, target) - values[t]
            through = delta + gl * carried
        carried = np.where(last, np.where(steps[t] >> 7 != 0, delta, 0.0), through)
        carried = np.where(played, carried, 0.0)
        out[t] = carried
    return out


def lambda_deltas_on_host(values, steps, lengths, gamma: float, lam: float) -> np.ndarray:
    """float64[T, B]: the lambda-differences pulse_tfe_nt_learn_lambda writes, operation for operation.  values float64[T, B], steps
    uint8[T, B], lengths int[B] (a game has min(lengths[g], T) moves).  gl = gamma * lam (one multiply); at a game's last move
    D = 0 - values[t] with its terminal bit and +0.0 without (the move is skipped); at any other D_t = ((reward(steps[t + 1]) + gamma *
    values[t + 1]) - values[t]) + gl * D_{t+1}, unclamped.  Rows at or beyond a game's length are returned as 0 (the device does
    not write them: they keep what `deltas` held)."""
    return _walk_deltas_on_host(values, steps, lengths, gamma, lam)


def learn_lambda_nt_on_host(keys, values, steps, lengths, tuples, symmetric, gamma: float, lam: float, acc, acc_abs=None) -> dict:
    """pulse_tfe_nt_learn_lambda on the host: learn_nt_on_host with lambda_deltas_on_host's D_t in place of the one-step difference.
    The skipped moves, the clamp to +-DELTA_MAX (applied to the add only: the recurrence carries the unclamped D), d and the adds are
    _add_moves_on_host's.  Returns dict(learnt, skipped, clamped, deltas float64[T, B])."""
    keys, values, steps = np.asarray(keys, dtype=_U64), np.asarray(values, dtype=np.float64), np.asarray(steps, dtype=np.uint8)
    deltas = lambda_deltas_on_host(values, steps, lengths, gamma, lam)
    return dict(_add_moves_on_host(keys, steps, lengths, deltas, tuples, symmetric, acc, acc_abs), deltas=deltas)


def backed_deltas_on_host(values, backed, steps, lengths, gamma: float, lam: float) -> np.ndarray:
    """float64[T, B]: the differences pulse_tfe_nt_learn_backed writes, operation for operation.  values and
    backed float64[T, B], steps uint8[T, B], lengths int[B] (a game has min(lengths[g], T) moves).  gl = gamma * lam (one multiply); at a
    game's last move D = 0 - values[t] with its terminal bit and +0.0 without (the move is skipped); at any other D_t = (backed[t + 1] -
    values[t]) + gl * D_{t+1}, unclamped: backed[t + 1] holds the next reward and its own gamma.  Rows at or beyond a game's length are
    returned as 0 (the device does not write them: they keep what `deltas` held)."""
    return _walk_deltas_on_host(values, steps, lengths, gamma, lam, np.asarray(backed, dtype=np.float64))


def learn_backed_nt_on_host(keys, values, backed, steps, lengths, tuples, symmetric, gamma: float, lam: float, acc, acc_abs=None) -> dict:
    """pulse_tfe_nt_learn_backed on the host: learn_lambda_nt_on_host with backed_deltas_on_host's D_t.  The skipped moves, the clamp
    to +-DELTA_MAX (applied to the add only), d and the adds -- to acc_abs too, where one is given -- are _add_moves_on_host's.
    Returns dict(learnt, skipped, clamped, deltas float64[T, B])."""
    keys, steps = np.asarray(keys, dtype=_U64), np.asarray(steps, dtype=np.uint8)
    deltas = backed_deltas_on_host(values, backed, steps, lengths, gamma, lam)
    return dict(_add_moves_on_host(keys, steps, lengths, deltas, tuples, symmetric, acc, acc_abs), deltas=deltas)


def apply_nt_on_host(weights, acc, step: float) -> int:
    """pulse_tfe_nt_apply on the host, in place: where cnt > 0, w = float32(float64(w) + step * ((sum / cnt) * 2^-16)), one rounding per
    operation, and the two accumulator words become 0.  Returns the number of weights moved."""
    at = np.flatnonzero(acc[:, 1] > 0)
    mean = acc[at, 0].astype(np.float64) / acc[at, 1].astype(np.float64) * 2.0 ** -FRAC_BITS
    weights[at] = (weights[at].astype(np.float64) + float(step) * mean).astype(np.float32)
    acc[at] = 0
    return len(at)


def learn_tc_nt_on_host(keys, values, steps, lengths, tuples, symmetric, gamma: float, lam: float, acc, acc_abs) -> dict:
    """pulse_tfe_nt_learn_tc on the host: learn_nt_on_host (lam == 0) or learn_lambda_nt_on_host (lam > 0) with the third accumulator,
    acc_abs int64[W] += |d| wherever those add sum += d, cnt += 1.  Returns what they return."""
    if float(lam) > 0.0:
        return learn_lambda_nt_on_host(keys, values, steps, lengths, tuples, symmetric, gamma, lam, acc, acc_abs)
    return learn_nt_on_host(keys, values, steps, lengths, tuples, symmetric, gamma, acc, acc_abs)


def apply_tc_nt_on_host(weights, acc, acc_abs, E, A, step: float):
    """pulse_tfe_nt_apply_tc on the host, in place, float64 with one rounding per operation.  Where cnt > 0: m = (sum / cnt) * 2^-16,
    a = (abs / cnt) * 2^-16, rho = |E| / A where A > 0 and 1.0 otherwise -- from E and A as they stand, before this round's are added --
    w = float32(float64(w) + (step * rho) * m), E = E + m, A = A + a, and the three accumulator words become 0.  A weight with
    cnt == 0 keeps its bits, its E and its A.  Returns (weights moved, the sum over them of round-half-even(rho * 2^32)): what the
    launch adds to tc_stats."""
    at = np.flatnonzero(acc[:, 1] > 0)
    cnt = acc[at, 1].astype(np.float64)
    m = acc[at, 0].astype(np.float64) / cnt * 2.0 ** -FRAC_BITS
    a = acc_abs[at].astype(np.float64) / cnt * 2.0 ** -FRAC_BITS
    e0, a0 = E[at], A[at]
    rho = np.ones(len(at), dtype=np.float64)
    pos = a0 > 0.0
    rho[pos] = np.abs(e0[pos]) / a0[pos]
    weights[at] = (weights[at].astype(np.float64) + (np.float64(step) * rho) * m).astype(np.float32)
    E[at], A[at] = e0 + m, a0 + a
    acc[at] = 0
    acc_abs[at] = 0
    return len(at), int(np.rint(np.ldexp(rho, TC_RHO_BITS)).astype(np.int64).sum())


def tc_summary_on_host(words) -> dict:
    """tc_stats' words as {"moved", "mean_rho"}: mean_rho = words[1] / words[0] * 2^-32, 1.0 where nothing moved."""
    moved, total = int(words[0]), int(words[1])
    return dict(moved=moved, mean_rho=(total / moved) * 2.0 ** -TC_RHO_BITS if moved else 1.0)


def eval_summary_on_host(words) -> dict:
    """pulse_tfe_nt_evaluate's 8 + 16 counters as a dict (tfe_common.eval_summary_on_host with this agent's EVAL_SUMMARY)."""
    return _eval_summary_on_host(words, EVAL_SUMMARY)


# ------------------------------------------------------------------ the checkpoint file
def write_checkpoint(path, weights, tuples, lam=0.0, tc=None, stage_tiles=(), **scalars) -> None:
    """The network as an .npz of plain arrays (np.savez, no pickles): the non-zero weights as index int64[m] (ascending) and value
    float32[m], the tuples as tuple_len int64[n_tuples] and tuple_cells int64[n_tuples, 6] (-1 beyond a tuple's length), the scalars of
    CHECKPOINT_SCALARS as 0-d arrays and `version`.  lam == 0 writes exactly that, as version 1; any other `lam` adds a 0-d float64
    `lam` and writes version 2.  tc = (E, A), float64[n_weights] each, writes version 4: version 2's arrays with `lam` whatever its
    value, tc_index int64[m'] (ascending: the weights whose E or A is not +0.0 by bit pattern) and tc_e / tc_a float64[m'].
    stage_tiles other than () writes version 5: version 2's arrays (with `lam` whatever its value) or, with tc, version 4's, every index
    over the S * W weights of the staged network, and stage_tiles int64[S - 1].  `path` is written as given."""
    if sorted(scalars) != sorted(CHECKPOINT_SCALARS):
        raise ValueError(f"a checkpoint holds exactly the scalars {CHECKPOINT_SCALARS}")
    weights = np.asarray(weights, dtype=np.float32).reshape(-1)
    index = np.flatnonzero(weights.view(np.uint32) != 0)                   # by bit pattern: what is not +0.0 is kept
    cells = np.full((len(tuples), MAX_LEN), -1, dtype=np.int64)
    for i, t in enumerate(tuples):
        cells[i, :len(t)] = t
    dtypes = dict(gamma=np.float64, epsilon=np.float64, alpha=np.float64, seed=np.uint64, board_id0=np.uint64)
    arrays = {k: np.array(scalars[k], dtype=dtypes.get(k, np.int64)) for k in CHECKPOINT_SCALARS}
    version, stage_tiles = CHECKPOINT_VERSION, check_stage_tiles(stage_tiles)
    if float(lam) != 0.0 or tc is not None or stage_tiles:
        arrays["lam"], version = np.array(lam, dtype=np.float64), CHECKPOINT_VERSION_LAMBDA
    if tc is not None:
        E, A = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in tc)
        if E.shape != weights.shape or A.shape != weights.shape:
            raise ValueError("tc = (E, A), one float64 per weight each")
        at = np.flatnonzero((E.view(np.uint64) != 0) | (A.view(np.uint64) != 0))
        arrays.update(tc_index=at.astype(np.int64), tc_e=E[at], tc_a=A[at])
        version = CHECKPOINT_VERSION_TC
    if stage_tiles:
        arrays["stage_tiles"], version = np.array(stage_tiles, dtype=np.int64), CHECKPOINT_VERSION_STAGED
    with open(path, "wb") as fh:
        np.savez(fh, version=np.array(version, dtype=np.int64), index=index.astype(np.int64), value=weights[index],
                 tuple_len=np.array([len(t) for t in tuples], dtype=np.int64), tuple_cells=cells, **arrays)


def read_checkpoint(path) -> dict:
    """What write_checkpoint wrote (np.load with allow_pickle=False), version 1, 2, 4 or 5: `tuples`, `index`, `value`, `n_weights`, the
    scalars as Python numbers, `lam` (0.0 for version 1), `tc` (False for versions 1 and 2) and `stage_tiles` (() below version 5); with
    tc also `tc_index`, `tc_e` and `tc_a`.  For version 5 `n_weights` is S * W, all stages', and `tc` says whether the file holds the tc
    arrays.  ValueError for another format version, a missing array, tuples or stage tiles the library would refuse or an index outside
    the network."""
    with np.load(path, allow_pickle=False) as f:
        missing = [k for k in ("version", "index", "value", "tuple_len", "tuple_cells") + CHECKPOINT_SCALARS if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not an n-tuple network checkpoint (no {missing})")
        version = int(f["version"])
        if version not in (CHECKPOINT_VERSION, CHECKPOINT_VERSION_LAMBDA, CHECKPOINT_VERSION_TC, CHECKPOINT_VERSION_STAGED):
            raise ValueError(f"{path}: format version {version}, this package reads {CHECKPOINT_VERSION}, {CHECKPOINT_VERSION_LAMBDA}, "
                             f"{CHECKPOINT_VERSION_TC} and {CHECKPOINT_VERSION_STAGED}")
        if version == CHECKPOINT_VERSION_STAGED and "stage_tiles" not in f.files:
            raise ValueError(f"{path}: format version {version} is a staged network's, and the file holds no stage_tiles")
        tc_names = ("tc_index", "tc_e", "tc_a")
        has_tc = version == CHECKPOINT_VERSION_TC or (version == CHECKPOINT_VERSION_STAGED and any(k in f.files for k in tc_names))
        more = ("lam",) * (version != CHECKPOINT_VERSION) + tc_names * has_tc
        if version == CHECKPOINT_VERSION_STAGED:
            more += ("stage_tiles",)
        missing = [k for k in more if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not an n-tuple network checkpoint (no {missing})")
        out = {k: (float(f[k]) if k in ("gamma", "epsilon", "alpha") else int(f[k])) for k in CHECKPOINT_SCALARS}
        out["lam"] = float(f["lam"]) if "lam" in more else 0.0
        out["tc"] = has_tc
        index, value, lens, cells = f["index"], f["value"], f["tuple_len"], f["tuple_cells"]
        tc_arrays = [f[k] for k in tc_names * has_tc]
        out["stage_tiles"] = check_stage_tiles(f["stage_tiles"].tolist()) if version == CHECKPOINT_VERSION_STAGED else ()
    if version == CHECKPOINT_VERSION_STAGED and not out["stage_tiles"]:
        raise ValueError(f"{path}: a version {CHECKPOINT_VERSION_STAGED} checkpoint holds at least one stage tile")
    out["symmetric"] = bool(out["symmetric"])
    out["tuples"] = with_stages([cells[i, :int(n)].tolist() for i, n in enumerate(lens.tolist())], out["stage_tiles"])
    out["n_weights"] = tuple_offsets(out["tuples"])[1] * (len(out["stage_tiles"]) + 1)
    def check_sparse(name, index, others, dtype, shapes):
        """index int64[m], strictly ascending inside the network, and `others` of `dtype` in its shape (ValueError)"""
        if index.dtype != np.int64 or index.ndim != 1 or any(x.dtype != dtype or x.shape != index.shape for x in others):
            raise ValueError(f"{path}: {shapes}")
        if len(index) and (int(index[0]) < 0 or int(index[-1]) >= out["n_weights"] or not bool((index[1:] > index[:-1]).all())):
            raise ValueError(f"{path}: {name} must be strictly ascending inside the network's {out['n_weights']} weights")
    check_sparse("index", index, [value], np.float32, "index must be int64[m] and value float32[m]")
    out["index"], out["value"] = index, value
    if out["tc"]:
        check_sparse("tc_index", tc_arrays[0], tc_arrays[1:], np.float64, "tc_index must be int64[m] and tc_e / tc_a float64[m]")
        out["tc_index"], out["tc_e"], out["tc_a"] = tc_arrays
    return out


def coherence_of_checkpoint(f: dict):
    """(E, A), float64[n_weights] each, of a version-4 read_checkpoint dict."""
    E, A = np.zeros(f["n_weights"], dtype=np.float64), np.zeros(f["n_weights"], dtype=np.float64)
    E[f["tc_index"]], A[f["tc_index"]] = f["tc_e"], f["tc_a"]
    return E, A


def weights_of_checkpoint(f: dict) -> np.ndarray:
    """float32[n_weights] of a read_checkpoint dict."""
    w = np.zeros(f["n_weights"], dtype=np.float32)
    w[f["index"]] = f["value"]
    return w


# ------------------------------------------------------------------ the device agent
class _TakesStageTiles(type):
    """The agent's call: NTupleTDAfterstateTFEGPU(..., stage_tiles=()) sets the attribute `stage_tiles` (checked) before __init__ runs,
    which takes the other arguments.  __init__'s own parameters are the agent's as it was without stages -- the tests of sections 13.6
    and 13.7 hold them to that list -- and the opt-ins since are attributes; this one sizes the allocations, so it has to be known when
    __init__ makes them.  Two consequences: inspect.signature of the class shows this call's (*args, stage_tiles=(), **kw), not
    __init__'s parameters (ask inspect.signature(cls.__init__) for those), and a subclass that builds instances another way -- its own
    __new__, a classmethod that calls __init__ itself -- must set `stage_tiles` on the instance before __init__ runs, or leave the
    class's default (): the one-stage network."""
    def __call__(cls, *args, stage_tiles=(), **kw):
        self = cls.__new__(cls)
        self.stage_tiles = check_stage_tiles(stage_tiles)
        self.__init__(*args, **kw)
        return self


class NTupleTDAfterstateTFEGPU(_TFEGamesGPU, metaclass=_TakesStageTiles):
    """`learn_batch` = `rollout` + `learn` + `apply` + `round += 1`: three launches and no synchronisation.  Everything that reads
    back (`weights`, `stats`, `trajectory`, `evaluate`, the per-game arrays' `.cpu()`) synchronises.  Round r plays the boards
    board_id0 + r * n_games + g, so no two rounds replay the same spawns.  `lam` > 0: `learn` is the TD(lambda) launch and the agent
    holds `deltas`, float64 in the shape of `values`; `lam` = 0 (the default) allocates nothing more and learns by TD(0).  `tc`:
    temporal-coherence step sizes (section 13.3): `learn` is pulse_tfe_nt_learn_tc under the agent's `lam`, `apply` is
    pulse_tfe_nt_apply_tc, and the agent holds `acc_abs`, `E`, `A` and `tc_stats`; without it (the default) none of them exists.
    `rollout_layers` (an attribute, 0 by default; section 13.5): 1 or 2 and `rollout`, so `learn_batch`, plays its games under
    expectimax search that many chance layers deep and records them as before; it is how rounds are played, not part of the network,
    so no checkpoint holds it.  `backed_targets` (an attribute, False by default; section 13.6): with `rollout_layers` 1 or 2, `rollout`
    also records the search's backed-up value of every move's board in `backed` (float64 in the shape of `values`, allocated at the
    first such launch) and `learn` is pulse_tfe_nt_learn_backed under the agent's `lam` and `tc`; it says how rounds are learnt, so
    no checkpoint holds it either.  `restart_fraction` (an attribute, 0.0 by default: off; section 13.7): in (0, 1) and `learn_batch`
    ends with the pick launch, which fills `start` (uint64[n_games], allocated at first use, as `restart_stats` int64[2] is) from the
    games of at least `restart_min_length` moves (an attribute, 64 by default: a starting point, not tuned), and `rollout` starts the
    next round's games there; with `rollout_layers` 2 it is refused.  No checkpoint holds either, and `start` is not saved: a loaded
    agent's next round starts at the reset boards.  `stage_tiles` (section 13.9; () by default: the agent as it was, launches, allocations
    and checkpoint files): up to three tiles, powers of two, strictly increasing, at which the stages 1, 2, ... begin.  `weights_dev`,
    `acc` and the TC state then hold S * W words, stage s in [s * W, (s + 1) * W) with W = `n_weights`; rollout, learn, evaluate,
    evaluate_search and search go through the `pulse_tfe_nt_*_staged` entry points under the agent's `lam`, `tc`, `rollout_layers` 0 or
    1, `backed_targets` and `restart_fraction`, and apply is one launch per stage; two chance layers are refused (ValueError, before
    anything is touched).  `tuples` carries the stage tiles (with_stages), so the host mirrors handed `agent.tuples` read by stage.
    `continue_games` (an attribute, False by default: the agent as it was; section 13.10): on an agent built with a small `max_steps`
    = K >= 2, a game a round cuts at K moves is taken up again by the next round instead of being reset: `learn_batch` ends with the
    continue pick, a fourth launch, which fills `start` with the board the cut move was made on, and `rollout` plays from `start`
    (rollout_from_launch, or the staged launch) at `rollout_layers` 0 or 1 with `backed_targets`, `lam`, `tc` and `stage_tiles` as
    they are; not with `restart_fraction` > 0 nor two layers (ValueError before anything is touched).  `carry_score` int64[n_games]
    and `carry_moves` int32[n_games] hold the games so far, `finished` int64[24] the whole games that ended (`finished_summary`);
    the three are allocated by the first continue launch.  `total_score`, `lengths` and stats() stay per segment.  A lambda-walk ends
    at the segment's cut.  No checkpoint holds any of it: a loaded agent's games begin at their resets.  `eval_max_steps` (an
    attribute, None by default: the agent's `max_steps`): the cap of evaluate_launch's games, so of evaluate and evaluate_search, any
    value in 1..65,535 -- the evaluation launches hold no per-move buffers."""
    STATS, EVAL_SUMMARY = STATS, EVAL_SUMMARY
    continue_games = False                                                 # set on the agent; checked at the launch
    eval_max_steps = None                                                  # set on the agent; None: the agent's max_steps
    carry_score = carry_moves = finished = None                            # allocated by the first continue launch
    restart_fraction = 0.0                                                 # set on the agent; checked at the launch (check_restart_fraction)
    restart_min_length = 64                                                # set on the agent; checked by the pick launch
    start = restart_stats = None                                           # allocated by the first restart launch
    rollout_layers = 0                                                     # set on the agent; checked at the launch (check_rollout_layers)
    backed_targets = False                                                 # set on the agent; checked at the launch, with rollout_layers
    stage_tiles = ()                                                       # set by the call (stage_tiles=...), before __init__ allocates; add_stage grows it

    def __init__(self, device, n_games, tuples=DEFAULT_TUPLES, symmetric=True, gamma=1.0, epsilon=0.0, alpha=1.0, max_steps=4096, seed=0,
                 board_id0=0, lam=0.0, tc=False):
        import torch
        self.lam, self.tc, self.stage_tiles = check_lam(lam), bool(tc), check_stage_tiles(self.stage_tiles or stage_tiles_of(tuples))
        super().__init__(device, n_games, 4, max_steps, gamma, epsilon, seed, board_id0)
        self.tuples, self.symmetric, self.alpha = with_stages(tuples, self.stage_tiles), bool(symmetric), float(alpha)
        self.n_features = len(self.tuples) * (8 if self.symmetric else 1)
        if not 0.0 < self.alpha <= self.n_features:
            raise ValueError("alpha must be in (0, F]: the apply launch takes step = alpha / F in (0, 1]")
        self.offsets, self.n_weights = tuple_offsets(self.tuples)
        self.weights_dev = torch.zeros(self.total_weights, dtype=torch.float32, device=self.device)
        self.acc = torch.zeros((self.total_weights, 2), dtype=torch.int64, device=self.device)        # {sum, cnt}; torch allocations are 16-byte aligned
        self.values = torch.zeros((self.max_steps, self.n_games), dtype=torch.float64, device=self.device)
        self.deltas = torch.zeros_like(self.values) if self.lam > 0.0 else None
        self.acc_abs = self.E = self.A = self.tc_stats = self.backed = None
        if self.tc:
            self._tc_state()

    # ------------------------------------------------------------------ weight sets by tile stage
    @property
    def n_stages(self) -> int:
        return len(self.stage_tiles) + 1

    @property
    def total_weights(self) -> int:
        """The weights of all stages: n_stages * n_weights (n_weights is one stage's, what the library's network struct holds)."""
        return self.n_stages * self.n_weights

    def _stages(self):
        """PulseTfeNtStages of the agent's stage tiles: threshold[s - 1] = log2 of the tile at which stage s begins."""
        st = _native.TfeNtStages()
        st.n_stages = self.n_stages
        for i, tile in enumerate(self.stage_tiles):
            st.threshold[i] = tile.bit_length() - 1
        return st

    def _refuse_two_layers(self, layers, what):
        if self.stage_tiles and layers == 2:
            raise ValueError(f"{what} = 2 on an agent with stage_tiles: two chance layers are not built on stages")

    def add_stage(self, tile):
        """Weight promotion: the stage that holds `tile` is split at it.  The new, upper stage's weights -- with tc its E and A too --
        start as a copy of the stage it is split from, and its accumulators are zero, so V of every board is what it was right after
        the call; from then on the boards whose largest tile has reached `tile` learn apart.  ValueError if `tile` is no stage tile,
        begins a stage already, or the agent has MAX_STAGES stages.  Reallocates `weights_dev`, `acc` and the TC state."""
        import torch
        (tile,) = check_stage_tiles((tile,))
        if tile in self.stage_tiles:
            raise ValueError(f"a stage begins at tile {tile} already")
        if self.n_stages >= MAX_STAGES:
            raise ValueError(f"the agent has {MAX_STAGES} stages already")
        tiles = tuple(sorted(self.stage_tiles + (tile,)))
        new = tiles.index(tile) + 1                                         # the new stage; it is split from stage new - 1
        source = [s if s < new else s - 1 for s in range(len(tiles) + 1)]
        W = self.n_weights

        def grown(t, copy):
            rows = t.reshape(self.n_stages, -1)
            out = torch.stack([rows[src] if copy or s != new else torch.zeros_like(rows[src]) for s, src in enumerate(source)])
            return out.reshape((len(source) * W,) + tuple(t.shape[1:])).contiguous()
        self.weights_dev, self.acc = grown(self.weights_dev, True), grown(self.acc, False)
        if self.acc_abs is not None:
            self.acc_abs, self.E, self.A = grown(self.acc_abs, False), grown(self.E, True), grown(self.A, True)
        self.stage_tiles = tiles
        self.tuples = with_stages(self.tuples, tiles)
        return self

    def rollout_staged_launch(self, layers, backed=False):
        """pulse_tfe_nt_rollout_staged alone: rollout_from_launch's games (layers 0 or 1, `backed` with 1) with V read by stage, begun
        on the boards of `start` where usable."""
        self._refuse_two_layers(layers, "layers")
        args = self._from_args(layers, backed)
        return self._launch("pulse_tfe_nt_rollout_staged", self._rollout_struct(), C.byref(self._stages()), *args)

    def learn_staged_launch(self, lam, backed=False, tc=False):
        """pulse_tfe_nt_learn_staged alone on the games last played: learn()'s adds (lam == 0 without backed: no deltas), the walk of
        learn_lambda_launch (lam > 0) or of learn_backed_launch (backed) into `deltas` first, with tc |d| into `acc_abs` as well; every
        move's adds go to the stage of its afterstate.  Allocates what the agent lacks of `deltas` and the TC state."""
        lam = check_lam(lam)
        if backed and self.backed is None:
            raise ValueError("no roll-out with backed values has run: the agent holds no backed")
        o = self._moves(_native.TfeNtLearnBacked())
        o.lam = lam
        if backed or lam > 0.0:
            o.deltas = self._per_move("deltas").data_ptr()
        if backed:
            o.backed = self.backed.data_ptr()
        if tc:
            self._tc_state()
            o.acc_abs = self.acc_abs.data_ptr()
        return self._launch("pulse_tfe_nt_learn_staged", o, C.byref(self._stages()))

    def _apply_staged(self):
        """pulse_tfe_nt_apply, or with tc pulse_tfe_nt_apply_tc, once per stage on that stage's slice of weights, acc, acc_abs, E and A."""
        for s in range(self.n_stages):
            self._launch(*self._apply_struct(s, self.tc))
        return self

    def _apply_struct(self, stage, tc):
        """(entry point, its struct): pulse_tfe_nt_apply, or with tc pulse_tfe_nt_apply_tc, on stage `stage`'s slices."""
        at = stage * self.n_weights
        o = _native.TfeNtApplyTc() if tc else _native.TfeNtApply()
        self._net(o.net)
        o.net.weights = self.weights_dev[at:].data_ptr()
        o.step, o.acc = self.alpha / self.n_features, self.acc[at:].data_ptr()
        if tc:
            o.acc_abs, o.e, o.a, o.tc_stats = self.acc_abs[at:].data_ptr(), self.E[at:].data_ptr(), self.A[at:].data_ptr(), self.tc_stats.data_ptr()
        return "pulse_tfe_nt_apply_tc" if tc else "pulse_tfe_nt_apply", o

    # ------------------------------------------------------------------ the launches
    def _net(self, net):
        net.n, net.n_tuples, net.symmetric = self.n, len(self.tuples), int(self.symmetric)
        for t, cells in enumerate(self.tuples):
            net.tuple_len[t] = len(cells)
            for i, c in enumerate(cells):
                net.cells[t][i] = c
        net.n_weights, net.weights = self.n_weights, self.weights_dev.data_ptr()

    def _rollout_struct(self):
        o = self._draws(_native.TfeNtRollout(), self.round_board_id0())
        self._net(o.net)
        o.n_games, o.max_steps, o.gamma, o.epsilon = self.n_games, self.max_steps, self.gamma, self.epsilon
        o.keys, o.values, o.steps, o.lengths = self.keys.data_ptr(), self.values.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr()
        o.total_score, o.episode_reward, o.stats = self.total_score.data_ptr(), self.episode_reward.data_ptr(), self.counters.data_ptr()
        return o

    def rollout(self, layers=None):
        """One launch: n_games games under the weights as they stand (round `self.round`), into keys / values / steps / lengths /
        scores.  layers (None: the agent's `rollout_layers`) = 0: pulse_tfe_nt_rollout, greedy on reward + gamma * V; 1 or 2:
        rollout_search_launch, greedy on the q of the search that deep.  ValueError for any other.  With `backed_targets` the depth
        must be 1 or 2 (ValueError otherwise, before anything is touched) and the launch is rollout_backed_launch.  With
        `restart_fraction` > 0 the depth must be 0 or 1 (ValueError otherwise, before anything is touched), and once a pick has filled
        `start` the launch is rollout_from_launch at that depth, with the backed values if `backed_targets`.  With `stage_tiles` the
        depth must be 0 or 1 and the launch is rollout_staged_launch, from `start` (zeroed here while restart_fraction is 0 and
        `continue_games` is off).  With `continue_games` the depth must be 0 or 1, restart_fraction 0 and max_steps at least 2
        (ValueError otherwise, before anything is touched), and once a continue pick has filled `start` the launch is
        rollout_from_launch at that depth, with the backed values if `backed_targets`."""
        layers = check_rollout_layers(self.rollout_layers if layers is None else layers)
        restart = check_restart_fraction(self.restart_fraction) > 0.0
        if self.continue_games:
            if restart:
                raise ValueError("continue_games does not go with restart_fraction > 0: both fill start for the next round")
            if layers == 2:
                raise ValueError("continue_games needs rollout_layers in (0, 1): the roll-out from start is not built two layers deep")
            if self.max_steps < 2:
                raise ValueError("continue_games needs max_steps >= 2: a segment of K moves gives K - 1 learnt ones")
            restart = True                                                  # from here on the launches are the restarted rounds': from `start`
        self._refuse_two_layers(layers, "rollout_layers")
        if restart and layers == 2:
            raise ValueError("restart_fraction > 0 needs rollout_layers in (0, 1): the restarted roll-out is not built two layers deep")
        if self.backed_targets and not layers:
            raise ValueError("backed_targets needs rollout_layers in (1, 2): a one-ply roll-out has no search to back a value up")
        if self.stage_tiles:                                                # one entry point: from `start`, all zero while restarts are off
            self._restart_state()
            if not restart:
                self.start.zero_()
            return self.rollout_staged_launch(layers, backed=bool(self.backed_targets))
        if self.backed_targets:
            if restart and self.start is not None:
                return self.rollout_from_launch(layers, backed=True)
            return self.rollout_backed_launch(layers)
        if restart and self.start is not None:
            return self.rollout_from_launch(layers)
        if layers:
            return self.rollout_search_launch(layers)
        return self._launch("pulse_tfe_nt_rollout", self._rollout_struct())

    def _restart_state(self):
        """`start` and `restart_stats`, zeroed, where the agent has none yet."""
        import torch
        if self.start is None:
            self.start = torch.zeros(self.n_games, dtype=torch.int64, device=self.device)             # (uint64 words)
            self.restart_stats = torch.zeros(2, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ games continued across rounds
    def _continue_state(self):
        """`carry_score`, `carry_moves` and `finished`, zeroed, where the agent has none yet; `start` too (_restart_state)."""
        import torch
        self._restart_state()
        if self.carry_score is None:
            self.carry_score = torch.zeros(self.n_games, dtype=torch.int64, device=self.device)
            self.carry_moves = torch.zeros(self.n_games, dtype=torch.int32, device=self.device)
            self.finished = torch.zeros(len(FINISHED_SUMMARY) + EVAL_BINS, dtype=torch.int64, device=self.device)

    def continue_pick_launch(self):
        """pulse_tfe_nt_continue_pick alone on the games last recorded (under this round's seed and boards), whatever the agent's
        `continue_games`: per game cut at `max_steps`, `start` becomes the board its last move was made on and the carries take the
        segment without that move; every other game is added whole to `finished`, and its `start` and carries become 0.  ValueError
        if max_steps < 2."""
        if self.max_steps < 2:
            raise ValueError("continue_games needs max_steps >= 2: a segment of K moves gives K - 1 learnt ones")
        self._continue_state()
        o = _native.TfeNtContinuePick()
        o.n_games, o.max_steps, o.env_seed, o.board_id0 = self.n_games, self.max_steps, self.env_seed, self.round_board_id0()
        o.keys, o.steps, o.lengths, o.total_score = self.keys.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr(), self.total_score.data_ptr()
        o.start, o.carry_score, o.carry_moves, o.finished = self.start.data_ptr(), self.carry_score.data_ptr(), self.carry_moves.data_ptr(), self.finished.data_ptr()
        return self._launch("pulse_tfe_nt_continue_pick", o)

    def finished_summary(self, clear=True) -> dict:
        """finished_summary_on_host of `finished` (synchronises): the whole games that ended since the words were last zeroed, the
        games continued by the pick launches since and the finished games that had been continued.  clear: `finished` is zeroed."""
        if self.finished is None:
            raise ValueError("no continue launch has run: the agent holds no finished")
        out = finished_summary_on_host(self.finished.cpu().tolist())
        if clear:
            self.finished.zero_()
        return out

    def _per_move(self, name):
        """The agent's `deltas` or `backed` (`name`): float64 in the shape of `values`, allocated zeroed where the agent has none yet."""
        import torch
        if getattr(self, name) is None:
            setattr(self, name, torch.zeros_like(self.values))
        return getattr(self, name)

    def _from_args(self, layers, backed):
        """What rollout_from_launch and rollout_staged_launch check and pass beside the struct: (layers, `backed` or None, `start`),
        `start` and `backed` allocated where the agent has none."""
        if isinstance(layers, bool) or layers not in (0, 1):
            raise ValueError("layers must be 0 or 1")
        if backed and not layers:
            raise ValueError("backed needs layers = 1: a one-ply roll-out has no search to back a value up")
        self._restart_state()
        return int(layers), self._per_move("backed").data_ptr() if backed else None, self.start.data_ptr()

    def rollout_from_launch(self, layers, backed=False):
        """pulse_tfe_nt_rollout_from alone, whatever the agent's attributes: rollout()'s games at `layers` = 0 (one ply) or 1 (one-layer
        search; ValueError for any other), each begun on the board in `start` where that board is usable and at its reset otherwise
        (`start` is 0 there afterwards).  backed: rollout_backed_launch's `backed` too (layers must be 1).  A `start` no pick has
        filled is all zero: the launch plays its sibling's games."""
        args = self._from_args(layers, backed)
        return self._launch("pulse_tfe_nt_rollout_from", self._rollout_struct(), *args)

    def restart_pick_launch(self, fraction=None, min_length=None):
        """pulse_tfe_nt_restart_pick alone on the games last recorded (under this round's seed and boards): `start` becomes, per game
        of at least `min_length` moves, the board it stood on before move floor(L * fraction), and 0 for the others; `restart_stats`
        has the boards picked and their depths added.  fraction, min_length: None for the agent's attributes."""
        fraction = check_restart_fraction(self.restart_fraction if fraction is None else fraction)
        if not fraction > 0.0:
            raise ValueError("the pick needs a fraction in (0, 1): restart_fraction is 0 (off)")
        self._restart_state()
        o = _native.TfeNtRestartPick()
        o.n_games, o.max_steps, o.env_seed, o.board_id0 = self.n_games, self.max_steps, self.env_seed, self.round_board_id0()
        o.fraction, o.min_length = fraction, int(self.restart_min_length if min_length is None else min_length)
        o.keys, o.lengths, o.start, o.picked = self.keys.data_ptr(), self.lengths.data_ptr(), self.start.data_ptr(), self.restart_stats.data_ptr()
        return self._launch("pulse_tfe_nt_restart_pick", o)

    def restart_summary(self) -> dict:
        """{"picked", "mean_depth", "started"} (restart_summary_on_host; synchronises): the boards the pick launches since the last call
        picked and the mean of their t*, and the non-zero entries of `start` as it stands -- after a pick the games that will be
        restarted, after a roll-out those that were.  `restart_stats` is zeroed."""
        if self.start is None:
            raise ValueError("no restart launch has run: the agent holds no start")
        out = restart_summary_on_host(self.restart_stats.cpu().tolist(), self.start.cpu().numpy())
        self.restart_stats.zero_()
        return out

    def rollout_search_launch(self, layers):
        """pulse_tfe_nt_rollout_search alone, whatever the agent's `rollout_layers`: the roll-out's games, draws and records with the
        greedy action taken on the q of expectimax search `layers` chance layers deep (1 or 2; ValueError for any other).  `values`
        holds the network's V of the chosen afterstates, so the learners read the records as they read rollout()'s."""
        layers = check_layers(layers)
        return self._launch("pulse_tfe_nt_rollout_search", self._rollout_struct(), layers)

    def rollout_backed_launch(self, layers):
        """pulse_tfe_nt_rollout_backed alone, whatever the agent's `rollout_layers` and `backed_targets`: rollout_search_launch's games
        and records, and in `backed` (allocated here if the agent has none) per move the largest q of the search over the moves that
        change the board."""
        layers = check_layers(layers)
        return self._launch("pulse_tfe_nt_rollout_backed", self._rollout_struct(), layers, self._per_move("backed").data_ptr())

    def _moves(self, o):
        """The network and the fields the two learners' structs share."""
        self._net(o.net)
        o.n_games, o.max_steps, o.gamma = self.n_games, self.max_steps, self.gamma
        o.keys, o.values, o.steps, o.lengths = self.keys.data_ptr(), self.values.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr()
        o.acc, o.stats = self.acc.data_ptr(), self.counters.data_ptr()
        return o

    def _tc_state(self):
        """The third accumulator, E, A and tc_stats, zeroed, where the agent has none yet."""
        import torch
        if self.acc_abs is None:
            self.acc_abs = torch.zeros(self.total_weights, dtype=torch.int64, device=self.device)
            self.E = torch.zeros(self.total_weights, dtype=torch.float64, device=self.device)
            self.A = torch.zeros(self.total_weights, dtype=torch.float64, device=self.device)
            self.tc_stats = torch.zeros(4, dtype=torch.int64, device=self.device)

    def learn(self):
        """The temporal differences of the games last played, into the accumulators: one launch, or with lam > 0
        learn_lambda_launch's two; with tc, learn_tc_launch's; with backed_targets, learn_backed_launch's; with stage_tiles,
        learn_staged_launch's under the same three."""
        if self.stage_tiles:
            return self.learn_staged_launch(self.lam, backed=bool(self.backed_targets), tc=self.tc)
        if self.backed_targets:
            return self.learn_backed_launch(self.lam)
        if self.tc:
            return self.learn_tc_launch(self.lam)
        if self.lam > 0.0:
            return self.learn_lambda_launch(self.lam)
        return self._launch("pulse_tfe_nt_learn", self._moves(_native.TfeNtLearn()))

    def learn_lambda_launch(self, lam):
        """pulse_tfe_nt_learn_lambda on the games last played, whatever the agent's own `lam`: the backward walk into `deltas`
        (allocated here if the agent has none) and the adds of the lambda-differences into the accumulators."""
        lam = check_lam(lam)
        o = self._moves(_native.TfeNtLearnLambda())
        o.lam, o.deltas = lam, self._per_move("deltas").data_ptr()
        return self._launch("pulse_tfe_nt_learn_lambda", o)

    def learn_tc_launch(self, lam):
        """pulse_tfe_nt_learn_tc on the games last played, whatever the agent's own `lam` and `tc`: the adds of learn() (lam == 0: one
        launch, no deltas) or of learn_lambda_launch (lam > 0: the walk into `deltas`, then the adds), with |d| into `acc_abs` as
        well.  Allocates the TC state, and for lam > 0 `deltas`, if the agent has none."""
        lam = check_lam(lam)
        self._tc_state()
        o = self._moves(_native.TfeNtLearnTc())
        o.lam, o.acc_abs = lam, self.acc_abs.data_ptr()
        if lam > 0.0:
            o.deltas = self._per_move("deltas").data_ptr()
        return self._launch("pulse_tfe_nt_learn_tc", o)

    def learn_backed_launch(self, lam):
        """pulse_tfe_nt_learn_backed on the games rollout_backed_launch last recorded, whatever the agent's own `lam` and
        `backed_targets`: the backward walk of backed[t + 1] - V_t into `deltas` (allocated here if the agent has none) and the adds
        of what it left -- with the agent's `tc` into `acc_abs` as well.  ValueError if no such roll-out has run."""
        lam = check_lam(lam)
        if self.backed is None:
            raise ValueError("no roll-out with backed values has run: the agent holds no backed")
        o = self._moves(_native.TfeNtLearnBacked())
        o.lam, o.deltas, o.backed = lam, self._per_move("deltas").data_ptr(), self.backed.data_ptr()
        if self.tc:
            self._tc_state()
            o.acc_abs = self.acc_abs.data_ptr()
        return self._launch("pulse_tfe_nt_learn_backed", o)

    def apply_tc_launch(self):
        """pulse_tfe_nt_apply_tc: every visited weight moves by (alpha / F) * rho of the mean of its adds, rho = |E| / A as they stood;
        E and A take the round's means, the three accumulator words are zero afterwards and tc_stats has the round added."""
        self._tc_state()
        return self._launch(*self._apply_struct(0, True))

    def apply(self):
        """One launch: every visited weight moves by alpha / F of the mean of its adds; the accumulators are zero afterwards.  With
        tc, apply_tc_launch.  With stage_tiles, either once per stage on that stage's slices."""
        if self.stage_tiles:
            return self._apply_staged()
        if self.tc:
            return self.apply_tc_launch()
        return self._launch(*self._apply_struct(0, False))

    def learn_batch(self):
        self.rollout()
        self.learn()
        self.apply()
        if self.continue_games:                                             # the cut games' boards for the next round, the ended games into `finished`
            self.continue_pick_launch()
        elif self.restart_fraction > 0.0:                                  # the next round's start boards, from this round's records
            self.restart_pick_launch()
        self.round += 1
        return self

    # ------------------------------------------------------------------ evaluation
    def _eval_struct(self):
        o = _native.TfeNtEval()
        self._net(o.net)
        o.gamma = self.gamma
        return o

    def _eval_launch(self, o):
        if self.stage_tiles:                                                # (_under_search has refused two layers)
            return self._launch("pulse_tfe_nt_evaluate_staged", o, C.byref(self._stages()), self._eval_layers)
        self._launch(self._eval_entry, o, *self._eval_args)

    # ------------------------------------------------------------------ expectimax search (DESIGN.md sections 13.1, 13.4 and 13.11)
    _eval_entry, _eval_args, _eval_layers = "pulse_tfe_nt_evaluate", (), 0     # the evaluation one ply deep; _under_search sets the three for one call
    depth_stats = None                                                     # int64[2] on the device, from the first adaptive evaluation: moves two layers deep, one layer deep

    def _check_depth(self, layers, deep_empty_max):
        """(layers, deep_empty_max) as ints (deep_empty_max: or None), or the ValueError of what the search refuses: a depth other than 1
        or 2, a threshold other than None or 0..16, a threshold without two layers, two layers on an agent with stage_tiles"""
        layers, deep_empty_max = check_layers(layers), check_deep_empty_max(deep_empty_max)
        if deep_empty_max is not None and layers != 2:
            raise ValueError("deep_empty_max needs layers = 2: it says where the two-layer search is used; layers = 1 searches no board deeper")
        self._refuse_two_layers(layers, "layers")
        return layers, deep_empty_max

    def _depth_words(self):
        import torch
        if self.depth_stats is None:
            self.depth_stats = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self.depth_stats

    def _under_search(self, layers, call, *args, deep_empty_max=None):
        """call(*args) with the evaluation's entry point set to the search's: at one layer pulse_tfe_nt_evaluate_search, at two
        pulse_tfe_nt_evaluate_search_deep with the depth beside the struct; with deep_empty_max (and two layers)
        pulse_tfe_nt_evaluate_search_adaptive with the threshold and the agent's `depth_stats` beside it."""
        layers, deep_empty_max = self._check_depth(layers, deep_empty_max)
        if layers == 1:
            self._eval_entry = "pulse_tfe_nt_evaluate_search"
        elif deep_empty_max is None:
            self._eval_entry, self._eval_args = "pulse_tfe_nt_evaluate_search_deep", (layers,)
        else:
            self._eval_entry, self._eval_args = "pulse_tfe_nt_evaluate_search_adaptive", (deep_empty_max, self._depth_words().data_ptr())
        self._eval_layers = int(layers)
        try:
            return call(*args)
        finally:
            self.__dict__.pop("_eval_entry", None)
            self.__dict__.pop("_eval_args", None)
            self.__dict__.pop("_eval_layers", None)

    def _search_struct(self, boards, q, action, candidates):
        o = _native.TfeNtSearch()
        self._net(o.net)
        o.n_boards, o.gamma, o.tie_seed, o.round = boards.numel(), self.gamma, self.tie_seed, self.round
        o.boards, o.q, o.action, o.candidates = boards.data_ptr(), q.data_ptr(), action.data_ptr(), candidates.data_ptr()
        return o

    def search_launch(self, boards, q, action, candidates, layers=1, deep_empty_max=None):
        """The launch of search() alone on device tensors: boards int64[N] (the keys' words), q float64[N, 4], action int8[N],
        candidates uint8[N].  layers = 1: pulse_tfe_nt_search; layers = 2: pulse_tfe_nt_search_deep (ValueError for any other); with
        layers = 2 and deep_empty_max = 0..16: pulse_tfe_nt_search_adaptive, two layers on the boards with at most that many empty
        cells and one layer on the others."""
        layers, deep_empty_max = self._check_depth(layers, deep_empty_max)
        o = self._search_struct(boards, q, action, candidates)
        if self.stage_tiles:
            return self._launch("pulse_tfe_nt_search_staged", o, C.byref(self._stages()))
        if layers == 1:
            return self._launch("pulse_tfe_nt_search", o)
        if deep_empty_max is not None:
            return self._launch("pulse_tfe_nt_search_adaptive", o, deep_empty_max)
        return self._launch("pulse_tfe_nt_search_deep", o, layers)

    def search(self, keys, layers=1, deep_empty_max=None) -> dict:
        """One launch and one read-back: q float64[N, 4] of the packed boards `keys` under `layers` chance layers of search (1 or 2), the
        greedy action int8[N] (-1: the board is over) and the candidates uint8[N] (bit a: move a changes the board); search_nt_on_host
        on the device, with deep_empty_max search_adaptive_nt_on_host."""
        import torch
        layers, deep_empty_max = self._check_depth(layers, deep_empty_max)
        keys = np.array(keys, dtype=_U64).reshape(-1)                       # (a copy: torch takes no read-only array)
        boards = torch.from_numpy(keys.view(np.int64)).to(self.device)
        q = torch.zeros((len(keys), 4), dtype=torch.float64, device=self.device)
        action, candidates = torch.zeros(len(keys), dtype=torch.int8, device=self.device), torch.zeros(len(keys), dtype=torch.uint8, device=self.device)
        self.search_launch(boards, q, action, candidates, layers, deep_empty_max)
        return dict(q=q.cpu().numpy(), action=action.cpu().numpy(), candidates=candidates.cpu().numpy())

    def evaluate_search_launch(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False, layers=1, deep_empty_max=None):
        """evaluate_launch() under the search policy of `layers` chance layers (1 or 2); with layers = 2 and deep_empty_max = 0..16 under
        the adaptive search, which also ADDS the moves at each depth to `depth_stats` (int64[2]: two layers, one layer)."""
        return self._under_search(layers, self.evaluate_launch, n_games, epsilon, board_id0, per_game, deep_empty_max=deep_empty_max)

    def evaluate_search(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False, layers=1, deep_empty_max=None) -> dict:
        """evaluate() under the search policy of `layers` chance layers (1 or 2): the same default boards, so the policies are paired on
        the spawns each game starts from.  With layers = 2 and deep_empty_max = 0..16 the search is two layers deep on the boards with at
        most that many empty cells and one layer deep on the others (section 13.11), and the dict also has moves_deep / moves_shallow."""
        layers, deep_empty_max = self._check_depth(layers, deep_empty_max)
        if deep_empty_max is not None:
            self._depth_words().zero_()
        out = self._under_search(layers, self.evaluate, n_games, epsilon, board_id0, per_game, deep_empty_max=deep_empty_max)
        if deep_empty_max is not None:
            out["moves_deep"], out["moves_shallow"] = self.depth_stats.cpu().tolist()
        return out

    # ------------------------------------------------------------------ read-back (the only syncs) and the checkpoint
    def weights(self) -> np.ndarray:
        """float32[n_weights] on the host; with stage_tiles float32[n_stages * n_weights], stage s at [s * n_weights, (s + 1) * n_weights)."""
        return self.weights_dev.cpu().numpy()

    def trajectory(self):
        """(keys uint64[T, B], values float64[T, B], steps uint8[T, B], lengths int32[B]) of the last batch, T = the longest game; rows
        at and beyond a game's length hold whatever the buffers held before."""
        T, lengths = self._played()
        return self.keys[:T].cpu().numpy().view(np.uint64), self.values[:T].cpu().numpy(), self.steps[:T].cpu().numpy(), lengths

    def trajectory_deltas(self) -> np.ndarray:
        """float64[T, B]: the lambda-differences of the last TD(lambda) learn launch, T = the longest game; rows at and beyond a game's
        length hold whatever `deltas` held before."""
        if self.deltas is None:
            raise ValueError("no TD(lambda) launch has run: the agent holds no deltas")
        T, _ = self._played()
        return self.deltas[:T].cpu().numpy()

    def trajectory_backed(self) -> np.ndarray:
        """float64[T, B]: the search's backed-up values of the last rollout_backed_launch, T = the longest game; rows at and beyond a
        game's length hold whatever `backed` held before."""
        if self.backed is None:
            raise ValueError("no roll-out with backed values has run: the agent holds no backed")
        T, _ = self._played()
        return self.backed[:T].cpu().numpy()

    def coherence(self):
        """(E, A), float64[n_weights] each, on the host."""
        if self.E is None:
            raise ValueError("no temporal-coherence launch has run: the agent holds no E and A")
        return self.E.cpu().numpy(), self.A.cpu().numpy()

    def tc_summary(self) -> dict:
        """{"moved", "mean_rho"} of the apply_tc launches since the last call (tc_summary_on_host; synchronises), and tc_stats zeroed."""
        if self.tc_stats is None:
            raise ValueError("no temporal-coherence launch has run: the agent holds no tc_stats")
        out = tc_summary_on_host(self.tc_stats.cpu().tolist())
        self.tc_stats.zero_()
        return out

    def save(self, path):
        """The non-zero weights and what a continued run needs as an .npz (write_checkpoint); with tc, E and A too.  `rollout_layers`,
        `backed_targets`, `restart_fraction`, `restart_min_length`, `continue_games` and `eval_max_steps` are not saved: they say how
        rounds are played, learnt and evaluated, not what the network is; nor are `start` and the carries of continued games."""
        write_checkpoint(path, self.weights(), self.tuples, symmetric=int(self.symmetric), gamma=self.gamma, epsilon=self.epsilon, alpha=self.alpha,
                         max_steps=self.max_steps, seed=self.seed, board_id0=self.board_id0, round=self.round, n_games=self.n_games, lam=self.lam,
                         tc=self.coherence() if self.tc else None, stage_tiles=self.stage_tiles)

    @classmethod
    def load(cls, path, device, n_games=None):
        """The agent save() wrote: weights, round, seeds, lam, tc and with it E and A restored.  With the saved n_games it continues the run the saved agent would
        have continued (another n_games plays other boards: round r starts at board_id0 + r * n_games).  `rollout_layers` is 0, whatever the saved
        agent played under, `backed_targets` False, `restart_fraction` 0.0 and `continue_games` False with no `start` and no carries:
        set them again to continue such rounds; a loaded agent's games begin at their resets."""
        import torch
        f = read_checkpoint(path)
        agent = cls(device, f["n_games"] if n_games is None else n_games, tuples=f["tuples"], symmetric=f["symmetric"], gamma=f["gamma"],
                    epsilon=f["epsilon"], alpha=f["alpha"], max_steps=f["max_steps"], seed=f["seed"], board_id0=f["board_id0"], lam=f["lam"], tc=f["tc"],
                    stage_tiles=f["stage_tiles"])
        agent.weights_dev.copy_(torch.from_numpy(weights_of_checkpoint(f)))
        if f["tc"]:
            E, A = coherence_of_checkpoint(f)
            agent.E.copy_(torch.from_numpy(E))
            agent.A.copy_(torch.from_numpy(A))
        agent.round = f["round"]
        return agent

    def clear(self):
        """The empty network, zeroed accumulators and counters, round 0."""
        self.weights_dev.zero_()
        self.acc.zero_()
        self.counters.zero_()
        for t in (self.acc_abs, self.E, self.A, self.tc_stats, self.start, self.restart_stats, self.carry_score, self.carry_moves, self.finished):
            if t is not None:
                t.zero_()
        self.round = 0
        return self
