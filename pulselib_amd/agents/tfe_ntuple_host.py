"""The 2048 n-tuple network on the host: numpy's statement of the arithmetic the device agent (tfe_ntuple_td_gpu.py) is held to word for
word, the checks of its options, and every constant.  No torch, no ctypes struct and no device is needed here.

The value of an afterstate -- the board after the move and before the spawn -- is the sum of a few lookup tables.
Each table is indexed by the tiles (4-bit log2, the state key's nibbles) on a fixed set of cells, read on the board's eight images under
the symmetries of the square, which share the table: `feature_cells_on_host`, `feature_indices_on_host`, `value_on_host`.  The policy of
a round is frozen and the learners' adds are fixed-point integers, so a round's result does not depend on scheduling, and the mirrors
below, vectorised over boards, state it exactly:
  the roll-out's greedy rule and the learner and apply launches (section 13): `greedy_nt_on_host`, `learn_nt_on_host`, `apply_nt_on_host`;
  expectimax search one and two chance layers deep (13.1, 13.4) and by the board's empty cells (13.11): `search_nt_on_host`,
    `search_adaptive_nt_on_host`;
  TD(lambda) (13.2): `lambda_deltas_on_host`, `learn_lambda_nt_on_host`;
  temporal-coherence step sizes (13.3): `learn_tc_nt_on_host`, `apply_tc_nt_on_host`;
  search-backed targets (13.6): `search_backed_on_host`, `backed_deltas_on_host`, `learn_backed_nt_on_host`;
  restarted roll-outs (13.7): `spawn_on_host`, `restart_pick_on_host`;
  weight sets by tile stage (13.9): the stages travel on `tuples` (`with_stages`), so every mirror reads and adds by stage;
    `stage_of_keys_on_host` states the stage, `split_stage_tiles` and `add_stage_on_host` the promotion;
  games continued across rounds (13.10): `continue_pick_on_host`;
  the roll-out at the adaptive depth (13.13): `search_adaptive_nt_on_host`'s q with `search_backed_on_host` of them; no mirror of its own;
  rank-parallel rounds (13.14): `pack_acc_on_host`, `unpack_acc_on_host`, `shard_round_board_id0`.
Which of a round's options go together is stated once, in `check_options` (13.12), in the agent's words and in the script's."""
from __future__ import annotations

import functools

import numpy as np

from .. import _native
from .tfe_common import EVAL_BINS, greedy_scan_many_on_host, philox_many_on_host, rewards_of_scores, transforms_on_host
from .tfe_common import eval_summary_on_host as _eval_summary_on_host

MAX_TUPLES, MAX_LEN, FRAC_BITS, DELTA_MAX = _native.TFE_NT_MAX_TUPLES, _native.TFE_NT_MAX_LEN, _native.TFE_NT_FRAC_BITS, _native.TFE_NT_DELTA_MAX
MAX_STAGES = _native.TFE_NT_MAX_STAGES
DEFAULT_TUPLES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))       # two rows and two 2 x 3 rectangles
STATS = ("moves", "learnt", "skipped", "truncated", "clamped")                                # words 0..4 of the stats buffer
EVAL_SUMMARY = ("games", "moves", "score_sum", "score_sq_sum", "max_score", "truncated", "moves_greedy", "tile_capped")
TC_RHO_BITS = 32                                                                              # rho is summed as llrint(rho * 2^32)
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


def split_stage_tiles(old_tiles, tile, whose="network"):
    """(the stage tiles with `tile` among them, the new stage): the stage that holds `tile` is split at it, and the new stage, the upper
    one, is split from stage new - 1.  ValueError if `tile` is no stage tile, a stage begins at it already or `whose` (the word of the
    message: the "network" or the "agent") has MAX_STAGES stages."""
    (tile,), old = check_stage_tiles((tile,)), tuple(old_tiles)
    if tile in old:
        raise ValueError(f"a stage begins at tile {tile} already")
    if len(old) + 1 >= MAX_STAGES:
        raise ValueError(f"the {whose} has {MAX_STAGES} stages already")
    tiles = tuple(sorted(old + (tile,)))
    return tiles, tiles.index(tile) + 1


def add_stage_on_host(arrays, tuples, tile, copy=True):
    """add_stage on the host: (the arrays grown by one stage, `tuples` carrying the stage tiles with `tile` among them).  Every array of
    `arrays` holds n_stages slices of equal length along its first axis; the stage that holds `tile` is split at it and the new, upper
    stage's slice is a copy of the slice it is split from (copy: the weights, E and A) or zero (the accumulators).  ValueError if a
    stage begins at `tile` already or MAX_STAGES stages exist."""
    old = stage_tiles_of(tuples)
    tiles, new = split_stage_tiles(old, tile)
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


def check_from_layers(layers, backed=False) -> int:
    """The depth of a roll-out from given boards (pulse_tfe_nt_rollout_from, pulse_tfe_nt_rollout_staged) as an int: 0 or 1, and 1 with
    `backed`, as the library checks its two arguments.  ValueError otherwise; a bool is no depth."""
    if isinstance(layers, bool) or layers not in (0, 1):
        raise ValueError("layers must be 0 or 1")
    if backed and not layers:
        raise ValueError("backed needs layers = 1: a one-ply roll-out has no search to back a value up")
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


# ------------------------------------------------------------------ which options go together
def check_options(depth=0, backed_targets=False, restart_fraction=0.0, continue_games=False, max_steps=None, staged=False, *,
                  search=False, layers=1, deep_empty_max=None, rollout_deep_empty_max=None, shard=None, script=False):
    """The one statement of which options of a round and of an evaluation go together.  Of the round: `depth`, the chance layers its
    games are played under (check_rollout_layers), `backed_targets`, `restart_fraction` (check_restart_fraction), `continue_games`,
    `max_steps` (None: not asked about) and `staged`, whether the network has weight sets by stage.  Of the evaluation or the search,
    where there is one (`search`): its `layers` (check_layers) and `deep_empty_max` (check_deep_empty_max).  Of the round again:
    `rollout_deep_empty_max` (check_deep_empty_max; None: off), the threshold of a roll-out at the adaptive depth (section 13.13), which
    is built from `start` too: with it two layers go with restarts and with continuation.  `shard` (section 13.14; None: one process
    plays the round): (n_games_total, game0, n_games), the job's games, the rank's first and how many it plays (check_shard).  A
    sharded round goes with every learner, `tc`, stages, restarts, continuation and the search roll-outs: the exchange sits between the
    learn and the apply launch and knows none of them, so the shard adds no row to the table.  ValueError at the first
    rule of the table below that is broken, in the agent's words (attributes and arguments) or, with `script`, in those of
    scripts/tfe_ntuple.py (flags).  Returns (depth, from_start, layers, deep_empty_max) as they are meant: from_start, the round's
    games begin on the boards of `start` (restarts or continuation); layers 0 without `search`.  A new option's rules are added here."""
    depth, restart = check_rollout_layers(depth), check_restart_fraction(restart_fraction) > 0.0
    layers, deep_empty_max = check_layers(layers) if search else 0, check_deep_empty_max(deep_empty_max)
    adaptive = check_deep_empty_max(rollout_deep_empty_max) is not None
    if shard is not None:
        check_shard(*shard)
    two_on_stages = "layers = 2 on an agent with stage_tiles: two chance layers are not built on stages"
    stages_two = "--stages / --add-stage do not go with two chance layers: the staged launches are one ply or one chance layer deep"
    rules = (                                                               # (broken, the agent's words, the script's), in the order they are tested
        (deep_empty_max is not None and layers != 2,
         "deep_empty_max needs layers = 2: it says where the two-layer search is used; layers = 1 searches no board deeper",
         "--deep-empty-max needs --search --layers 2: it says on which boards the evaluation's search looks two chance layers ahead"),
        (deep_empty_max is not None and staged, two_on_stages,
         "--deep-empty-max does not go with --stages / --add-stage: two chance layers are not built on stages"),
        (adaptive and depth != 2,
         "rollout_deep_empty_max needs rollout_layers = 2: it says on which boards the roll-out's search looks two chance layers ahead",
         "--train-deep-empty-max needs --train-layers 2: it says on which boards the roll-out's search looks two chance layers ahead"),
        (adaptive and staged, "rollout_deep_empty_max on an agent with stage_tiles: two chance layers are not built on stages",
         "--train-deep-empty-max does not go with --stages / --add-stage: two chance layers are not built on stages"),
        (continue_games and restart,
         "continue_games does not go with restart_fraction > 0: both fill start for the next round",
         "--continue-games does not go with --restart: both choose the boards the next round's games begin on"),
        (continue_games and depth == 2 and not adaptive,
         "continue_games needs rollout_layers in (0, 1): the roll-out from start is not built two layers deep",
         "--continue-games does not go with --train-layers 2: the roll-out from given boards is one ply or one chance layer deep"),
        (continue_games and max_steps is not None and max_steps < 2,
         "continue_games needs max_steps >= 2: a segment of K moves gives K - 1 learnt ones",
         "--continue-games needs --max-steps 2 or more: a segment of K moves gives K - 1 learnt ones"),
        (staged and depth == 2, "rollout_" + two_on_stages, stages_two),
        (staged and layers == 2, two_on_stages, stages_two),
        (restart and depth == 2 and not adaptive,
         "restart_fraction > 0 needs rollout_layers in (0, 1): the restarted roll-out is not built two layers deep",
         "--restart does not go with --train-layers 2: the restarted roll-out is one ply or one chance layer deep"),
        (backed_targets and not depth,
         "backed_targets needs rollout_layers in (1, 2): a one-ply roll-out has no search to back a value up",
         "--backed needs --train-layers 1 or 2: the backed-up values are the search's"))
    for broken, *words in rules:
        if broken:
            raise ValueError(words[bool(script)])
    return depth, restart or bool(continue_games), layers, deep_empty_max


# ------------------------------------------------------------------ rank-parallel rounds
ACC_LIST_HEADER, ACC_LIST_ENTRY = 4, 4                                                         # int64 words: {found, written, 0, 0}; {index, sum, cnt, abs}


def check_shard(n_games_total, game0, n_games) -> tuple:
    """A rank's share of a round as ints (n_games_total, game0, n_games): the games game0 .. game0 + n_games - 1 of the job's
    n_games_total.  ValueError unless 0 <= game0, 1 <= n_games and game0 + n_games <= n_games_total; a bool is no count."""
    if any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in (n_games_total, game0, n_games)):
        raise ValueError("a shard's n_games_total, game0 and n_games must be ints")
    n_games_total, game0, n_games = int(n_games_total), int(game0), int(n_games)
    if game0 < 0 or n_games < 1 or game0 + n_games > n_games_total:
        raise ValueError("a shard must lie inside the job's games: 0 <= game0, 1 <= n_games, game0 + n_games <= n_games_total")
    return n_games_total, game0, n_games


def shard_round_board_id0(board_id0, round, n_games_total, game0) -> int:
    """The id of the first board a rank plays in round `round`: board_id0 + round * n_games_total + game0.  The single process plays
    board_id0 + round * n_games_total + g for g < n_games_total, so the rank whose games begin at game0 plays exactly its games."""
    return int(board_id0) + int(round) * int(n_games_total) + int(game0)


def pack_acc_on_host(acc, acc_abs=None) -> np.ndarray:
    """pulse_tfe_nt_acc_pack's entries on the host, int64[k, 4] = {index, sum, cnt, abs} in ascending index order (the device's order
    is not defined: compare after sorting by index): one per cell with cnt > 0 -- cnt, not sum: a cell whose differences cancel is
    still a visit -- abs from acc_abs, 0 without one.  acc int64[W, 2], acc_abs int64[W] or None; neither is written."""
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, 2)
    at = np.flatnonzero(acc[:, 1] > 0)
    out = np.zeros((len(at), ACC_LIST_ENTRY), dtype=np.int64)
    out[:, 0], out[:, 1:3] = at, acc[at]
    if acc_abs is not None:
        out[:, 3] = np.asarray(acc_abs, dtype=np.int64).reshape(-1)[at]
    return out


def unpack_acc_on_host(acc, acc_abs, entries):
    """pulse_tfe_nt_acc_unpack's adds on the host, in place: for every entry {index, sum, cnt, abs} of int64[k, 4] with 0 <= index <
    len(acc) (the index read as unsigned: a negative one is outside) and cnt > 0, acc[index] += {sum, cnt} and, with acc_abs,
    acc_abs[index] += abs; any other entry adds nothing.  Entries may repeat an index.  Returns (added, refused)."""
    entries = np.asarray(entries, dtype=np.int64).reshape(-1, ACC_LIST_ENTRY)
    good = (entries[:, 0] >= 0) & (entries[:, 0] < len(acc)) & (entries[:, 2] > 0)
    e = entries[good]
    np.add.at(acc[:, 0], e[:, 0], e[:, 1])
    np.add.at(acc[:, 1], e[:, 0], e[:, 2])
    if acc_abs is not None:
        np.add.at(acc_abs, e[:, 0], e[:, 3])
    return int(good.sum()), int(len(entries) - good.sum())


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

