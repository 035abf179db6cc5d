"""On-policy first-visit Monte-Carlo control for 2048 on the device (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71 on the games of
scripts/TFE/mctrain.py): two launches per batch of games and nothing read back in between.

`pulse_tfe_mc_rollout` (csrc/tfe_mc.hip) plays `n_games` whole games, one lane each, against the policy of a hash table of
states in HBM and records one key and one byte per move; `pulse_tfe_mc_learn` walks the games backwards and adds the first-visit
returns into that table as fixed-point integers.  The table holds per (state, action) the count and the sum of those returns:
q(s, a) = sum / count * 2^-frac_bits, 0.0 where nothing was seen (the reference's defaultdict(float)).

Against the reference: the policy improves once per BATCH of games, not after every game; the coin that
breaks a tie between equal q is drawn per (state, round), not per look; actions and spawns come from Philox streams; a game is cut
at `max_steps` moves.  Round r plays the boards board_id0 + r * n_games + g, so no two rounds replay the same spawns.

`symmetric=True` keeps a board's eight images under the symmetries of the square as one state:
`pulse_tfe_mc_rollout_canon` looks up the smallest of the eight keys, takes the greedy action in that image's frame and moves the
board by the action mapped back; the learner is the same.  `evaluate()` (`pulse_tfe_mc_evaluate`) plays games under the table without
recording them and returns score statistics reduced in the launch.

`learn_on_host`, `greedy_on_host`, `first_visit_flags_on_host` and `run_mask_flags_on_host` are the host's statement of the same
arithmetic, in numpy and pure Python; `transforms_on_host`, `canon_on_host`, `ACTION_MAP` and `fold_table_on_host` that of the symmetries.
What the n-tuple agent shares with this one (Philox, the state key, the greedy scan, the evaluation counters, the agents' base class)
is in tfe_common.py and re-exported here.

The table as a whole goes through one more launch, `pulse_tfe_mc_table_merge`: dst += src over entries by key.
`merge_from` adds another agent's table (folding a plain one into a symmetric one), `grow` re-inserts the table into a larger one,
`to_symmetric` folds it, `save` / `load` write and read an .npz of the live rows; `merge_tables_on_host` is the host's statement.

`afterstate=True` learns V(afterstate) instead of Q(state, action): the key is the board after the move and
before the spawn, cnt[0] / sum[0] of its entry hold the returns that followed it, and the policy takes the largest
reward + gamma * v among the board's four afterstates (`pulse_tfe_mc_rollout_after`, `_after_canon`, `pulse_tfe_mc_learn_after`,
`pulse_tfe_mc_evaluate_after`, `pulse_tfe_mc_table_fold_after`).  `move_on_host`, `afterstates_on_host`, `greedy_after_on_host`,
`learn_after_on_host` and `fold_values_on_host` are the host's statement of it."""
from __future__ import annotations

import functools
import math

import numpy as np

from .. import _native
from .tfe_common import (AGENT_KEY, EVAL_BINS, TIE_KEY, _TFEGamesGPU, greedy_scan_on_host, pack_board, philox4x32,  # noqa: F401 (re-exported)
                         reward_of_score, transforms_on_host, unpack_key, unpack_steps)
from .tfe_common import eval_summary_on_host as _eval_summary_on_host

ENTRY_BYTES, MAX_PROBE, R_MAX = _native.TFE_MC_ENTRY_BYTES, _native.TFE_MC_MAX_PROBE, _native.TFE_MC_R_MAX
STATS = ("steps", "first_visits", "dropped", "truncated")
EVAL_SUMMARY = ("games", "moves", "score_sum", "score_sq_sum", "max_score", "truncated", "moves_with_entry", "moves_greedy")
MERGE_STATS = ("live", "placed", "dropped")     # pulse_tfe_mc_table_merge's counters


def frac_bits_for(gamma: float, max_steps: int) -> int:
    """The largest frac_bits <= 30 with G_max * 2^frac_bits * 2^32 < 2^62, G_max = 17 * min(max_steps, 1 / (1 - gamma)): room for 2^32
    adds per cell.  (The library's own rule: pulse_tfe_mc_* refuse anything above it.)"""
    horizon = 1.0 / (1.0 - gamma) if gamma < 1.0 else math.inf
    g_max = float(R_MAX) * min(float(max_steps), horizon)
    for f in range(30, -1, -1):
        if math.ldexp(g_max, f) < 2.0 ** 30:
            return f
    raise ValueError("no frac_bits fits")


# The eight symmetries of the square.  T_0..T_3 rotate the board 0..3 times by the environment's own
# rotation (TFE.py:38-44: out[r][c] = in[c][n - 1 - r]); T_4..T_7 do the same to the transposed board.  ACTION_MAP[j][a] is the
# action with T_j(move(B, a)) == move(T_j(B), ACTION_MAP[j][a]): the moves are 0 left, 1 up, 2 right, 3 down, a rotation turns
# them by one, the transpose swaps left with up and right with down.  (tests/test_tfe_mc_sym_cpu.py establishes the table against
# the environment's move; the device holds the same 32 numbers, two bits each, in one 64-bit constant.)
ACTION_MAP = ((0, 1, 2, 3), (3, 0, 1, 2), (2, 3, 0, 1), (1, 2, 3, 0), (1, 0, 3, 2), (0, 3, 2, 1), (3, 2, 1, 0), (2, 1, 0, 3))
ACTION_UNMAP = tuple(tuple(row.index(a) for a in range(4)) for row in ACTION_MAP)      # ACTION_UNMAP[j][ACTION_MAP[j][a]] == a


def canon_key_on_host(key: int, n: int):
    """(key_c, j*) of a state key: the smallest of the keys of its eight images and the smallest j whose image has it."""
    cells = unpack_key(key, n)
    images = [sum(cells[s] << (4 * i) for i, s in enumerate(src)) for src in transforms_on_host(n).tolist()]
    key_c = min(images)
    return key_c, images.index(key_c)


def canon_on_host(board):
    """(key_c, j*) of an n x n board of tiles."""
    board = np.asarray(board)
    return canon_key_on_host(pack_board(board), board.shape[-1])


def merge_tables_on_host(dst: dict, src: dict, n=None, canonical=False, keep_slots=False) -> dict:
    """pulse_tfe_mc_table_merge on the host: dst += src over entries, in place and returned.  Every entry of `src` goes to its key -- with
    `canonical` to its canonical key, cnt / sum permuted by ACTION_MAP[j*] (n: the board side the keys were packed for) -- and is added
    to what `dst` holds there; `dst`'s own keys stay as they are.  `src` is not changed.  `keep_slots`: cnt / sum stay in the slots
    they have (pulse_tfe_mc_table_fold_after: a value has no action to map)."""
    if canonical and n is None:
        raise ValueError("canonical=True needs the board side n")
    for key, (cnt, total) in src.items():
        key_c, j = canon_key_on_host(key, n) if canonical else (int(key), 0)
        c, s = dst.setdefault(key_c, ([0] * 4, [0] * 4))
        amap = ACTION_MAP[0 if keep_slots else j]
        for a in range(4):
            c[amap[a]] += int(cnt[a])
            s[amap[a]] += int(total[a])
    return dst


def fold_table_on_host(table: dict, n: int) -> dict:
    """A plain table {key: (cnt[4], sum[4])} as the table of canonical states: every entry goes to its canonical key with cnt / sum
    permuted by ACTION_MAP[j*], and entries that meet are added.  (n: the board side the keys were packed for.)"""
    return merge_tables_on_host({}, table, n, canonical=True)


def fold_values_on_host(table: dict, n: int) -> dict:
    """A plain VALUE table {key: (cnt[4], sum[4])} as the table of canonical afterstates: every entry goes to its canonical key with
    cnt / sum in the slots they have (a value has no action to map), and entries that meet are added."""
    return merge_tables_on_host({}, table, n, canonical=True, keep_slots=True)


# ------------------------------------------------------------------ the checkpoint file (save / load)
CHECKPOINT_VERSION = 1
CHECKPOINT_SCALARS = ("n", "gamma", "epsilon", "frac_bits", "max_steps", "seed", "board_id0", "round", "symmetric", "n_games")
CHECKPOINT_OPTIONAL = ("afterstate",)           # written by save(); a file without it holds a Q(state, action) table
_CHECKPOINT_DTYPES = dict(gamma=np.float64, epsilon=np.float64, seed=np.uint64, board_id0=np.uint64)         # the others: int64


def write_checkpoint(path, keys, cnt, total, **scalars) -> None:
    """The table as an .npz of plain arrays (np.savez, no pickles): keys uint64[m] sorted ascending, cnt int64[m, 4], sum int64[m, 4],
    the scalars of CHECKPOINT_SCALARS as 0-d arrays and `version`.  Rows are sorted here, so equal tables give equal arrays whatever
    slots their entries had.  `path` is written as given (no suffix is appended).  `afterstate=` (optional, 0 or 1) is written as one
    more scalar: the kind of the table."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    cnt, total = np.asarray(cnt, dtype=np.int64).reshape(-1, 4), np.asarray(total, dtype=np.int64).reshape(-1, 4)
    if not len(keys) == len(cnt) == len(total):
        raise ValueError("keys, cnt and sum must have one row per entry")
    if sorted(k for k in scalars if k not in CHECKPOINT_OPTIONAL) != sorted(CHECKPOINT_SCALARS):
        raise ValueError(f"a checkpoint holds exactly the scalars {CHECKPOINT_SCALARS}")
    order = np.argsort(keys, kind="stable")
    arrays = {k: np.array(scalars[k], dtype=_CHECKPOINT_DTYPES.get(k, np.int64)) for k in CHECKPOINT_SCALARS + CHECKPOINT_OPTIONAL if k in scalars}
    with open(path, "wb") as fh:
        np.savez(fh, version=np.array(CHECKPOINT_VERSION, dtype=np.int64), keys=keys[order], cnt=cnt[order], sum=total[order], **arrays)


def read_checkpoint(path, n=None) -> dict:
    """What write_checkpoint wrote (np.load with allow_pickle=False): the three arrays and the scalars as Python numbers.  ValueError
    for another format version, a missing or misshapen array, keys that are not strictly ascending from above 0 or do not fit n * n
    cells, and, where `n` is given, a file of another board side.  `afterstate` is False for a file without that scalar."""
    with np.load(path, allow_pickle=False) as f:
        missing = [k for k in ("version", "keys", "cnt", "sum") + CHECKPOINT_SCALARS if k not in f.files]
        if missing:
            raise ValueError(f"{path}: not a 2048 Monte-Carlo checkpoint (no {missing})")
        if int(f["version"]) != CHECKPOINT_VERSION:
            raise ValueError(f"{path}: format version {int(f['version'])}, this package reads {CHECKPOINT_VERSION}")
        out = {k: f[k] for k in ("keys", "cnt", "sum")}
        for k in CHECKPOINT_SCALARS:
            if f[k].shape != ():
                raise ValueError(f"{path}: {k} is not a scalar")
            out[k] = float(f[k]) if k in ("gamma", "epsilon") else int(f[k])
        out["afterstate"] = "afterstate" in f.files and bool(int(f["afterstate"]))
    out["symmetric"] = bool(out["symmetric"])
    keys, m = out["keys"], len(out["keys"])
    if keys.dtype != np.uint64 or keys.ndim != 1 or any(out[k].dtype != np.int64 or out[k].shape != (m, 4) for k in ("cnt", "sum")):
        raise ValueError(f"{path}: keys must be uint64[m], cnt and sum int64[m, 4]")
    if not 2 <= out["n"] <= 4 or (n is not None and out["n"] != int(n)):
        raise ValueError(f"{path}: board side {out['n']}" + (f", expected {int(n)}" if n is not None else " outside 2..4"))
    if m and (int(keys[0]) == 0 or not bool((keys[1:] > keys[:-1]).all()) or int(keys[-1]) >> (4 * out["n"] ** 2)):
        raise ValueError(f"{path}: keys must be strictly ascending, non-zero and fit the {out['n']} x {out['n']} cells")
    return out


def first_visit_flags_on_host(keys, actions) -> np.ndarray:
    """One game: True where (state, action) occurs for the first time -- the dict rule of OnPolicyFirstVisit.py:30-36."""
    seen, out = set(), []
    for pair in zip(np.asarray(keys).tolist(), np.asarray(actions).tolist()):
        out.append(pair not in seen)
        seen.add(pair)
    return np.array(out, dtype=bool)


def run_mask_flags_on_host(keys, actions) -> np.ndarray:
    """One game, the roll-out kernel's rule: True where the action was not yet taken in the current run of identical boards."""
    out, prev, taken = [], None, 0
    for key, a in zip(np.asarray(keys).tolist(), np.asarray(actions).tolist()):
        if key != prev:
            prev, taken = key, 0
        out.append(not (taken >> a) & 1)
        taken |= 1 << a
    return np.array(out, dtype=bool)


def q_of_entry(entry, frac_bits: int):
    cnt, total = entry
    return [float(int(total[a])) / float(int(cnt[a])) * 2.0 ** -frac_bits if cnt[a] > 0 else 0.0 for a in range(4)]


def greedy_on_host(entry, key: int, tie_seed: int, round: int, philox=philox4x32) -> int:
    """The greedy action of a table entry (cnt[4], sum[4]) as the roll-out takes it (OnPolicyFirstVisit.py:52-62): the actions in
    order, a larger q replaces the best, an equal q replaces it iff bit 31 of word a - 1 of philox(tie_seed, key, round) is set.
    (The factor 2^-frac_bits is exact and the same for the four q: it does not enter a comparison.)"""
    return greedy_scan_on_host(q_of_entry(entry, 0), lambda: philox(tie_seed, key, round))


def _learn_on_host(keys, steps, lengths, gamma: float, frac_bits: int, table: dict, after: bool) -> dict:
    """The backward pass of both learners: per game t = length - 1 .. 0, G = gamma * G + reward in float64, one rounding per
    operation; a flagged step adds round-half-even(G * 2^frac_bits) to sum[a] and 1 to cnt[a] of its key.  Without `after` a is the
    step's action and G includes the step's reward; with it a = 0 and G is taken BEFORE the step's reward enters."""
    keys, steps = np.asarray(keys, dtype=np.uint64), np.asarray(steps, dtype=np.uint8)
    if keys.ndim == 1:
        keys, steps = keys[:, None], steps[:, None]
    for g, length in enumerate(np.asarray(lengths).reshape(-1).tolist()):
        tail = 0.0
        for t in range(int(length) - 1, -1, -1):
            s = int(steps[t, g])
            if not after:
                tail = gamma * tail + float((s >> 2) & 31)
            if s & 0x80:
                a = 0 if after else s & 3
                cnt, total = table.setdefault(int(keys[t, g]), ([0] * 4, [0] * 4))
                total[a] += round(math.ldexp(tail, frac_bits))
                cnt[a] += 1
            if after:
                tail = gamma * tail + float((s >> 2) & 31)
    return table


def learn_on_host(keys, steps, lengths, gamma: float, frac_bits: int, table: dict) -> dict:
    """pulse_tfe_mc_learn on the host.  keys uint64[T, B], steps uint8[T, B], lengths int[B]; table {key: (cnt[4], sum[4])} of Python
    ints, added to in place and returned.  Per game t = length - 1 .. 0, G = gamma * G + reward in float64; at a flagged step
    sum[a] += round-half-even(G * 2^frac_bits), cnt[a] += 1."""
    return _learn_on_host(keys, steps, lengths, gamma, frac_bits, table, False)


# ------------------------------------------------------------------ afterstates
@functools.lru_cache(maxsize=None)
def _transform_lists(n: int) -> tuple:
    return tuple(tuple(row) for row in transforms_on_host(n).tolist())


def move_cells_on_host(cells, n: int, a: int):
    """(cells, merge score) of move `a` WITHOUT the spawn on the n * n tiles of a board as a list (TFE.py:154-178): the board rotated
    `a` times, every row squashed to the left -- a tile merges with an equal neighbour once --, rotated back."""
    src = _transform_lists(n)[a]
    out, score = [0] * (n * n), 0
    for r in range(0, n * n, n):
        res, w, merged = [0] * n, 0, False
        for c in range(n):
            val = cells[src[r + c]]
            if val == 0:
                continue
            if res[w] == 0:
                res[w] = val
            elif res[w] == val and not merged:
                res[w], score, merged = 2 * val, score + 2 * val, True
            else:
                w, merged = w + 1, False
                res[w] = val
        for c in range(n):
            out[src[r + c]] = res[c]
    return out, score


def move_on_host(board, a):
    """(board, merge score) of move `a` without the spawn: int[n, n] in, a new int64[n, n] out (move_cells_on_host)."""
    board = np.asarray(board, dtype=np.int64)
    n = board.shape[-1]
    cells, score = move_cells_on_host(board.reshape(-1).tolist(), n, int(a))
    return np.array(cells, dtype=np.int64).reshape(n, n), score


def afterstates_on_host(board, symmetric=False):
    """(keys[4], rewards[4]) of the four moves of a board: the afterstate's key (its canonical key with `symmetric`) and the reward."""
    board = np.asarray(board)
    n, cells = board.shape[-1], board.reshape(-1).tolist()
    keys, rewards = [], []
    for a in range(4):
        after, score = move_cells_on_host(cells, n, a)
        logs = [min(v.bit_length() - 1, 15) if v > 0 else 0 for v in after]
        images = _transform_lists(n) if symmetric else _transform_lists(n)[:1]
        keys.append(min(sum(logs[s] << (4 * i) for i, s in enumerate(src)) for src in images))
        rewards.append(reward_of_score(score))
    return keys, rewards


def v_of_entry(entry, frac_bits: int) -> float:
    cnt, total = entry
    return float(int(total[0])) / float(int(cnt[0])) * 2.0 ** -frac_bits if cnt[0] > 0 else 0.0


def greedy_after_on_host(board, table: dict, gamma: float, frac_bits: int, tie_seed: int, round: int, symmetric=False, philox=philox4x32):
    """The afterstate roll-out's greedy rule on one board: (action or None, keys[4], rewards[4]).  q_a = r_a + gamma * v(key_a) in
    float64, 0.0 for a key without an entry; a = 0..3 in order, a larger q replaces the best, an equal q replaces it iff bit 31 of
    word a - 1 of philox(tie_seed, plain key of the board, round) is set.  None: none of the four keys has an entry."""
    keys, rewards = afterstates_on_host(board, symmetric)
    if not any(k in table for k in keys):
        return None, keys, rewards
    q = [float(r) + gamma * (v_of_entry(table[k], frac_bits) if k in table else 0.0) for k, r in zip(keys, rewards)]
    return greedy_scan_on_host(q, lambda: philox(tie_seed, pack_board(board), round)), keys, rewards


def learn_after_on_host(keys, steps, lengths, gamma: float, frac_bits: int, table: dict) -> dict:
    """pulse_tfe_mc_learn_after on the host, in learn_on_host's shapes.  Per game t = length - 1 .. 0: at a flagged step
    sum[0] += round-half-even(G * 2^frac_bits), cnt[0] += 1 with G as it stands, THEN G = gamma * G + reward -- an afterstate
    collects the return that follows it."""
    return _learn_on_host(keys, steps, lengths, gamma, frac_bits, table, True)


def eval_summary_on_host(words) -> dict:
    """pulse_tfe_mc_evaluate's 8 + 16 counters as a dict (tfe_common.eval_summary_on_host with this agent's EVAL_SUMMARY)."""
    return _eval_summary_on_host(words, EVAL_SUMMARY)


class OnPolicyFirstVisitMCTFEGPU(_TFEGamesGPU):
    """`learn_batch` = `rollout` + `learn` + `round += 1`, two launches and no synchronisation.  Everything that reads back
    (`table`, `q`, `greedy`, `stats`, `trajectory`, the per-game arrays' `.cpu()`) synchronises."""
    STATS, EVAL_SUMMARY = STATS, EVAL_SUMMARY

    def __init__(self, device, n_games, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 22, max_steps=1024, seed=0, board_id0=0,
                 symmetric=False, afterstate=False):
        import torch
        super().__init__(device, n_games, board_size, max_steps, gamma, epsilon, seed, board_id0)
        if not 2 <= int(board_size) <= 4:
            raise ValueError("board_size must be 2..4 (the state key holds 16 cells)")
        if int(capacity) < 1 or int(capacity) & (int(capacity) - 1):
            raise ValueError("capacity must be a power of two")
        self.capacity, self.symmetric = int(capacity), bool(symmetric)
        self.frac_bits = frac_bits_for(self.gamma, self.max_steps)
        self.afterstate = bool(afterstate)              # the table holds V(afterstate) in cnt[0] / sum[0]
        self.entries = self._new_table(self.capacity)
        self._merge = torch.zeros(4, dtype=torch.int64, device=self.device)                           # merge_from(): live, placed, dropped

    def _new_table(self, rows):
        """int64[rows, 16] on the device, zeroed and 128-byte aligned: a table of `rows` slots, or a dense array of entries."""
        import torch
        words = ENTRY_BYTES // 8
        storage = torch.zeros(rows * words + words, dtype=torch.int64, device=self.device)
        skip = (-storage.data_ptr() % ENTRY_BYTES) // 8
        return storage[skip:skip + rows * words].view(rows, words)

    # ------------------------------------------------------------------ the launches
    def _head(self, o):
        o.entries, o.capacity = self.entries.data_ptr(), self.capacity
        o.n_games, o.n, o.max_steps, o.frac_bits = self.n_games, self.n, self.max_steps, self.frac_bits
        o.gamma, o.epsilon = self.gamma, self.epsilon
        o.keys, o.steps, o.lengths, o.stats = self.keys.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr(), self.counters.data_ptr()
        return o

    def rollout(self):
        """One launch: n_games games under the table as it stands (round `self.round`), into keys / steps / lengths / scores.
        With `symmetric` the recorded keys and actions are those of the canonical frame (pulse_tfe_mc_rollout_canon).  With
        `afterstate` the keys are those of the boards after the moves and the actions the board's own (pulse_tfe_mc_rollout_after*)."""
        o = self._draws(self._head(_native.TfeMCRollout()), self.round_board_id0())
        o.total_score, o.episode_reward = self.total_score.data_ptr(), self.episode_reward.data_ptr()
        return self._launch("pulse_tfe_mc_rollout" + ("_after" if self.afterstate else "") + ("_canon" if self.symmetric else ""), o)

    def learn(self):
        """One launch: the first-visit returns of the games last played, into the table."""
        return self._launch("pulse_tfe_mc_learn_after" if self.afterstate else "pulse_tfe_mc_learn", self._head(_native.TfeMCLearn()))

    def learn_batch(self):
        self.rollout()
        self.learn()
        self.round += 1
        return self

    # ------------------------------------------------------------------ the table as a whole
    def _merge_launch(self, src, dst, canonical, stats):
        """pulse_tfe_mc_table_merge: dst += src over entries, both int64[rows, 16] device tensors; the three counters are added to `stats`.
        The fold of a value table (`afterstate` and canonical) is pulse_tfe_mc_table_fold_after: the slots stay where they are."""
        o = _native.TfeMCMerge()
        o.src, o.src_entries, o.dst, o.dst_capacity = src.data_ptr(), src.shape[0], dst.data_ptr(), dst.shape[0]
        o.n, o.canonical, o.stats = self.n, int(canonical), stats.data_ptr()
        self._launch("pulse_tfe_mc_table_fold_after" if self.afterstate and canonical else "pulse_tfe_mc_table_merge", o)

    def dense_entries(self, keys, cnt, total):
        """keys uint64[m], cnt / sum int64[m, 4] of the host as a dense array of entries on the device (int64[m, 16], 128-byte aligned):
        what merge_from takes and a checkpoint load uploads."""
        import torch
        rows = np.zeros((len(keys), ENTRY_BYTES // 8), dtype=np.int64)
        rows[:, 0] = np.asarray(keys, dtype=np.uint64).view(np.int64)
        rows[:, 1:5], rows[:, 5:9] = cnt, total
        dense = self._new_table(len(keys))
        dense.copy_(torch.from_numpy(rows))
        return dense

    def merge_from(self, other, canonical=None):
        """This table += `other`: another agent's table, or an int64[m, 16] device tensor of entries (a dense array or a table with holes;
        key 0 = skip).  One launch, no synchronisation; merge_stats() tells what it placed.  The two tables must share n, gamma and
        frac_bits (ValueError otherwise: the sums would be on different scales).  A plain agent's table into a symmetric one is folded
        on the way; a symmetric one into a plain one is refused.  For a tensor `canonical` says whether its keys are to be folded
        (default: no; only a symmetric agent may ask for it).  A Q(state, action) table and a table of afterstate values do not mix:
        an agent of the other kind is refused (a tensor is taken as entries of this agent's kind)."""
        import torch
        if other is self:
            raise ValueError("merge_from: an agent cannot be merged into itself (source and destination overlap)")
        if isinstance(other, OnPolicyFirstVisitMCTFEGPU):
            for name in ("n", "gamma", "frac_bits"):
                if getattr(other, name) != getattr(self, name):
                    raise ValueError(f"merge_from: {name} differs ({getattr(other, name)} against {getattr(self, name)})")
            if other.afterstate != self.afterstate:
                kinds = ("Q(state, action)", "afterstate values")
                raise ValueError(f"merge_from: the source holds {kinds[other.afterstate]}, this table {kinds[self.afterstate]}")
            if other.symmetric and not self.symmetric:
                raise ValueError("merge_from: a table of canonical states cannot be merged into a plain one")
            if canonical is not None:
                raise ValueError("merge_from: `canonical` is for a tensor of entries; between agents it follows from `symmetric`")
            src, canonical = other.entries, self.symmetric and not other.symmetric
        else:
            src, canonical = other, bool(canonical)
            if not (isinstance(src, torch.Tensor) and src.dtype == torch.int64 and src.dim() == 2 and src.shape[1] == ENTRY_BYTES // 8
                    and src.shape[0] >= 1 and src.is_contiguous()):
                raise ValueError("merge_from takes an agent or a contiguous int64[m, 16] tensor of entries, m >= 1")
            if canonical and not self.symmetric:
                raise ValueError("merge_from: canonical=True needs a symmetric destination")
        if src.device != self.entries.device:
            raise ValueError(f"merge_from: the source is on {src.device}, the table on {self.entries.device}")
        self._merge_launch(src, self.entries, canonical, self._merge)
        return self

    def merge_stats(self, clear=False) -> dict:
        """What the merge_from launches since the last clear added up to: live source entries, entries placed, entries dropped for want
        of room (nothing of a dropped entry is added).  Synchronises; with clear the counters are zeroed afterwards."""
        out = dict(zip(MERGE_STATS, self._merge.cpu().tolist()[:3]))
        if clear:
            self._merge.zero_()
        return out

    def occupancy(self) -> int:
        """The number of live slots (synchronises)."""
        return int((self.entries[:, 0] != 0).sum().item())

    def grow(self, capacity):
        """The same map in a new zeroed table of `capacity` slots (a power of two; smaller is allowed): one merge launch and one read-back.
        If an entry finds no room there, RuntimeError, and the agent keeps the table it had.  Round, seeds, trajectory buffers and
        counters are untouched; the roll-out reads the table only by key, so the games to come are those of an agent that had
        this capacity from the start."""
        import torch
        capacity = int(capacity)
        if capacity < 1 or capacity & (capacity - 1):
            raise ValueError("capacity must be a power of two")
        table, stats = self._new_table(capacity), torch.zeros(4, dtype=torch.int64, device=self.device)
        self._merge_launch(self.entries, table, False, stats)
        live, placed, dropped = stats.cpu().tolist()[:3]
        if dropped or placed != live:
            raise RuntimeError(f"grow({capacity}): {dropped} of {live} entries found no room; the table of {self.capacity} slots is kept")
        self.entries, self.capacity = table, capacity
        return self

    def _like(self, n_games=None, capacity=None, symmetric=None):
        return type(self)(self.device, self.n_games if n_games is None else n_games, board_size=self.n, gamma=self.gamma, epsilon=self.epsilon,
                          capacity=self.capacity if capacity is None else capacity, max_steps=self.max_steps, seed=self.seed,
                          board_id0=self.board_id0, symmetric=self.symmetric if symmetric is None else symmetric, afterstate=self.afterstate)

    def to_symmetric(self, capacity=None):
        """A new agent with symmetric=True that holds the fold of this plain table (fold_table_on_host, with `afterstate`
        fold_values_on_host, as one launch), with this agent's
        seeds, round and shapes; `capacity` defaults to this one's.  RuntimeError if an entry found no room."""
        if self.symmetric:
            raise ValueError("to_symmetric: the table already holds canonical states")
        out = self._like(capacity=capacity, symmetric=True)
        out.round = self.round
        st = out.merge_from(self).merge_stats()
        if st["dropped"]:
            raise RuntimeError(f"to_symmetric: {st['dropped']} of {st['live']} entries found no room in {out.capacity} slots")
        return out

    def save(self, path):
        """The table and what a continued run needs as an .npz (write_checkpoint).  The live rows are compacted on the device; only
        they cross to the host."""
        e = self.entries
        rows = e[e[:, 0] != 0].cpu().numpy()
        write_checkpoint(path, np.ascontiguousarray(rows[:, 0]).view(np.uint64), rows[:, 1:5], rows[:, 5:9], n=self.n, gamma=self.gamma,
                         epsilon=self.epsilon, frac_bits=self.frac_bits, max_steps=self.max_steps, seed=self.seed, board_id0=self.board_id0,
                         round=self.round, symmetric=int(self.symmetric), n_games=self.n_games, afterstate=int(self.afterstate))

    @classmethod
    def load(cls, path, device, capacity=None, n_games=None, afterstate=None):
        """The agent save() wrote, of the kind it had (a file without an `afterstate` scalar holds a Q table; `afterstate`, where
        given, is the kind the caller expects: ValueError for a file of the other kind): the rows are uploaded as a dense array of entries and merged into a zeroed table of `capacity` slots
        (default: the smallest power of two >= 4 m and >= 2^12), round and seeds restored.  With the saved n_games it continues the
        run the saved agent would have continued (another n_games plays other boards: round r starts at board_id0 + r * n_games)."""
        f = read_checkpoint(path)
        if afterstate is not None and bool(afterstate) != f["afterstate"]:
            kinds = ("Q(state, action)", "afterstate values")
            raise ValueError(f"{path}: the checkpoint holds {kinds[f['afterstate']]}, not {kinds[bool(afterstate)]}")
        m = len(f["keys"])
        if capacity is None:
            capacity = max(1 << 12, 1 << max(4 * m - 1, 0).bit_length())
        agent = cls(device, f["n_games"] if n_games is None else n_games, board_size=f["n"], gamma=f["gamma"], epsilon=f["epsilon"],
                    capacity=capacity, max_steps=f["max_steps"], seed=f["seed"], board_id0=f["board_id0"], symmetric=f["symmetric"],
                    afterstate=f["afterstate"])
        if agent.frac_bits != f["frac_bits"]:
            raise ValueError(f"{path}: frac_bits {f['frac_bits']}, but gamma {f['gamma']} and max_steps {f['max_steps']} give {agent.frac_bits}")
        if m:
            st = agent.merge_from(agent.dense_entries(f["keys"], f["cnt"], f["sum"])).merge_stats()
            if st["dropped"] or st["placed"] != m:
                raise RuntimeError(f"{path}: {st['dropped']} of {m} entries found no room in {agent.capacity} slots")
        agent.round = f["round"]
        return agent

    # ------------------------------------------------------------------ read-back (the only syncs)
    def table(self) -> dict:
        """{key: (cnt[4], sum[4])} of Python ints for every stored state."""
        e = self.entries.cpu().numpy()
        rows = e[e[:, 0] != 0]
        return {int(k): (r[1:5].tolist(), r[5:9].tolist()) for k, r in zip(rows[:, 0].view(np.uint64).tolist(), rows)}

    def q(self) -> dict:
        """{(key, a): q} for the four actions of every stored state; a pair never seen reads 0.0.  ValueError on an afterstate agent."""
        if self.afterstate:
            raise ValueError("q(): this table holds afterstate values; read v()")
        return {(k, a): v for k, e in self.table().items() for a, v in enumerate(q_of_entry(e, self.frac_bits))}

    def v(self) -> dict:
        """{key: v} for every stored afterstate.  ValueError on a Q(state, action) agent."""
        if not self.afterstate:
            raise ValueError("v(): this table holds Q(state, action); read q()")
        return {k: v_of_entry(e, self.frac_bits) for k, e in self.table().items()}

    def greedy(self, keys, round=None) -> list:
        """The greedy action the roll-out of `round` takes in each of `keys` (the keys of boards as they lie), or None where the table
        has no entry.  With `symmetric` a key is looked up as its canonical state and the action comes back in the board's own frame.
        On an afterstate agent `keys` are BOARDS (n x n tiles): the rule needs their four moves (greedy_after_on_host); None where
        none of the four afterstates has an entry."""
        table, r = self.table(), self.round if round is None else int(round)
        if getattr(self, "afterstate", False):
            return [greedy_after_on_host(b, table, self.gamma, self.frac_bits, self.tie_seed, r, self.symmetric)[0] for b in keys]
        out = []
        for k in keys:
            k, j = canon_key_on_host(int(k), self.n) if self.symmetric else (int(k), 0)
            out.append(ACTION_UNMAP[j][greedy_on_host(table[k], k, self.tie_seed, r)] if k in table else None)
        return out

    # evaluate() (tfe_common.py): pulse_tfe_mc_evaluate, with `afterstate` pulse_tfe_mc_evaluate_after; a state without an entry still
    # plays the uniform default, and `coverage` is the share of moves whose state had an entry
    def _eval_struct(self):
        o = _native.TfeMCEval()
        o.entries, o.capacity, o.n, o.frac_bits, o.canonical = self.entries.data_ptr(), self.capacity, self.n, self.frac_bits, int(self.symmetric)
        return o

    def _eval_launch(self, o):
        if self.afterstate:
            self._launch("pulse_tfe_mc_evaluate_after", o, self.gamma)
        else:
            self._launch("pulse_tfe_mc_evaluate", o)

    def trajectory(self):
        """(keys uint64[T, B], steps uint8[T, B], lengths int32[B]) of the last batch, T = the longest game; rows at and beyond a
        game's length hold whatever the buffers held before."""
        T, lengths = self._played()
        return self.keys[:T].cpu().numpy().view(np.uint64), self.steps[:T].cpu().numpy(), lengths

    def episodes(self):
        """The last batch as the reference's episode lists [(state key, action, reward), ...], one per game."""
        keys, steps, lengths = self.trajectory()
        a, r, _ = unpack_steps(steps)
        return [[(int(keys[t, g]), int(a[t, g]), int(r[t, g])) for t in range(int(n))] for g, n in enumerate(lengths.tolist())]

    def clear(self):
        """An empty table, zeroed counters, round 0."""
        self.entries.zero_()
        self.counters.zero_()
        self._merge.zero_()
        self.round = 0
        return self
