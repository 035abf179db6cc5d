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
arithmetic, in numpy and pure Python; `transforms_on_host`, `canon_on_host`, `ACTION_MAP` and `fold_table_on_host` that of the symmetries."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _native

ENTRY_BYTES, MAX_PROBE, R_MAX = _native.TFE_MC_ENTRY_BYTES, _native.TFE_MC_MAX_PROBE, _native.TFE_MC_R_MAX
AGENT_KEY = 0x2048AC7105EED                     # the agent's draws are keyed apart from the environment's (the seed itself) ...
TIE_KEY = 0x20487C01F11B5                       # ... and the tie coins apart from both
STATS = ("steps", "first_visits", "dropped", "truncated")
EVAL_SUMMARY = ("games", "moves", "score_sum", "score_sq_sum", "max_score", "truncated", "moves_with_entry", "moves_greedy")
EVAL_BINS = 16                                  # bin = log2 of the largest tile of the final board


def frac_bits_for(gamma: float, max_steps: int) -> int:
    """The largest frac_bits <= 30 with G_max * 2^frac_bits * 2^32 < 2^62, G_max = 17 * min(max_steps, 1 / (1 - gamma)): room for 2^32
    adds per cell.  (The library's own rule: pulse_tfe_mc_* refuse anything above it.)"""
    horizon = 1.0 / (1.0 - gamma) if gamma < 1.0 else math.inf
    g_max = float(R_MAX) * min(float(max_steps), horizon)
    for f in range(30, -1, -1):
        if math.ldexp(g_max, f) < 2.0 ** 30:
            return f
    raise ValueError("no frac_bits fits")


def philox4x32(seed: int, subseq: int, offset: int):
    """Philox4x32-10 with the device's layout (csrc/blackjack_device.h): counter {offset, subseq}, key = seed.  Four uint32 as ints."""
    c0, c1, c2, c3 = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF, subseq & 0xFFFFFFFF, (subseq >> 32) & 0xFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def pack_board(board) -> int:
    """The state key: 4 bits of log2(tile) per cell (0 = empty), row-major, cell 0 in the low nibble."""
    key = 0
    for i, v in enumerate(np.asarray(board).ravel().tolist()):
        key |= (min(int(v).bit_length() - 1, 15) if v > 0 else 0) << (4 * i)
    return key


def unpack_key(key: int, n: int) -> list:
    """The n * n log2 tiles of a state key, row-major."""
    return [(int(key) >> (4 * i)) & 15 for i in range(n * n)]


# The eight symmetries of the square.  T_0..T_3 rotate the board 0..3 times by the environment's own
# rotation (TFE.py:38-44: out[r][c] = in[c][n - 1 - r]); T_4..T_7 do the same to the transposed board.  ACTION_MAP[j][a] is the
# action with T_j(move(B, a)) == move(T_j(B), ACTION_MAP[j][a]): the moves are 0 left, 1 up, 2 right, 3 down, a rotation turns
# them by one, the transpose swaps left with up and right with down.  (tests/test_tfe_mc_sym_cpu.py establishes the table against
# the environment's move; the device holds the same 32 numbers, two bits each, in one 64-bit constant.)
ACTION_MAP = ((0, 1, 2, 3), (3, 0, 1, 2), (2, 3, 0, 1), (1, 2, 3, 0), (1, 0, 3, 2), (0, 3, 2, 1), (3, 2, 1, 0), (2, 1, 0, 3))
ACTION_UNMAP = tuple(tuple(row.index(a) for a in range(4)) for row in ACTION_MAP)      # ACTION_UNMAP[j][ACTION_MAP[j][a]] == a


def transforms_on_host(n: int) -> np.ndarray:
    """int64[8, n * n]: T_j(B).ravel() == B.ravel()[transforms_on_host(n)[j]]."""
    out = np.zeros((8, n * n), dtype=np.int64)
    for j in range(8):
        for r in range(n):
            for c in range(n):
                rr, cc = r, c
                for _ in range(j & 3):                                     # rot_src of csrc/tfe_device.h
                    rr, cc = cc, n - 1 - rr
                out[j, r * n + c] = cc * n + rr if j >= 4 else rr * n + cc
    return out


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


def fold_table_on_host(table: dict, n: int) -> dict:
    """A plain table {key: (cnt[4], sum[4])} as the table of canonical states: every entry goes to its canonical key with cnt / sum
    permuted by ACTION_MAP[j*], and entries that meet are added.  (n: the board side the keys were packed for.)"""
    out = {}
    for key, (cnt, total) in table.items():
        key_c, j = canon_key_on_host(key, n)
        c, s = out.setdefault(key_c, ([0] * 4, [0] * 4))
        for a in range(4):
            c[ACTION_MAP[j][a]] += int(cnt[a])
            s[ACTION_MAP[j][a]] += int(total[a])
    return out


def unpack_steps(steps):
    """(action, reward, first) of the per-move bytes."""
    s = np.asarray(steps, dtype=np.uint8)
    return s & 3, (s >> 2) & 31, (s >> 7).astype(bool)


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
    q = q_of_entry(entry, 0)
    coins = None
    best, best_q = 0, q[0]
    for a in (1, 2, 3):
        if q[a] > best_q:
            best, best_q = a, q[a]
        elif q[a] == best_q:
            if coins is None:
                coins = [int(w) for w in philox(tie_seed, key, round)]
            if coins[a - 1] >> 31:
                best = a
    return best


def learn_on_host(keys, steps, lengths, gamma: float, frac_bits: int, table: dict) -> dict:
    """pulse_tfe_mc_learn on the host.  keys uint64[T, B], steps uint8[T, B], lengths int[B]; table {key: (cnt[4], sum[4])} of Python
    ints, added to in place and returned.  Per game t = length - 1 .. 0, G = gamma * G + reward in float64; at a flagged step
    sum[a] += round-half-even(G * 2^frac_bits), cnt[a] += 1."""
    keys, steps = np.asarray(keys, dtype=np.uint64), np.asarray(steps, dtype=np.uint8)
    if keys.ndim == 1:
        keys, steps = keys[:, None], steps[:, None]
    for g, length in enumerate(np.asarray(lengths).reshape(-1).tolist()):
        tail = 0.0
        for t in range(int(length) - 1, -1, -1):
            s = int(steps[t, g])
            tail = gamma * tail + float((s >> 2) & 31)
            if s & 0x80:
                cnt, total = table.setdefault(int(keys[t, g]), ([0] * 4, [0] * 4))
                total[s & 3] += round(math.ldexp(tail, frac_bits))
                cnt[s & 3] += 1
    return table


def eval_summary_on_host(words) -> dict:
    """pulse_tfe_mc_evaluate's 8 + 16 counters as a dict: the words by name, the histogram, and mean / std (sample standard deviation,
    from the exact integer sums) / max of the final score, the mean length and the share of moves whose state had a table entry."""
    w = [int(x) for x in words]
    out = dict(zip(EVAL_SUMMARY, w[:len(EVAL_SUMMARY)]))
    n, s, ss = out["games"], out["score_sum"], out["score_sq_sum"]
    out["max_tile_hist"] = w[len(EVAL_SUMMARY):len(EVAL_SUMMARY) + EVAL_BINS]
    out["mean_score"] = s / n if n else 0.0
    out["std_score"] = math.sqrt((n * ss - s * s) / (n * (n - 1))) if n > 1 else 0.0          # exact integers under the root
    out["mean_length"] = out["moves"] / n if n else 0.0
    out["coverage"] = out["moves_with_entry"] / out["moves"] if out["moves"] else 0.0
    return out


class OnPolicyFirstVisitMCTFEGPU:
    """`learn_batch` = `rollout` + `learn` + `round += 1`, two launches and no synchronisation.  Everything that reads back
    (`table`, `q`, `greedy`, `stats`, `trajectory`, the per-game arrays' `.cpu()`) synchronises."""

    def __init__(self, device, n_games, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 22, max_steps=1024, seed=0, board_id0=0,
                 symmetric=False):
        import torch
        device = _native.gpu_device(device, "OnPolicyFirstVisitMCTFEGPU")
        if not 2 <= int(board_size) <= 4:
            raise ValueError("board_size must be 2..4 (the state key holds 16 cells)")
        if int(capacity) < 1 or int(capacity) & (int(capacity) - 1):
            raise ValueError("capacity must be a power of two")
        if int(n_games) < 1 or not 1 <= int(max_steps) <= 65535:
            raise ValueError("n_games must be positive and max_steps in 1..65535")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= epsilon <= 1.0):
            raise ValueError("gamma and epsilon must be in [0, 1]")
        self._lib = _native.lib()
        self.device = device
        self.n_games, self.n, self.capacity, self.max_steps = int(n_games), int(board_size), int(capacity), int(max_steps)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.frac_bits = frac_bits_for(self.gamma, self.max_steps)
        self.seed, self.board_id0, self.round, self.symmetric = int(seed), int(board_id0), 0, bool(symmetric)
        self.env_seed, self.agent_seed, self.tie_seed = self.seed, self.seed ^ AGENT_KEY, self.seed ^ TIE_KEY
        words = ENTRY_BYTES // 8
        self._storage = torch.zeros(self.capacity * words + words, dtype=torch.int64, device=device)
        skip = (-self._storage.data_ptr() % ENTRY_BYTES) // 8
        self.entries = self._storage[skip:skip + self.capacity * words].view(self.capacity, words)   # 128-byte aligned
        self.keys = torch.zeros((self.max_steps, self.n_games), dtype=torch.int64, device=device)    # (uint64 words)
        self.steps = torch.zeros((self.max_steps, self.n_games), dtype=torch.uint8, device=device)
        self.lengths = torch.zeros(self.n_games, dtype=torch.int32, device=device)
        self.total_score = torch.zeros(self.n_games, dtype=torch.int64, device=device)
        self.episode_reward = torch.zeros(self.n_games, dtype=torch.int32, device=device)
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)
        self._eval = torch.zeros(len(EVAL_SUMMARY) + EVAL_BINS, dtype=torch.int64, device=device)     # evaluate(): summary, then the histogram

    # ------------------------------------------------------------------ the launches
    def _head(self, o):
        o.entries, o.capacity = self.entries.data_ptr(), self.capacity
        o.n_games, o.n, o.max_steps, o.frac_bits = self.n_games, self.n, self.max_steps, self.frac_bits
        o.gamma, o.epsilon = self.gamma, self.epsilon
        o.keys, o.steps, o.lengths, o.stats = self.keys.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr(), self.counters.data_ptr()
        return o

    def round_board_id0(self, round=None) -> int:
        return self.board_id0 + (self.round if round is None else int(round)) * self.n_games

    def rollout(self):
        """One launch: n_games games under the table as it stands (round `self.round`), into keys / steps / lengths / scores.
        With `symmetric` the recorded keys and actions are those of the canonical frame (pulse_tfe_mc_rollout_canon)."""
        o = self._head(_native.TfeMCRollout())
        o.env_seed, o.agent_seed, o.tie_seed, o.board_id0, o.round = self.env_seed, self.agent_seed, self.tie_seed, self.round_board_id0(), self.round
        o.total_score, o.episode_reward = self.total_score.data_ptr(), self.episode_reward.data_ptr()
        name = "pulse_tfe_mc_rollout_canon" if self.symmetric else "pulse_tfe_mc_rollout"
        _native.check(getattr(self._lib, name)(C.byref(o), _native.current_stream(self.device)), name)
        return self

    def learn(self):
        """One launch: the first-visit returns of the games last played, into the table."""
        o = self._head(_native.TfeMCLearn())
        _native.check(self._lib.pulse_tfe_mc_learn(C.byref(o), _native.current_stream(self.device)), "pulse_tfe_mc_learn")
        return self

    def learn_batch(self):
        self.rollout()
        self.learn()
        self.round += 1
        return self

    # ------------------------------------------------------------------ read-back (the only syncs)
    def table(self) -> dict:
        """{key: (cnt[4], sum[4])} of Python ints for every stored state."""
        e = self.entries.cpu().numpy()
        rows = e[e[:, 0] != 0]
        return {int(k): (r[1:5].tolist(), r[5:9].tolist()) for k, r in zip(rows[:, 0].view(np.uint64).tolist(), rows)}

    def q(self) -> dict:
        """{(key, a): q} for the four actions of every stored state; a pair never seen reads 0.0."""
        return {(k, a): v for k, e in self.table().items() for a, v in enumerate(q_of_entry(e, self.frac_bits))}

    def greedy(self, keys, round=None) -> list:
        """The greedy action the roll-out of `round` takes in each of `keys` (the keys of boards as they lie), or None where the table
        has no entry.  With `symmetric` a key is looked up as its canonical state and the action comes back in the board's own frame."""
        table, r = self.table(), self.round if round is None else int(round)
        out = []
        for k in keys:
            k, j = canon_key_on_host(int(k), self.n) if self.symmetric else (int(k), 0)
            out.append(ACTION_UNMAP[j][greedy_on_host(table[k], k, self.tie_seed, r)] if k in table else None)
        return out

    def eval_board_id0(self) -> int:
        """evaluate()'s default boards: board_id0 + 2^62 + g.  Round r trains on board_id0 + r * n_games + g, so training meets them
        only after 2^62 / n_games rounds; every call with the default replays the same spawns (scores of two tables are paired)."""
        return (self.board_id0 + (1 << 62)) & 0xFFFFFFFFFFFFFFFF

    def evaluate_launch(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False):
        """The launch of evaluate() alone (pulse_tfe_mc_evaluate): ADDS to the counters of `eval_counters` and reads nothing back.
        Returns the per-game device tensors (total_score int64[B], lengths int32[B]) with per_game, else None."""
        import torch
        B = self.n_games if n_games is None else int(n_games)
        o = _native.TfeMCEval()
        o.entries, o.capacity, o.n_games, o.n, o.max_steps, o.frac_bits = self.entries.data_ptr(), self.capacity, B, self.n, self.max_steps, self.frac_bits
        o.epsilon, o.env_seed, o.agent_seed, o.tie_seed, o.round = float(epsilon), self.env_seed, self.agent_seed, self.tie_seed, self.round
        o.board_id0 = self.eval_board_id0() if board_id0 is None else int(board_id0)
        o.canonical = int(self.symmetric)
        o.summary, o.max_tile_hist = self._eval.data_ptr(), self._eval[len(EVAL_SUMMARY):].data_ptr()
        arrays = None
        if per_game:
            arrays = (torch.zeros(B, dtype=torch.int64, device=self.device), torch.zeros(B, dtype=torch.int32, device=self.device))
            o.total_score, o.lengths = arrays[0].data_ptr(), arrays[1].data_ptr()
        _native.check(self._lib.pulse_tfe_mc_evaluate(C.byref(o), _native.current_stream(self.device)), "pulse_tfe_mc_evaluate")
        return arrays

    def eval_counters(self, clear=False) -> dict:
        """What the evaluation launches since the last clear added up to (eval_summary_on_host; synchronises), or, with clear, nothing:
        the counters are zeroed."""
        if clear:
            self._eval.zero_()
            return {}
        return eval_summary_on_host(self._eval.cpu().tolist())

    def evaluate(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False) -> dict:
        """One launch and one read-back: `n_games` games (default: the agent's) under the table as it stands and `epsilon` (default 0:
        the greedy policy; a state without an entry still plays the uniform default), no trajectory.  With equal seeds, round, epsilon
        and board_id0 they are the games rollout() plays.  Returns the counters by name, the histogram of the largest tile, mean /
        standard deviation / maximum of the final score, the mean length, the games cut at max_steps and the share of moves whose
        state had an entry; per_game adds the arrays total_score / lengths."""
        self.eval_counters(clear=True)
        arrays = self.evaluate_launch(n_games, epsilon, board_id0, per_game)
        out = self.eval_counters()
        if per_game:
            out["total_score"], out["lengths"] = arrays[0].cpu().numpy(), arrays[1].cpu().numpy()
        return out

    def stats(self) -> dict:
        return dict(zip(STATS, self.counters.cpu().tolist()[:4]))

    def trajectory(self):
        """(keys uint64[T, B], steps uint8[T, B], lengths int32[B]) of the last batch, T = the longest game; rows at and beyond a
        game's length hold whatever the buffers held before."""
        lengths = self.lengths.cpu().numpy()
        T = int(lengths.max()) if lengths.size else 0
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
        self.round = 0
        return self
