"""On-policy first-visit Monte-Carlo control for 2048 on the device (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71 on the games of
scripts/TFE/mctrain.py): two launches per batch of games and nothing read back in between.

`pulse_tfe_mc_rollout` (csrc/tfe_mc.hip) plays `n_games` whole games, one lane each, against the policy of a hash table of
states in HBM and records one key and one byte per move; `pulse_tfe_mc_learn` walks the games backwards and adds the first-visit
returns into that table as fixed-point integers.  The table holds per (state, action) the count and the sum of those returns:
q(s, a) = sum / count * 2^-frac_bits, 0.0 where nothing was seen (the reference's defaultdict(float)).

Against the reference: the policy improves once per BATCH of games, not after every game; the coin that
breaks a tie between equal q is drawn per (state, round), not per look; actions and spawns come from Philox streams; a game is cut
at `max_steps` moves.  Round r plays the boards board_id0 + r * n_games + g, so no two rounds replay the same spawns.

`learn_on_host`, `greedy_on_host`, `first_visit_flags_on_host` and `run_mask_flags_on_host` are the host's statement of the same
arithmetic, in numpy and pure Python."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _native

ENTRY_BYTES, MAX_PROBE, R_MAX = _native.TFE_MC_ENTRY_BYTES, _native.TFE_MC_MAX_PROBE, _native.TFE_MC_R_MAX
AGENT_KEY = 0x2048AC7105EED                     # the agent's draws are keyed apart from the environment's (the seed itself) ...
TIE_KEY = 0x20487C01F11B5                       # ... and the tie coins apart from both
STATS = ("steps", "first_visits", "dropped", "truncated")


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


class OnPolicyFirstVisitMCTFEGPU:
    """`learn_batch` = `rollout` + `learn` + `round += 1`, two launches and no synchronisation.  Everything that reads back
    (`table`, `q`, `greedy`, `stats`, `trajectory`, the per-game arrays' `.cpu()`) synchronises."""

    def __init__(self, device, n_games, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 22, max_steps=1024, seed=0, board_id0=0):
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
        self.seed, self.board_id0, self.round = int(seed), int(board_id0), 0
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
        """One launch: n_games games under the table as it stands (round `self.round`), into keys / steps / lengths / scores."""
        o = self._head(_native.TfeMCRollout())
        o.env_seed, o.agent_seed, o.tie_seed, o.board_id0, o.round = self.env_seed, self.agent_seed, self.tie_seed, self.round_board_id0(), self.round
        o.total_score, o.episode_reward = self.total_score.data_ptr(), self.episode_reward.data_ptr()
        _native.check(self._lib.pulse_tfe_mc_rollout(C.byref(o), _native.current_stream(self.device)), "pulse_tfe_mc_rollout")
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
        """The greedy action the roll-out of `round` takes in each of `keys`, or None where the table has no entry."""
        table, r = self.table(), self.round if round is None else int(round)
        return [greedy_on_host(table[int(k)], int(k), self.tie_seed, r) if int(k) in table else None for k in keys]

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
