"""What the 2048 device agents share (tfe_on_policy_mc_gpu.py, tfe_ntuple_td_gpu.py; csrc/tfe_agent_device.h is the device's half): the
keys of the three Philox streams, Philox itself, the state key and its symmetries, the per-move byte, the reward, the greedy scan
with its tie coins and the evaluation counters as the host states them, and the base class of the agents: seeds, the buffers of a
batch of games, the evaluation launch and the read-backs.  An agent adds its own structs, entry points, buffers and counter names."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .. import _native

AGENT_KEY = 0x2048AC7105EED                     # the agent's draws are keyed apart from the environment's (the seed itself) ...
TIE_KEY = 0x20487C01F11B5                       # ... and the tie coins apart from both
EVAL_BINS = 16                                  # bin = log2 of the largest tile of the final board
_U64 = np.uint64


# ------------------------------------------------------------------ Philox
def _philox_rounds(seed: int, c0, c1, c2, c3):
    """Philox4x32-10 on four 32-bit counter words held in Python ints, or in uint64 arrays (32 x 32 -> 64 bits: no overflow)."""
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox4x32(seed: int, subseq: int, offset: int):
    """Philox4x32-10 with the device's layout (csrc/philox_device.h): counter {offset, subseq}, key = seed.  Four uint32 as ints."""
    return list(_philox_rounds(seed, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF, subseq & 0xFFFFFFFF, (subseq >> 32) & 0xFFFFFFFF))


def philox_many_on_host(seed: int, subseq, offset) -> np.ndarray:
    """uint32[N, 4]: philox4x32 for arrays (or scalars) of subseq and offset."""
    subseq, offset = np.broadcast_arrays(np.asarray(subseq, dtype=_U64).reshape(-1), np.asarray(offset, dtype=_U64).reshape(-1))
    m32 = _U64(0xFFFFFFFF)
    return np.stack(_philox_rounds(seed, offset & m32, offset >> _U64(32), subseq & m32, subseq >> _U64(32)), axis=1).astype(np.uint32)


# ------------------------------------------------------------------ the state key, its symmetries, the per-move byte, the reward
def pack_board(board) -> int:
    """The state key: 4 bits of log2(tile) per cell (0 = empty), row-major, cell 0 in the low nibble."""
    key = 0
    for i, v in enumerate(np.asarray(board).ravel().tolist()):
        key |= (min(int(v).bit_length() - 1, 15) if v > 0 else 0) << (4 * i)
    return key


def unpack_key(key: int, n: int) -> list:
    """The n * n log2 tiles of a state key, row-major."""
    return [(int(key) >> (4 * i)) & 15 for i in range(n * n)]


def transforms_on_host(n: int) -> np.ndarray:
    """int64[8, n * n]: T_j(B).ravel() == B.ravel()[transforms_on_host(n)[j]] for the eight symmetries of the square (DESIGN.md
    section 12.1): T_0..T_3 rotate the board 0..3 times by the environment's own rotation (TFE.py:38-44: out[r][c] = in[c][n - 1 - r]),
    T_4..T_7 do the same to the transposed board."""
    out = np.zeros((8, n * n), dtype=np.int64)
    for j in range(8):
        for r in range(n):
            for c in range(n):
                rr, cc = r, c
                for _ in range(j & 3):                                     # rot_src of csrc/tfe_device.h
                    rr, cc = cc, n - 1 - rr
                out[j, r * n + c] = cc * n + rr if j >= 4 else rr * n + cc
    return out


def unpack_steps(steps):
    """(action, reward, flag) of the per-move bytes; the flag is the learner's: a first visit, or the game's terminal move."""
    s = np.asarray(steps, dtype=np.uint8)
    return s & 3, (s >> 2) & 31, (s >> 7).astype(bool)


def reward_of_score(score: int) -> int:
    """TFE.py:185-187: bit length - 1 of the merge score of a move, 0 for 0."""
    return int(score).bit_length() - 1 if score > 0 else 0


def rewards_of_scores(scores) -> np.ndarray:
    """reward_of_score over an array (scores are sums of powers of two below 2^18: exact)."""
    s = np.asarray(scores, dtype=np.int64)
    return np.where(s > 0, np.floor(np.log2(np.maximum(s, 1))).astype(np.int64), 0)


# ------------------------------------------------------------------ the greedy scan (greedy_scan of csrc/tfe_agent_device.h)
def greedy_scan_on_host(q, coins, cand=(True, True, True, True)) -> int:
    """The greedy action among four q: the candidates in the order a = 0..3, the first is the best so far, a larger q replaces it, an
    equal q replaces it iff bit 31 of word a - 1 of coins() is set.  -1: no candidate.  `coins` is called once, and only if two q
    meet as equals."""
    words, best, best_q = None, -1, 0.0
    for a in range(4):
        if not cand[a]:
            continue
        if best < 0 or q[a] > best_q:
            best, best_q = a, q[a]
        elif q[a] == best_q:
            if words is None:
                words = [int(w) for w in coins()]
            if words[a - 1] >> 31:
                best = a
    return best


def greedy_scan_many_on_host(q, coins, cand) -> np.ndarray:
    """greedy_scan_on_host over N boards at once: q float64[N, 4], coins uint32[N, 4] (the Philox words), cand bool[N, 4].  int64[N]."""
    best, best_q = np.full(len(q), -1, dtype=np.int64), np.zeros(len(q), dtype=np.float64)
    for a in range(4):
        take = cand[:, a] & ((best < 0) | (q[:, a] > best_q))
        if a:
            take |= cand[:, a] & (best >= 0) & (q[:, a] == best_q) & (coins[:, a - 1] >> np.uint32(31) != 0)
        best, best_q = np.where(take, a, best), np.where(take, q[:, a], best_q)
    return best


# ------------------------------------------------------------------ the evaluation launches' counters
def eval_summary_on_host(words, names) -> dict:
    """An evaluation launch's 8 + 16 counters as a dict: the words by `names`, the histogram of the largest tile (bin = its log2), and
    mean / std (sample standard deviation, from the exact integer sums) of the final score and the mean length; where the agent
    counts `moves_with_entry`, `coverage`: the share of moves whose state had a table entry."""
    w = [int(x) for x in words]
    out = dict(zip(names, w[:len(names)]))
    n, s, ss = out["games"], out["score_sum"], out["score_sq_sum"]
    out["max_tile_hist"] = w[len(names):len(names) + EVAL_BINS]
    out["mean_score"] = s / n if n else 0.0
    out["std_score"] = math.sqrt((n * ss - s * s) / (n * (n - 1))) if n > 1 else 0.0          # exact integers under the root
    out["mean_length"] = out["moves"] / n if n else 0.0
    if "moves_with_entry" in names:
        out["coverage"] = out["moves_with_entry"] / out["moves"] if out["moves"] else 0.0
    return out


# ------------------------------------------------------------------ the agents' base class
class _TFEGamesGPU:
    """A device agent that plays batches of whole 2048 games: the seeds, the round, the trajectory and score buffers, the evaluation
    launch and the read-backs.  A subclass names its counters (STATS, EVAL_SUMMARY), fills its own structs and launches them, and
    gives the evaluation its struct (`_eval_struct`) and its entry point (`_eval_launch`)."""
    STATS = EVAL_SUMMARY = ()

    def __init__(self, device, n_games, n, max_steps, gamma, epsilon, seed, board_id0):
        import torch
        device = _native.gpu_device(device, type(self).__name__)
        if int(n_games) < 1 or not 1 <= int(max_steps) <= 65535:
            raise ValueError("n_games must be positive and max_steps in 1..65535")
        if not (0.0 <= gamma <= 1.0 and 0.0 <= epsilon <= 1.0):
            raise ValueError("gamma and epsilon must be in [0, 1]")
        self._lib = _native.lib()
        self.device = device
        self.n_games, self.n, self.max_steps = int(n_games), int(n), int(max_steps)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.seed, self.board_id0, self.round = int(seed), int(board_id0), 0
        self.env_seed, self.agent_seed, self.tie_seed = self.seed, self.seed ^ AGENT_KEY, self.seed ^ TIE_KEY
        self.keys = torch.zeros((self.max_steps, self.n_games), dtype=torch.int64, device=device)    # (uint64 words)
        self.steps = torch.zeros((self.max_steps, self.n_games), dtype=torch.uint8, device=device)
        self.lengths = torch.zeros(self.n_games, dtype=torch.int32, device=device)
        self.total_score = torch.zeros(self.n_games, dtype=torch.int64, device=device)
        self.episode_reward = torch.zeros(self.n_games, dtype=torch.int32, device=device)
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)
        self._eval = torch.zeros(len(self.EVAL_SUMMARY) + EVAL_BINS, dtype=torch.int64, device=device)     # evaluate(): summary, then the histogram

    def _launch(self, name, o, *args):
        _native.check(getattr(self._lib, name)(C.byref(o), *args, _native.current_stream(self.device)), name)
        return self

    def _draws(self, o, board_id0):
        """The streams of a batch of games: the three seeds, the first board's id and the round of the tie coins."""
        o.env_seed, o.agent_seed, o.tie_seed, o.board_id0, o.round = self.env_seed, self.agent_seed, self.tie_seed, board_id0, self.round
        return o

    def round_board_id0(self, round=None) -> int:
        return self.board_id0 + (self.round if round is None else int(round)) * self.n_games

    def eval_board_id0(self) -> int:
        """evaluate()'s default boards: board_id0 + 2^62 + g.  Round r trains on board_id0 + r * n_games + g, so training meets them
        only after 2^62 / n_games rounds; every call with the default replays the same spawns (scores of two policies are paired)."""
        return (self.board_id0 + (1 << 62)) & 0xFFFFFFFFFFFFFFFF

    def evaluate_launch(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False):
        """The launch of evaluate() alone: ADDS to the counters of `eval_counters` and reads nothing back.  Returns the per-game device
        tensors (total_score int64[B], lengths int32[B]) with per_game, else None."""
        return self._evaluate_launch_with(self._eval_launch, n_games, epsilon, board_id0, per_game)

    def _evaluate_launch_with(self, launch, n_games, epsilon, board_id0, per_game):
        """evaluate_launch's body: the evaluation's struct filled, then launch(struct) -- the agent's `_eval_launch`, or the entry point
        of another policy on the same struct."""
        import torch
        B = self.n_games if n_games is None else int(n_games)
        o = self._draws(self._eval_struct(), self.eval_board_id0() if board_id0 is None else int(board_id0))
        o.n_games, o.max_steps, o.epsilon = B, self._eval_cap(), float(epsilon)
        o.summary, o.max_tile_hist = self._eval.data_ptr(), self._eval[len(self.EVAL_SUMMARY):].data_ptr()
        arrays = None
        if per_game:
            arrays = (torch.zeros(B, dtype=torch.int64, device=self.device), torch.zeros(B, dtype=torch.int32, device=self.device))
            o.total_score, o.lengths = arrays[0].data_ptr(), arrays[1].data_ptr()
        launch(o)
        return arrays

    def _eval_cap(self) -> int:
        """The cap of an evaluation's games: the attribute `eval_max_steps` where the agent has one that is not None (1..65,535;
        ValueError otherwise), else the agent's max_steps.  The evaluation launches hold no per-move buffers: any cap is free."""
        cap = getattr(self, "eval_max_steps", None)
        if cap is None:
            return self.max_steps
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= int(cap) <= 65535:
            raise ValueError("eval_max_steps must be None or an int in 1..65535")
        return int(cap)

    def eval_counters(self, clear=False) -> dict:
        """What the evaluation launches since the last clear added up to (eval_summary_on_host; synchronises), or, with clear, nothing:
        the counters are zeroed."""
        if clear:
            self._eval.zero_()
            return {}
        return eval_summary_on_host(self._eval.cpu().tolist(), self.EVAL_SUMMARY)

    def evaluate(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False) -> dict:
        """One launch and one read-back: `n_games` games (default: the agent's) under the policy as it stands and `epsilon` (default 0:
        the greedy policy), no trajectory.  With equal seeds, round, epsilon and board_id0 they are the games rollout() plays.  Returns
        what eval_summary_on_host makes of the agent's counters; per_game adds the arrays total_score / lengths."""
        return self._evaluate_with(self._eval_launch, n_games, epsilon, board_id0, per_game)

    def _evaluate_with(self, launch, n_games, epsilon, board_id0, per_game) -> dict:
        """evaluate's body: the counters cleared, _evaluate_launch_with(launch, ...) and the read-back."""
        self.eval_counters(clear=True)
        arrays = self._evaluate_launch_with(launch, n_games, epsilon, board_id0, per_game)
        out = self.eval_counters()
        if per_game:
            out["total_score"], out["lengths"] = arrays[0].cpu().numpy(), arrays[1].cpu().numpy()
        return out

    def stats(self) -> dict:
        return dict(zip(self.STATS, self.counters.cpu().tolist()))

    def _played(self):
        """(T, lengths int32[B]) of the last batch, T = the longest game: rows at and beyond a game's length hold whatever the buffers
        held before."""
        lengths = self.lengths.cpu().numpy()
        return (int(lengths.max()) if lengths.size else 0), lengths
