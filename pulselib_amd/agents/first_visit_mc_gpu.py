"""First-visit Monte-Carlo state-value estimation for Blackjack on the device: shuffle, play and learn in ONE launch
(csrc/blackjack_mc.hip, pulse_blackjack_mc_rollout) instead of reset + up to 12 steps + a per-game learn() on the host
(scripts/blackjack_fvmc.py: run).

The reward of a Blackjack game is 0 before the terminal step and +-1 at it, so the first-visit return of the state seen k steps
before the terminal step is r * gamma^k.  The launch counts first visits per (state, k, sign of r) into an int64 histogram --
integer adds, the same bit for bit whatever order they land in -- and `returns_from_histogram` turns the histogram into the
reference's `returns[state] = [sum of returns, count]` (agents/MonteCarlo/FirstVisitMonteCarlo.py:5-31) on the host in float64.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native

MAX_ACTIONS = _native.BJ_MC_MAX_ACTIONS                   # k = 0 .. 15
N_STATES = _native.BJ_MC_STATES                           # 32 sums x 2 x 16 upcards
ACC_LEN = _native.BJ_MC_ACC_LEN


def state_index(player_sum: int, has_ace: int, upcard: int) -> int:
    """PULSE_BJ_MC_STATE_INDEX (include/pulse_env.h): player's sum 0..31, usable ace 0/1, dealer's upcard 0..15."""
    if not (0 <= player_sum < 32 and has_ace in (0, 1) and 0 <= upcard < 16):
        raise ValueError(f"state {(player_sum, has_ace, upcard)} is outside the accumulator's layout")
    return (player_sum * 2 + int(has_ace)) * 16 + upcard


def state_from_index(index: int) -> tuple[int, int, int]:
    return index >> 5, (index >> 4) & 1, index & 15


def returns_from_histogram(hist, gamma: float) -> dict:
    """{(sum, has_ace, upcard): [sum of returns, count]} from the launch's histogram int64[N_STATES, MAX_ACTIONS, 2]
    (cell [s, k, 0] = first visits of s, k steps before a terminal reward of +1; [s, k, 1] = before a -1).

    gamma^k is built by repeated multiplication from 1.0 -- the k products `gamma * tail` of the reference's backward pass,
    which starts from the terminal reward +-1 -- and a state's sum runs over k in ascending order, in float64."""
    h = np.asarray(hist, dtype=np.int64).reshape(N_STATES, MAX_ACTIONS, 2)
    pow_k = np.empty(MAX_ACTIONS, dtype=np.float64)
    p = 1.0
    for k in range(MAX_ACTIONS):
        pow_k[k] = p
        p = float(gamma) * p
    counts = h.sum(axis=(1, 2))
    out = {}
    for s in np.nonzero(counts)[0].tolist():
        total = 0.0
        for k in range(MAX_ACTIONS):
            net = int(h[s, k, 0]) - int(h[s, k, 1])
            if net:
                total += float(net) * float(pow_k[k])
        out[state_from_index(s)] = [total, float(counts[s])]
    return out


class HitPolicy:
    """A named host-side table of hit probabilities (state_index order); an agent uploads it the first time it is used."""

    def __init__(self, key, table):
        self.key, self.table = key, np.ascontiguousarray(table, dtype=np.float32)


class _BlackjackMCAgent:
    """What the two Blackjack Monte-Carlo agents share: the env's counters, the launch's buffers, the policy tables and the
    roll-out launch itself.  A subclass owns `acc`, its histogram."""

    def __init__(self, device, seed: int):
        import torch
        self.device = device = _native.gpu_device(device, type(self).__name__)
        self._lib = _native.lib()
        self.seed, self.episode = int(seed), 0            # the env's counters: episode e is BlackJack(seed).reset() number e
        self.counters = torch.zeros(4, dtype=torch.int64, device=device)
        self.last_trace = None                            # int8[n_episodes * n_games, 16] of the last learn_batch(trace=True)
        self._policies = {}

    # ------------------------------------------------------------------ policies: fp32[N_STATES], probability of hitting
    @staticmethod
    def threshold_policy(hit_below: int = 17) -> "HitPolicy":
        """Hit while the player's sum is below `hit_below` (scripts/blackjack_fvmc.py: obs[:, 0] >= hit_below stands)."""
        return HitPolicy(("threshold", int(hit_below)), (np.arange(N_STATES) >> 5 < int(hit_below)).astype(np.float32))

    @staticmethod
    def uniform_policy() -> "HitPolicy":
        """The reference agent's action_space.sample(): hit with probability 0.5 in every state."""
        return HitPolicy(("uniform",), np.full(N_STATES, 0.5, dtype=np.float32))

    def _table(self, policy):
        import torch
        if isinstance(policy, HitPolicy):                 # uploaded once per agent, then the launch reads the device copy
            if policy.key not in self._policies:
                self._policies[policy.key] = torch.from_numpy(policy.table).to(self.device)
            return self._policies[policy.key]
        if not (isinstance(policy, torch.Tensor) and policy.dtype == torch.float32 and policy.device == self.device
                and policy.is_contiguous() and policy.numel() == N_STATES):
            raise ValueError(f"policy must be a contiguous fp32 tensor of {N_STATES} hit probabilities on {self.device}, "
                             "threshold_policy(n) or uniform_policy()")
        return policy

    # ------------------------------------------------------------------ the launch
    def _rollout(self, struct_type, symbol: str, table, n_games: int, n_episodes: int, decks, trace: bool, max_blocks: int):
        """One launch of `symbol` under the device table `table`, no host sync; its first visits are added to `acc`."""
        import torch
        n_games, n_episodes = int(n_games), int(n_episodes)
        o = struct_type()
        o.n_games, o.n_episodes, o.seed, o.episode = n_games, n_episodes, self.seed, self.episode
        o.hit_prob, o.acc, o.stats, o.max_blocks = table.data_ptr(), self.acc.data_ptr(), self.counters.data_ptr(), int(max_blocks)
        src = None
        if decks is not None:
            src = torch.as_tensor(decks).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(src.shape) != (n_games * n_episodes, 52):
                raise ValueError(f"decks must have shape {(n_games * n_episodes, 52)}, got {tuple(src.shape)}")
            o.decks_src = src.data_ptr()
        if trace:
            self.last_trace = torch.empty((max(n_games * n_episodes, 0), MAX_ACTIONS), dtype=torch.int8, device=self.device)
            o.trace = self.last_trace.data_ptr()
        _native.check(getattr(self._lib, symbol)(C.byref(o), _native.current_stream(self.device)), symbol)
        self.episode += n_episodes
        return self

    def stats(self) -> dict:
        games, wins, actions, capped = self.counters.cpu().tolist()
        return {"games": games, "wins": wins, "actions": actions, "capped": capped}


class FirstVisitMonteCarloGPU(_BlackjackMCAgent):
    """`learn_batch` plays n_games x n_episodes games under a fixed policy and adds their first visits to the device
    histogram; `returns` / `values` read it back in the shapes of the CPU class (agents/first_visit_mc.py)."""

    def __init__(self, device, gamma: float, seed: int = 0):
        import torch
        super().__init__(device, seed)
        self.gamma = float(gamma)
        self.acc = torch.zeros(ACC_LEN, dtype=torch.int64, device=self.device)

    def learn_batch(self, n_games: int, policy, n_episodes: int = 1, decks=None, trace: bool = False, max_blocks: int = 0):
        """One launch, no host sync.  policy: a device fp32[N_STATES] table, threshold_policy(n) or uniform_policy().
        decks: None = the env's device shuffle, else int32[n_episodes * n_games, 52] used as they are."""
        return self._rollout(_native.BlackjackMC, "pulse_blackjack_mc_rollout", self._table(policy), n_games, n_episodes, decks, trace, max_blocks)

    # ------------------------------------------------------------------ read-back (the only syncs)
    def histogram(self) -> np.ndarray:
        return self.acc.cpu().numpy().reshape(N_STATES, MAX_ACTIONS, 2)

    @property
    def returns(self) -> dict:
        return returns_from_histogram(self.histogram(), self.gamma)

    @property
    def values(self) -> dict:
        return {s: total / count for s, (total, count) in self.returns.items()}

    def clear(self):
        self.acc.zero_()
        self.counters.zero_()
        return self
