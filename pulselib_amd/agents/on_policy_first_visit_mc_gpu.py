"""On-policy first-visit Monte-Carlo control for Blackjack on the device (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71 and the
reset / step / per-game learn() loop that would feed it): two launches per batch of games and nothing read back in between.

`pulse_blackjack_mc_control_rollout` (csrc/blackjack_mc.hip) shuffles, plays under the agent's own epsilon-soft table and counts
first visits of (state, action) pairs per (k steps before the terminal reward, sign of that reward) into an int64 histogram;
`pulse_blackjack_mc_improve` turns the histogram into q(s, a) and the next table.  A stand ends the game, so it is only ever
seen at k = 0: a state has 32 hit cells and 2 stand cells.

Against the reference: the policy improves once per BATCH of games, not after every game, and the coin
that breaks an exact tie between q(s, hit) and q(s, stand) is drawn again for every visited state at every improvement.
`returns_from_action_histogram` and `improve_on_host` are the host's statement of the same arithmetic, in float64."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native
from .first_visit_mc_gpu import MAX_ACTIONS, N_STATES, HitPolicy, FirstVisitMonteCarloGPU, _BlackjackMCAgent, state_from_index, state_index  # noqa: F401

CELLS = _native.BJ_MCC_CELLS                              # per state: hit x k 0..15 x sign, then stand x sign
ACC_LEN = _native.BJ_MCC_ACC_LEN
HIT, STAND = 0, 1                                         # the env's actions (blackjack.py:116,137)


def cell_hit(state: int, k: int, negative: int) -> int:
    """PULSE_BJ_MCC_CELL_HIT (include/pulse_env.h)"""
    return state * CELLS + k * 2 + int(negative)


def cell_stand(state: int, negative: int) -> int:
    """PULSE_BJ_MCC_CELL_STAND (include/pulse_env.h)"""
    return state * CELLS + MAX_ACTIONS * 2 + int(negative)


def _sums_and_counts(hist, gamma: float):
    """float64[N_STATES, 2] sums of returns and int64[N_STATES, 2] counts, (hit, stand): gamma^k by repeated multiplication from
    1.0 and a pair's sum over k in ascending order, as first_visit_mc_gpu.returns_from_histogram forms them."""
    h = np.asarray(hist, dtype=np.int64).reshape(N_STATES, CELLS)
    hit = h[:, :MAX_ACTIONS * 2].reshape(N_STATES, MAX_ACTIONS, 2)
    stand = h[:, MAX_ACTIONS * 2:]
    counts = np.stack([hit.sum(axis=(1, 2)), stand.sum(axis=1)], axis=1)
    sums = np.zeros((N_STATES, 2), dtype=np.float64)
    p = 1.0
    for k in range(MAX_ACTIONS):
        sums[:, HIT] += (hit[:, k, 0] - hit[:, k, 1]).astype(np.float64) * p
        p = float(gamma) * p
    sums[:, STAND] = (stand[:, 0] - stand[:, 1]).astype(np.float64)
    return sums, counts


def returns_from_action_histogram(hist, gamma: float) -> dict:
    """{(sum, has_ace, upcard, action): [sum of returns, count]} of every pair seen, from the launch's histogram
    int64[N_STATES, CELLS]."""
    sums, counts = _sums_and_counts(hist, gamma)
    return {state_from_index(s) + (a,): [float(sums[s, a]), float(counts[s, a])]
            for s, a in zip(*(x.tolist() for x in np.nonzero(counts)))}


def improve_on_host(hist, gamma: float, epsilon: float, hit_prob, tie_stand):
    """pulse_blackjack_mc_improve on the host: (q float64[N_STATES, 2], the new fp32[N_STATES] table).  tie_stand: bool[N_STATES],
    the coin of each state (True = an exact tie goes to stand); the kernel draws them from Philox, this takes them as given."""
    sums, counts = _sums_and_counts(hist, gamma)
    q = np.zeros((N_STATES, 2), dtype=np.float64)
    np.divide(sums, counts.astype(np.float64), out=q, where=counts > 0)     # an unseen pair reads 0.0 (defaultdict(float))
    stand = np.where(q[:, STAND] == q[:, HIT], np.asarray(tie_stand, dtype=bool), q[:, STAND] > q[:, HIT])
    explore = float(epsilon) / 2.0
    soft = np.where(stand, explore, 1.0 - float(epsilon) + explore).astype(np.float32)
    out = np.array(hit_prob, dtype=np.float32).reshape(N_STATES)
    visited = counts.sum(axis=1) > 0
    out[visited] = soft[visited]
    return q, out


class OnPolicyFirstVisitMCGPU(_BlackjackMCAgent):
    """`learn_batch` plays n_games x n_episodes games under the agent's table and adds their pair first visits to the device
    histogram; `improve` makes the table epsilon-soft around the greedy actions of that histogram; `train` alternates the two."""

    def __init__(self, device, gamma: float, epsilon: float, seed: int = 0):
        import torch
        super().__init__(device, seed)
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.round = 0                                                     # the number of improvements so far
        self.acc = torch.zeros(ACC_LEN, dtype=torch.int64, device=self.device)
        self.hit_prob = torch.full((N_STATES,), 0.5, dtype=torch.float32, device=self.device)   # the reference's uniform default
        self.q_table = torch.zeros((N_STATES, 2), dtype=torch.float64, device=self.device)      # written by improve()

    # ------------------------------------------------------------------ the launches
    def learn_batch(self, n_games: int, n_episodes: int = 1, decks=None, trace: bool = False, max_blocks: int = 0, policy=None):
        """One roll-out launch, no host sync, under the agent's own table -- or under `policy` (a device fp32[N_STATES] table,
        threshold_policy(n) or uniform_policy()).  decks: None = the env's device shuffle, else int32[n_episodes * n_games, 52]."""
        table = self.hit_prob if policy is None else self._table(policy)
        return self._rollout(_native.BlackjackMCControl, "pulse_blackjack_mc_control_rollout", table, n_games, n_episodes, decks, trace, max_blocks)

    def improve(self):
        """One launch: q(s, a) of the histogram so far into `q_table`, and `hit_prob` epsilon-soft around its greedy actions."""
        o = _native.BlackjackMCImprove()
        o.acc, o.gamma, o.epsilon, o.seed, o.round = self.acc.data_ptr(), self.gamma, self.epsilon, self.seed, self.round
        o.q, o.hit_prob = self.q_table.data_ptr(), self.hit_prob.data_ptr()
        _native.check(self._lib.pulse_blackjack_mc_improve(C.byref(o), _native.current_stream(self.device)), "pulse_blackjack_mc_improve")
        self.round += 1
        return self

    def train(self, batches: int, n_games: int, n_episodes: int = 1):
        """roll-out, improve, repeat: two launches per batch, no synchronisation and nothing read back."""
        for _ in range(int(batches)):
            self.learn_batch(n_games, n_episodes)
            self.improve()
        return self

    # ------------------------------------------------------------------ read-back (the only syncs)
    def histogram(self) -> np.ndarray:
        return self.acc.cpu().numpy().reshape(N_STATES, CELLS)

    @property
    def returns(self) -> dict:
        return returns_from_action_histogram(self.histogram(), self.gamma)

    @property
    def q(self) -> dict:
        """{(sum, has_ace, upcard, action): mean first-visit return} for both actions of every state visited: the pair not seen
        reads 0.0, as it does in the reference's table once `learn` has looked it up."""
        sums, counts = _sums_and_counts(self.histogram(), self.gamma)
        out = {}
        for s in np.nonzero(counts.sum(axis=1))[0].tolist():
            for a in (HIT, STAND):
                out[state_from_index(s) + (a,)] = float(sums[s, a]) / float(counts[s, a]) if counts[s, a] else 0.0
        return out

    @property
    def policy(self) -> dict:
        """{state: [p_hit, p_stand]} of every state visited, from the device table."""
        p = self.hit_prob.cpu().numpy().astype(np.float64)
        visited = np.nonzero(self.histogram().sum(axis=1))[0].tolist()
        return {state_from_index(s): [float(p[s]), 1.0 - float(p[s])] for s in visited}

    def greedy_policy(self) -> dict:
        """{state: HIT or STAND} of every state visited: the action the table favours."""
        return {s: HIT if p[0] > p[1] else STAND for s, p in self.policy.items()}

    def clear(self):
        """A new estimate: histogram, counters and q emptied, the table uniform again, round 0."""
        self.acc.zero_()
        self.counters.zero_()
        self.q_table.zero_()
        self.hit_prob.fill_(0.5)
        self.round = 0
        return self
