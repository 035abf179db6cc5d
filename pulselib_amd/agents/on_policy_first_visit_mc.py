"""On-policy first-visit Monte-Carlo control on the CPU, epsilon-soft.

Interface and arithmetic of the reference's agents/MonteCarlo/OnPolicyFirstVisit.py:6-71.  `learn` takes one episode as
[(state, action, reward), ...] and walks it backwards with G_t = gamma * G_{t+1} + r_t; at the FIRST occurrence of a
(state, action) pair, G_t joins that pair's running mean (`returns[pair] = [sum, count]`, `q[pair] = sum / count`).  At EVERY
step the state's policy is made epsilon-soft around its greedy action: 1 - epsilon + epsilon / n for it, epsilon / n for the
others.  The greedy action is found by scanning the actions in order; a q equal to the best so far replaces it on a coin
(`random.random() > 0.5`, one draw per tie), and reading the q of a pair never seen inserts 0.0 for it, as the reference's
defaultdict does -- so the key sets, and under one `random.seed` every draw of `action` and `learn`, are the reference's."""
from __future__ import annotations

import random
from collections import defaultdict


class OnPolicyFirstVisitMC:
    def __init__(self, gamma: float, epsilon: float, n_actions: int = 2):
        self.gamma, self.epsilon, self.n = gamma, epsilon, int(n_actions)
        self.actions = list(range(self.n))
        self.q = defaultdict(float)                                        # state + (action,) -> mean first-visit return
        self.returns = defaultdict(lambda: [0.0, 0.0])                     # state + (action,) -> [sum of returns, count]
        self.policy = defaultdict(lambda: [1.0 / self.n] * self.n)         # state -> probability of each action

    def action(self, state):
        return random.choices(population=self.actions, weights=self.policy[state], k=1)[0]

    def _greedy(self, state):
        best, best_q = 0, float("-inf")
        for a in self.actions:
            q = self.q[state + (a,)]
            if q > best_q:
                best, best_q = a, q
            elif q == best_q and random.random() > 0.5:
                best = a
        return best

    def learn(self, episode):
        first_seen = {}
        for t, (state, action, _) in enumerate(episode):
            first_seen.setdefault(state + (action,), t)
        tail = 0
        for t in reversed(range(len(episode))):
            state, action, reward = episode[t]
            tail = self.gamma * tail + reward
            pair = state + (action,)
            if first_seen[pair] == t:
                record = self.returns[pair]
                record[0] += tail
                record[1] += 1.0
                self.q[pair] = record[0] / record[1]
            greedy = self._greedy(state)
            probs = self.policy[state]
            for a in self.actions:
                probs[a] = 1 - self.epsilon + self.epsilon / self.n if a == greedy else self.epsilon / self.n
