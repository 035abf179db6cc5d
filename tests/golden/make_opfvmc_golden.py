"""Generate tests/golden/opfvmc.npz by RUNNING THE REFERENCE's agents/MonteCarlo/OnPolicyFirstVisit.py.

Usage (only where the reference checkout exists; never on the GPU box):
    python tests/golden/make_opfvmc_golden.py

Recorded (arrays only, no reference source text):
  steps, episode_lengths   seeded blackjack-shaped episodes, rows (sum, usable ace, upcard, action, reward): hits (0) with
                           reward 0, then a last action that is a hit with -1 or a stand (1) with +-1.  Among them: pairs that
                           repeat within an episode, states whose two actions tie at exactly equal q (both seen, and one seen
                           against the 0.0 of the one never seen), episodes of length 1;
  seed                     `random.seed(seed)` precedes every run (the tie coins of learn, the draws of action);
  r{i}/gamma, epsilon      gamma in {0.5, 0.9} x epsilon in {0.1, 0.3};
  r{i}/draw_states, draws  action() called on a handful of states after the last episode (two of them never seen: the call
                           enters them into the policy table);
  r{i}/q_*, returns_*, policy_*   every key (in the tables' own order) and value of q, returns and policy after the draws.
"""
from __future__ import annotations

import random
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import make_golden as mg  # noqa: E402

SEED = 20261
RUNS = ((0.5, 0.1), (0.5, 0.3), (0.9, 0.1), (0.9, 0.3))


def episodes():
    A, B, D, E = (16, 0, 10), (13, 0, 4), (14, 1, 9), (19, 1, 9)
    out = [
        [(B, 0, 0), (B, 0, 0), ((15, 0, 4), 1, 1)],             # (B, hit) twice: only the first counts
        [(A, 0, -1)], [(A, 1, -1)],                             # length 1; q(A, hit) = q(A, stand) = -1 exactly
        [(D, 0, 0), (E, 1, 1)], [(D, 0, 0), (E, 1, -1)],        # q(D, hit) = 0 = the unseen (D, stand); likewise (E, stand)
    ]
    rng = np.random.default_rng(SEED)
    for _ in range(120):
        T = int(rng.integers(1, 6))
        ep, state = [], None
        for t in range(T):
            if state is None or rng.random() >= 0.15:           # else the state repeats, and with it the pair (state, hit)
                state = (int(rng.integers(12, 18)), int(rng.integers(0, 2)), int(rng.integers(2, 5)))
            if t < T - 1:
                ep.append((state, 0, 0))
            elif rng.random() < 0.4:
                ep.append((state, 0, -1))
            else:
                ep.append((state, 1, 1 if rng.random() < 0.45 else -1))
        out.append(ep)
    order = rng.permutation(len(out))
    return [out[i] for i in order.tolist()]


def main():
    mg._install_gym_stub()
    ref = mg._load_by_path("ref_opfvmc", "agents/MonteCarlo/OnPolicyFirstVisit.py")
    space = sys.modules["gymnasium"].spaces.Discrete(2)
    eps = episodes()
    store = {"seed": np.array(SEED), "episode_lengths": np.array([len(e) for e in eps], dtype=np.int64),
             "steps": np.array([[*s, a, r] for e in eps for s, a, r in e], dtype=np.int64), "runs": np.array(len(RUNS))}
    seen = sorted({s for e in eps for s, _, _ in e})
    draw_states = [seen[i] for i in range(0, len(seen), max(1, len(seen) // 10))][:10] + [(5, 0, 2), (21, 1, 11)]
    for i, (gamma, epsilon) in enumerate(RUNS):
        random.seed(SEED)
        agent = ref.OnPolicyFirstVisitMC(gamma, epsilon, space)
        for e in eps:
            agent.learn(e)
        draws = [agent.action(s) for s in draw_states for _ in range(4)]
        store[f"r{i}/gamma"], store[f"r{i}/epsilon"] = np.array(gamma), np.array(epsilon)
        store[f"r{i}/draw_states"] = np.array([s for s in draw_states for _ in range(4)], dtype=np.int64)
        store[f"r{i}/draws"] = np.array(draws, dtype=np.int64)
        for name, table, width in (("q", agent.q, 4), ("returns", agent.returns, 4), ("policy", agent.policy, 3)):
            keys = list(table)
            store[f"r{i}/{name}_keys"] = np.array(keys, dtype=np.int64).reshape(len(keys), width)
            store[f"r{i}/{name}_values"] = np.array([table[k] for k in keys], dtype=np.float64)
    out = HERE / "opfvmc.npz"
    np.savez_compressed(out, **store)
    print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
