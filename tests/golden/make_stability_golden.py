"""Generate tests/golden/stability.npz by RUNNING THE REFERENCE's utils/stability.py and Player.PokerQNetwork on CPU torch.

Usage (only where the reference checkout exists; never on the GPU box):
    python tests/golden/make_stability_golden.py

Recorded (arrays and name lists only, no reference source text):
  steps/*   run_stability_measured_q_learning_step on seeded batches with mixed seat statuses in column 12 (one batch with
            no valid row), one network stepping through them; the initial weights, each batch, the seed of its dropout
            draws (torch.manual_seed before the call, as make_golden.make_qnetwork does) and the seven metrics per step (NaN row
            and valid = 0 where the reference returned None) -- each step's metrics depend on the updates before it;
  episode/* summarize_episode_stability_metrics over recorded per-step sequences (an empty one included);
  final/*   calculate_final_stability_metrics over recorded episode sequences: empty, one episode (trend 0), several.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import make_golden as mg  # noqa: E402

METRICS = ("loss", "td_error", "grad_norm", "clip_rate", "q_mean", "q_min", "q_max")
EPISODE = ("reward", "q_mean", "q_min", "q_max", "td_error", "clip_rate")
FINAL = ("reward_std", "mean_reward", "global_min", "global_max", "mean_q", "td_error_trend", "average_clip_rate", "total_time_seconds")
# (n rows, state scale, valid pattern): "mixed" = statuses 0..3 drawn, "none" = only FOLDED / OUT (1, 3)
BATCHES = ((300, 3.0, "mixed"), (77, 3.0, "mixed"), (50, 3.0, "none"), (129, 0.05, "mixed"), (1, 3.0, "active"), (400, 6.0, "mixed"))


def _flat_final(f):
    return [float(f["reward_std"]), float(f["mean_reward"]), float(f["q_bounds"]["global_min"]), float(f["q_bounds"]["global_max"]),
            float(f["q_bounds"]["mean_q"]), float(f["td_error_trend"]), float(f["average_clip_rate"]), float(f["total_time_seconds"])]


def main():
    from oracle import oracle as orc
    stab = mg._load_by_path("ref_stability", "utils/stability.py")
    player = mg.load_reference_player(mg.load_reference_poker(orc.hand_ranks()))
    store = {"metric_names": np.array(METRICS), "episode_names": np.array(EPISODE), "final_names": np.array(FINAL)}

    # ---- per-step metrics
    torch.manual_seed(4242)
    q = player.PokerQNetwork(weights_path="/nonexistent.pth", device=torch.device("cpu"), gamma=.95, update_freq=2, state_dim=40,
                             action_dim=13, learning_rate=2e-4, weight_decay=1e-5)
    for k, v in q.network.state_dict().items():
        store[f"steps/w0/{k}"] = v.detach().numpy().copy()
    rows, valid = [], []
    g = torch.Generator().manual_seed(7)
    for i, (n, scale, pattern) in enumerate(BATCHES):
        states = torch.randn((n, 40), generator=g) * scale
        if pattern == "mixed":
            states[:, 12] = torch.randint(0, 4, (n,), generator=g).float()
        elif pattern == "none":
            states[:, 12] = torch.where(torch.rand((n,), generator=g) < 0.5, 1.0, 3.0)
        else:
            states[:, 12] = 0.0
        next_states = torch.randn((n, 40), generator=g) * scale
        actions = torch.randint(0, 13, (n,), generator=g)
        rewards = torch.randn((n,), generator=g) * 5.0
        dones = torch.rand((n,), generator=g) < 0.3
        for name, x in (("states", states), ("next_states", next_states), ("actions", actions), ("rewards", rewards), ("dones", dones)):
            store[f"steps/b{i}/{name}"] = x.numpy().copy()
        seed = 900 + i
        store[f"steps/b{i}/seed"] = np.array(seed)
        torch.manual_seed(seed)
        m = stab.run_stability_measured_q_learning_step(q_network=q, states=states, actions=actions, rewards=rewards,
                                                        next_states=next_states, dones=dones)
        valid.append(m is not None)
        rows.append([float(m[k]) for k in METRICS] if m is not None else [np.nan] * len(METRICS))
    store["steps/metrics"] = np.array(rows, dtype=np.float64)
    store["steps/valid"] = np.array(valid, dtype=np.uint8)
    store["steps/step_count"] = np.array(q.step_count)

    # ---- episode summaries over recorded per-step sequences
    rng = np.random.default_rng(31)
    lengths = (0, 1, 4, 9)
    for e, L in enumerate(lengths):
        seq = rng.standard_normal((L, len(METRICS))).astype(np.float32)
        seq[:, METRICS.index("clip_rate")] = (rng.random(L) < 0.4).astype(np.float32)
        seq[:, METRICS.index("td_error")] = np.abs(seq[:, METRICS.index("td_error")])
        reward = np.float32(rng.standard_normal() * 40)
        steps = [{k: torch.tensor(seq[s, j]) for j, k in enumerate(METRICS)} for s in range(L)]
        out = stab.summarize_episode_stability_metrics(episode_reward=torch.tensor(reward), step_metrics=steps)
        store[f"episode/e{e}/steps"] = seq.reshape(L, len(METRICS))
        store[f"episode/e{e}/reward"] = np.array(reward)
        store[f"episode/e{e}/out"] = np.array([float(out[k]) for k in EPISODE], dtype=np.float64)
    store["episode/count"] = np.array(len(lengths))

    # ---- final metrics over recorded episode sequences
    for c, E in enumerate((0, 1, 2, 7)):
        ep = rng.standard_normal((E, len(EPISODE))).astype(np.float32)
        ep[:, EPISODE.index("reward")] *= 50
        ep[:, EPISODE.index("clip_rate")] = rng.random(E).astype(np.float32)
        cols = {k: [torch.tensor(ep[i, j]) for i in range(E)] for j, k in enumerate(EPISODE)}
        f = stab.calculate_final_stability_metrics(epoch_rewards=cols["reward"], epoch_q_means=cols["q_mean"], epoch_q_mins=cols["q_min"],
                                                   epoch_q_maxs=cols["q_max"], epoch_td_errors=cols["td_error"],
                                                   epoch_clip_rates=cols["clip_rate"], elapsed_seconds=12.5 + c)
        store[f"final/c{c}/episodes"] = ep.reshape(E, len(EPISODE))
        store[f"final/c{c}/elapsed"] = np.array(12.5 + c)
        store[f"final/c{c}/out"] = np.array(_flat_final(f), dtype=np.float64)
        trend = stab.calculate_td_error_trend(cols["td_error"])
        store[f"final/c{c}/trend"] = np.array(float(trend))
    store["final/count"] = np.array(4)
    out = HERE / "stability.npz"
    np.savez_compressed(out, **store)
    print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
