"""Training-stability metrics of the Q-network learner (the reference's utils/stability.py, used by its
scripts/Poker/trainGPU_stability.py) without per-step host syncs on the GPU.

The reference measures every update through boolean indexing and autograd (a host sync per mask) and reduces the per-row
TD errors and Q(s, a) values with torch.  Here the training launches of csrc/qnet.hip total them per workgroup next to the
loss terms they already compute, and the reduce / AdamW launch writes the per-call block and adds it to a per-episode
accumulator on the device (`PokerQNetwork.enable_stability_metrics`; include/pulse_env.h: PulseQNetTrain.stability).
`StabilityMetrics` reads the accumulator back once per episode, as `HandMetrics` (utils/performance.py) does its sums.

Function names, arguments and return keys follow the reference's utils/stability.py; the aggregations are the same
formulas (episode values are means over measured steps of the per-step means, q_min / q_max the min / max over steps)."""
from __future__ import annotations

from typing import Any

import torch

METRIC_KEYS = ("loss", "td_error", "grad_norm", "clip_rate", "q_mean", "q_min", "q_max")
EPISODE_KEYS = ("reward", "q_mean", "q_min", "q_max", "td_error", "clip_rate")
# PulseQNetTrain.stability: the per-call block [0..7] ...
STEP_ROWS, STEP_TD, STEP_QMEAN, STEP_QMIN, STEP_QMAX, STEP_NORM, STEP_CLIPPED, STEP_LOSS = range(8)
# ... and the per-episode accumulator [8..15], counted from its start
ACC_STEPS, ACC_TD, ACC_QMEAN, ACC_QMIN, ACC_QMAX, ACC_CLIPPED, ACC_LOSS = range(7)


def build_valid_q_learning_batch(states, actions, rewards, next_states, dones):
    """The rows whose seat status (column 12) is ACTIVE or ALLIN, or None when there is none (one host sync)."""
    status = states[:, 12]
    keep = (status == 0) | (status == 2)
    if not bool(keep.any()):
        return None
    return tuple(x[keep] for x in (states, actions, rewards, next_states, dones))


def calculate_q_learning_targets(q_network, rewards, next_states, dones):
    """r + gamma * max_a' Q_target(s', a') * (1 - done), without autograd."""
    with torch.no_grad():
        best_next = q_network.target_network(next_states).max(dim=1).values
        return rewards + q_network.gamma * best_next * (~dones).float()


def calculate_q_value_summary(q_values_for_actions):
    return {"q_mean": q_values_for_actions.mean(), "q_min": q_values_for_actions.min(), "q_max": q_values_for_actions.max()}


def calculate_td_error(q_values_for_actions, targets):
    """mean |Q(s, a) - target|"""
    return (q_values_for_actions - targets).abs().mean()


def calculate_gradient_clip_rate(total_grad_norm, clip_threshold: float = 1.0):
    """1.0 where the norm before clipping exceeds the threshold, else 0.0 (the norm's dtype and device)."""
    return (total_grad_norm > clip_threshold).to(total_grad_norm.dtype)


def _runs_native(q_network, states) -> bool:
    return getattr(q_network, "_flat", None) is not None and hasattr(q_network, "enable_stability_metrics") and states.is_cuda


def _torch_step(q_network, states, actions, rewards, next_states, dones, clip_threshold):
    batch = build_valid_q_learning_batch(states, actions, rewards, next_states, dones)
    if batch is None:
        return None
    s, a, r, ns, d = batch
    q_taken = q_network(s).gather(1, a.unsqueeze(1)).squeeze(1)
    targets = calculate_q_learning_targets(q_network, r, ns, d)
    loss = q_network.criterion(q_taken, targets)
    q_network.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(q_network.parameters(), max_norm=clip_threshold)
    q_network.optimizer.step()
    q_network.step_count += 1
    if q_network.step_count % q_network.update_freq == 0:
        q_network.target_network.load_state_dict(q_network.network.state_dict())
    q_taken = q_taken.detach()
    out = {"loss": loss.detach(), "td_error": calculate_td_error(q_taken, targets), "grad_norm": norm,
           "clip_rate": calculate_gradient_clip_rate(norm, clip_threshold)}
    out.update(calculate_q_value_summary(q_taken))
    return out


def _native_step(q_network, states, actions, rewards, next_states, dones, clip_threshold):
    # like the reference (and PokerQNetwork.train_step): one host sync to learn whether any row is valid; nothing is launched if not
    if states.shape[0] == 0 or not bool(((states[:, 12] == 0) | (states[:, 12] == 2)).any()):
        return None
    q_network.enable_stability_metrics()
    kept = q_network.max_grad_norm
    q_network.max_grad_norm = float(clip_threshold)
    try:
        q_network.train_step_native(states, actions, rewards, next_states, dones, None)
    finally:
        q_network.max_grad_norm = kept
    block = q_network.stability_step().clone()          # the next call overwrites the per-call block: keep this one's
    return {"loss": block[STEP_LOSS], "td_error": block[STEP_TD], "grad_norm": block[STEP_NORM], "clip_rate": block[STEP_CLIPPED],
            "q_mean": block[STEP_QMEAN], "q_min": block[STEP_QMIN], "q_max": block[STEP_QMAX]}


def run_stability_measured_q_learning_step(q_network: Any, states, actions, rewards, next_states, dones, *,
                                           clip_threshold: float = 1.0) -> dict | None:
    """One measured update.  On a PokerQNetwork of a GPU: the native update (csrc/qnet.hip) with the metrics taken inside
    its launches -> a dict of 0-d device tensors {loss, td_error, grad_norm, clip_rate, q_mean, q_min, q_max}, or None when
    no row is valid.  Q(s, a) is the train-mode (dropout) value the update differentiates.  On a CPU module: the same
    update on torch autograd."""
    if _runs_native(q_network, states):
        return _native_step(q_network, states, actions, rewards, next_states, dones, clip_threshold)
    return _torch_step(q_network, states, actions, rewards, next_states, dones, clip_threshold)


def stack_metric_values(step_metrics: list, key: str):
    return torch.stack([m[key] for m in step_metrics])


def summarize_episode_stability_metrics(episode_reward, step_metrics: list) -> dict:
    """Per episode: the reward, the mean over measured steps of the step means (q_mean, td_error, clip_rate) and the
    min / max over steps of the step min / max.  No measured step: every metric 0."""
    reward = episode_reward.detach()
    if not step_metrics:
        zero = torch.zeros((), dtype=reward.dtype, device=reward.device)
        return {"reward": reward, "q_mean": zero, "q_min": zero, "q_max": zero, "td_error": zero, "clip_rate": zero}
    return {"reward": reward,
            "q_mean": stack_metric_values(step_metrics, "q_mean").mean(),
            "q_min": stack_metric_values(step_metrics, "q_min").min(),
            "q_max": stack_metric_values(step_metrics, "q_max").max(),
            "td_error": stack_metric_values(step_metrics, "td_error").mean(),
            "clip_rate": stack_metric_values(step_metrics, "clip_rate").mean()}


def calculate_td_error_trend(td_errors: list):
    """Least-squares slope of the episodes' TD errors against the episode index (0 for fewer than two episodes)."""
    if len(td_errors) < 2:
        return torch.zeros((), dtype=td_errors[0].dtype, device=td_errors[0].device) if td_errors else torch.zeros(())
    y = torch.stack(list(td_errors))
    x = torch.arange(y.numel(), dtype=y.dtype, device=y.device)
    dx, dy = x - x.mean(), y - y.mean()
    return (dx * dy).sum() / (dx * dx).sum().clamp_min(torch.finfo(y.dtype).eps)


def resolve_metric_device(*metric_lists):
    for values in metric_lists:
        if values:
            return values[0].device
    return torch.device("cpu")


def calculate_final_stability_metrics(*, epoch_rewards: list, epoch_q_means: list, epoch_q_mins: list, epoch_q_maxs: list,
                                      epoch_td_errors: list, epoch_clip_rates: list, elapsed_seconds: float) -> dict:
    """The run's summary: population std and mean of the episode rewards, Q bounds (min / max over episodes, mean of
    the episode means), TD-error trend, mean clip rate, elapsed time.  No episode: every value 0."""
    device = resolve_metric_device(epoch_rewards, epoch_q_means, epoch_q_mins, epoch_q_maxs, epoch_td_errors, epoch_clip_rates)
    elapsed = torch.tensor(elapsed_seconds, device=device)

    def zero():
        return torch.zeros((), device=device)

    def over(values, reduce):
        return reduce(torch.stack(list(values))) if values else zero()
    if not epoch_rewards:
        return {"reward_std": zero(), "mean_reward": zero(),
                "q_bounds": {"global_min": zero(), "global_max": zero(), "mean_q": zero()},
                "td_error_trend": zero(), "average_clip_rate": zero(), "total_time_seconds": elapsed}
    rewards = torch.stack(list(epoch_rewards))
    return {"reward_std": rewards.std(unbiased=False), "mean_reward": rewards.mean(),
            "q_bounds": {"global_min": over(epoch_q_mins, torch.min), "global_max": over(epoch_q_maxs, torch.max),
                         "mean_q": over(epoch_q_means, torch.mean)},
            "td_error_trend": calculate_td_error_trend(epoch_td_errors),
            "average_clip_rate": over(epoch_clip_rates, torch.mean), "total_time_seconds": elapsed}


def metric_values(d: dict) -> dict:
    """A (nested) metrics dict with every tensor as a Python float."""
    return {k: metric_values(v) if isinstance(v, dict) else (float(v) if torch.is_tensor(v) else v) for k, v in d.items()}


def episode_from_accumulator(reward: float, acc) -> dict:
    """The episode summary from the values of the device accumulator (PulseQNetTrain.stability[8..15], on the host): the
    numbers summarize_episode_stability_metrics gives over the episode's per-step dicts."""
    steps = float(acc[ACC_STEPS])
    if steps <= 0.0:
        return {"reward": float(reward), "q_mean": 0.0, "q_min": 0.0, "q_max": 0.0, "td_error": 0.0, "clip_rate": 0.0}
    return {"reward": float(reward), "q_mean": float(acc[ACC_QMEAN]) / steps, "q_min": float(acc[ACC_QMIN]),
            "q_max": float(acc[ACC_QMAX]), "td_error": float(acc[ACC_TD]) / steps, "clip_rate": float(acc[ACC_CLIPPED]) / steps}


class StabilityMetrics:
    """The stability side channel of train_agent_fused, shaped like utils.performance.HandMetrics: `begin_episode()`
    clears the learner's device accumulator, the native updates add to it inside their own launches, `end_episode(reward)`
    reads it back once and returns the episode's summary (plain floats, the keys of summarize_episode_stability_metrics),
    `summary(elapsed)` the run's (calculate_final_stability_metrics: 0-d tensors)."""

    def __init__(self, q_net):
        self.q_net = q_net
        q_net.enable_stability_metrics()
        self.episodes = []
        self.measured_steps = []

    def begin_episode(self) -> None:
        self.q_net.clear_stability_metrics()

    def end_episode(self, episode_reward) -> dict:
        acc = self.q_net.stability_episode()
        reward = episode_reward.detach().reshape(1).to(device=acc.device, dtype=torch.float64)
        host = torch.cat([reward, acc.to(torch.float64)]).cpu().tolist()         # the one read-back of the episode
        ep = episode_from_accumulator(host[0], host[1:])
        self.episodes.append(ep)
        self.measured_steps.append(int(host[1 + ACC_STEPS]))
        return ep

    def summary(self, elapsed_seconds: float) -> dict:
        col = {k: [torch.tensor(e[k], dtype=torch.float32) for e in self.episodes] for k in EPISODE_KEYS}
        return calculate_final_stability_metrics(epoch_rewards=col["reward"], epoch_q_means=col["q_mean"], epoch_q_mins=col["q_min"],
                                                 epoch_q_maxs=col["q_max"], epoch_td_errors=col["td_error"],
                                                 epoch_clip_rates=col["clip_rate"], elapsed_seconds=float(elapsed_seconds))
