"""The training-stability benchmark (the reference's scripts/Poker/trainGPU_stability.py) on the fused trainer loop:
reward standard deviation over episodes, the slope of the mean |TD error| across episodes, the gradient-clip rate and the
bounds of Q(s, a), measured inside the native learner's launches (utils/stability.py) instead of through a boolean-indexed
autograd update per step.  The reference's TrainingLogger files are not written (like the other output services).

    python -m pulselib_amd.scripts.trainGPU_stability [--tables N] [--episodes E]"""
from __future__ import annotations

import argparse

import torch

STABILITY_BENCHMARK_DEFAULTS = {
    "NUM_PLAYERS": 9,
    "N_GAMES": 100000,
    "EPISODES": 50,
    "STARTING_BBS": 100,
    "POKER_ACTION_SPACE_N": 13,
    "STATE_SPACE": 40,
    "ACTION_SPACE": 13,
    "GAMMA": 0.95,
    "UPDATE_FREQ": 20,
    "LEARNING_RATE": 2e-4,
    "WEIGHT_DECAY": 1e-5,
    "W1": 0.5,
    "W2": 0.3,
    "K": 100,
    "ALPHA": 50,
    "AGENT_STRINGS": ["tight_aggressive", "heuristic_hands", "heuristic_hands", "loose_passive", "tight_aggressive", "random",
                      "loose_passive", "small_ball", "tight_aggressive"],
    # keys of this engine (pulselib_amd/utils/config.py: POKER_GPU_ENGINE_KEYS)
    "SEED": 20260401,
    "MAX_EPISODE_STEPS": 200,
}


def format_final_block(final: dict) -> str:
    """The reference's closing block, from calculate_final_stability_metrics' dict."""
    bar = "=" * 50
    qb = final["q_bounds"]
    return "\n".join([
        "", bar, "FINAL STABILITY METRICS:", bar,
        f"Reward Std Dev (Stability): {float(final['reward_std']):.2f}",
        f"TD Error Trend (slope):     {float(final['td_error_trend']):.6f} (negative is better)",
        f"Average Gradient Clip Rate: {float(final['average_clip_rate']):.4f}",
        f"Q-Value Bounds:             [{float(qb['global_min']):.2f}, {float(qb['global_max']):.2f}]",
        f"Mean Q-Value:               {float(qb['mean_q']):.4f}",
        f"Total Run Time:             {float(final['total_time_seconds']):.2f}s",
        bar])


def run_stability_benchmark(config_overrides: dict | None = None) -> dict:
    """Runs the benchmark on cuda (train_agent_fused with a StabilityMetrics side channel) and returns the reference's final
    dict of 0-d tensors: reward_std, mean_reward, q_bounds{global_min, global_max, mean_q}, td_error_trend,
    average_clip_rate, total_time_seconds.  Prints the episode line every 5th episode and the final block, as the reference."""
    from ..environments.Poker import PokerGPU, PokerQNetwork, load_gpu_agents
    from ..environments.Poker.utils import PokerAgentType
    from ..utils.stability import StabilityMetrics
    from .trainGPU import train_agent_fused
    config = dict(STABILITY_BENCHMARK_DEFAULTS)
    if config_overrides is not None:
        config.update(config_overrides)
    if not torch.cuda.is_available():
        raise RuntimeError("run_stability_benchmark: the fused trainer runs on the MI355X only (no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device())
    seed, n_games, episodes = int(config["SEED"]), int(config["N_GAMES"]), int(config["EPISODES"])
    agents, agent_types = load_gpu_agents(device, config["NUM_PLAYERS"], config["AGENT_STRINGS"], config["STARTING_BBS"],
                                          config["POKER_ACTION_SPACE_N"])
    q_net = PokerQNetwork(weights_path="", device=device, gamma=config["GAMMA"], update_freq=config["UPDATE_FREQ"],
                          state_dim=config["STATE_SPACE"], action_dim=config["ACTION_SPACE"], learning_rate=config["LEARNING_RATE"],
                          weight_decay=config["WEIGHT_DECAY"], epsilon=0.5, epsilon_decay=0.95, epsilon_end=0.05, seed=seed)
    agents.insert(0, q_net)
    agent_types.insert(0, PokerAgentType.QLEARNING)
    n_players = int(config["NUM_PLAYERS"]) + 1
    env = PokerGPU(device=device, agents=agents, n_players=n_players, max_players=max(10, n_players), n_games=n_games,
                   starting_bbs=config["STARTING_BBS"], w1=config["W1"], w2=config["W2"], K=config["K"], alpha=config["ALPHA"], seed=seed)
    metrics = StabilityMetrics(q_net)
    out = train_agent_fused(env, agents, agent_types, episodes, n_games, device, reduce_stats=False,
                            max_episode_steps=config["MAX_EPISODE_STEPS"], stability_metrics=metrics)
    for e, ep in enumerate(out["stability"]["episodes"], start=1):
        if e % 5 == 0:
            print(f"Episode {e:2d}/{episodes} | Reward: {ep['reward']:8.2f} | TD Error: {ep['td_error']:6.4f} | "
                  f"Clip Rate: {ep['clip_rate']:4.2f}")
    final = metrics.summary(out["total_training_seconds"])
    print(format_final_block(final))
    return final


def main(argv=None):
    ap = argparse.ArgumentParser(description="training-stability benchmark of the Poker learner (native metrics)")
    ap.add_argument("--tables", type=int, default=None, help="override N_GAMES")
    ap.add_argument("--episodes", type=int, default=None, help="override EPISODES")
    args = ap.parse_args(argv)
    overrides = {}
    if args.tables is not None:
        overrides["N_GAMES"] = args.tables
    if args.episodes is not None:
        overrides["EPISODES"] = args.episodes
    return run_stability_benchmark(overrides)


if __name__ == "__main__":
    main()
