"""On-policy first-visit Monte-Carlo control on Blackjack with the whole loop on the device
(agents/on_policy_first_visit_mc_gpu.py): every batch is a roll-out launch under the agent's epsilon-soft table and a
policy-improvement launch.  Defaults: GAMMA 0.9, EPSILON 0.1 (the reference's config/on_policy_first_visit_monte_carlo.yaml,
which `--config PATH` reads as it is: GAMMA, EPSILON, NUM_EPISODES).  Prints the greedy hit / stand table learnt for hard and
soft hands and the win rate of the games played while learning (the env counts a push as a win)."""
from __future__ import annotations

import argparse

import torch

from ..agents import OnPolicyFirstVisitMCGPU
from ..agents.on_policy_first_visit_mc_gpu import HIT


def run(device, batches=64, batch_size=65536, episodes_per_launch=1, gamma=0.9, epsilon=0.1, seed=1):
    agent = OnPolicyFirstVisitMCGPU(device, gamma, epsilon, seed=seed)
    agent.train(batches, batch_size, episodes_per_launch)
    return agent, batches * batch_size * episodes_per_launch


def table_text(greedy: dict) -> str:
    """Rows: the player's sum; columns: the dealer's upcard 2..11 (11 = ace); H / S, '.' = a state never visited."""
    lines = []
    for ace, title, sums in ((0, "hard", range(4, 22)), (1, "soft", range(12, 22))):
        lines.append(f"{title:>4} " + " ".join(f"{u:>2}" for u in range(2, 12)))
        for s in sums:
            row = [greedy.get((s, ace, u)) for u in range(2, 12)]
            lines.append(f"{s:>4} " + " ".join(" ." if a is None else (" H" if a == HIT else " S") for a in row))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", help="a YAML file with GAMMA, EPSILON and NUM_EPISODES (the reference's own file can be passed)")
    ap.add_argument("--batches", type=int, help="policy improvements (default 64, or NUM_EPISODES / (batch size x episodes per launch))")
    ap.add_argument("--batch-size", type=int, default=65536, help="games per episode of a launch")
    ap.add_argument("--episodes-per-launch", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    gamma, epsilon, batches = 0.9, 0.1, args.batches
    if args.config:
        import yaml
        with open(args.config) as fh:
            cfg = yaml.safe_load(fh)
        gamma, epsilon = float(cfg.get("GAMMA", gamma)), float(cfg.get("EPSILON", epsilon))
        if batches is None and "NUM_EPISODES" in cfg:
            per_batch = args.batch_size * args.episodes_per_launch
            batches = max(1, -(-int(cfg["NUM_EPISODES"]) // per_batch))
    agent, n = run(torch.device("cuda"), 64 if batches is None else batches, args.batch_size, args.episodes_per_launch, gamma, epsilon, args.seed)
    st = agent.stats()
    print(f"{n} games in {agent.round} batches, gamma {gamma}, epsilon {epsilon}: {len(agent.q) // 2} states visited")
    print(table_text(agent.greedy_policy()))
    print(f"win rate while learning: {st['wins'] / st['games']:.4f} ({st['capped']} games capped)")


if __name__ == "__main__":
    main()
