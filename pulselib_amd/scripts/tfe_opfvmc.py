"""On-policy first-visit Monte-Carlo control on 2048 with the whole loop on the device (agents/tfe_on_policy_mc_gpu.py): every
round is a roll-out launch of `--tables` whole games against the table's policy and a learn launch into that table.  Defaults:
GAMMA 0.9, EPSILON 0.1, NUM_EPISODES 1,000,000 on a 3 x 3 board (the reference's scripts/TFE/mctrain.py with
config/on_policy_first_visit_monte_carlo.yaml, which `--config PATH` reads as it is).  Per logging interval it prints what
mctrain.py:54 prints: the average episode reward, the final score and the steps per second -- here of the rounds since the last
line, each line costing one synchronisation.  `--symmetric` keeps a board's eight images under the symmetries of the square as one
state; `--eval-every K --eval-games M` prints, every K rounds, the scores of M games under the greedy policy
of the table as it stands (one evaluation launch, no trajectory; the same boards at every check).  `--grow-at LOAD` doubles the table
at a printed line while it holds LOAD x capacity states or more, or once after first visits were dropped since the last line (the
line then also prints the occupancy); `--save PATH` writes the table and the run's state at the end, `--resume PATH` continues such
a run for `--rounds` more rounds.  `--afterstate` learns the value of the board after the move instead of
Q(state, action); it works with all of the above, and `--resume` refuses a checkpoint of the other kind."""
from __future__ import annotations

import argparse
import time

import torch

from ..agents import OnPolicyFirstVisitMCTFEGPU


def run(device, rounds, tables=65536, board=3, gamma=0.9, epsilon=0.1, seed=0, capacity=None, max_steps=1024, log_every=1, out=print,
        symmetric=False, eval_every=0, eval_games=None, grow_at=0.0, save=None, resume=None, afterstate=False):
    if resume:                                                              # capacity None: what load() takes for the saved rows
        agent = OnPolicyFirstVisitMCTFEGPU.load(resume, device, capacity=capacity, afterstate=afterstate)
        want = dict(n_games=tables, n=board, gamma=float(gamma), epsilon=float(epsilon), max_steps=max_steps, seed=seed, symmetric=bool(symmetric))
        differ = {k: (getattr(agent, k), v) for k, v in want.items() if getattr(agent, k) != v}
        if differ:
            raise ValueError(f"{resume} continues another run: (saved, asked) {differ}")
    else:
        agent = OnPolicyFirstVisitMCTFEGPU(device, tables, board_size=board, gamma=gamma, epsilon=epsilon, capacity=capacity or 1 << 22,
                                           max_steps=max_steps, seed=seed, symmetric=symmetric, afterstate=afterstate)
    first, dropped_before = agent.round, 0
    steps_before, t0 = 0, time.perf_counter()
    for r in range(first, first + rounds):
        agent.learn_batch()
        if (r + 1 - first) % log_every == 0 or r + 1 == first + rounds:
            reward = agent.episode_reward.double().mean().item()            # (synchronises)
            score, best = agent.total_score.double().mean().item(), int(agent.total_score.max().item())
            st, now = agent.stats(), time.perf_counter()
            line = (f"Round {r}: episodes {(r + 1) * tables}, Avg episode reward: {reward:.2f}, Avg final score: {score:.2f}, Highest: {best}, "
                    f"Steps/sec: {(st['steps'] - steps_before) / (now - t0):.0f}, dropped {st['dropped']}, truncated {st['truncated']}")
            if grow_at:                                                     # (this line has synchronised already)
                occupancy, slots, lost = agent.occupancy(), agent.capacity, st["dropped"] > dropped_before
                while lost or occupancy >= grow_at * agent.capacity:
                    agent.grow(2 * agent.capacity)
                    lost = False
                line += f", occupancy {occupancy} of {slots}" + (f", grown to {agent.capacity}" if agent.capacity != slots else "")
                dropped_before = st["dropped"]
            out(line)
            steps_before, t0 = st["steps"], time.perf_counter() if grow_at else now
        if eval_every and (r + 1) % eval_every == 0:
            e = agent.evaluate(n_games=eval_games)                          # (synchronises)
            out(f"Round {r}: greedy policy over {e['games']} games: Avg final score: {e['mean_score']:.2f} +- {e['std_score'] / e['games'] ** .5:.2f}, "
                f"Highest: {e['max_score']}, Avg length: {e['mean_length']:.1f}, truncated {e['truncated']}, moves with a table entry: "
                f"{100 * e['coverage']:.1f} %, largest tile 2^k: {e['max_tile_hist']}")
    if save:
        agent.save(save)
    return agent


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", help="a YAML file with GAMMA, EPSILON and NUM_EPISODES (the reference's own file can be passed)")
    ap.add_argument("--tables", type=int, default=65536, help="games per round (one policy improvement per round)")
    ap.add_argument("--board", type=int, default=3, help="board side, 2..4")
    ap.add_argument("--rounds", type=int, help="default: NUM_EPISODES / tables, rounded up")
    ap.add_argument("--capacity", type=int, help="table slots, a power of two (128 bytes each); default 2^22, with --resume the smallest "
                                                 "power of two that is at least four times the saved states and 2^12")
    ap.add_argument("--max-steps", type=int, default=1024)
    ap.add_argument("--log-every", type=int, default=1, help="rounds per printed line")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--symmetric", action="store_true", help="one state per board up to rotation and reflection")
    ap.add_argument("--afterstate", action="store_true", help="learn V(board after the move) instead of Q(state, action)")
    ap.add_argument("--eval-every", type=int, default=0, help="rounds between evaluations of the greedy policy (0: never)")
    ap.add_argument("--eval-games", type=int, help="games per evaluation (default: --tables)")
    ap.add_argument("--grow-at", type=float, default=0.0, metavar="LOAD",
                    help="double the table at a printed line while occupancy >= LOAD * capacity, or after drops since the last line (0: never)")
    ap.add_argument("--save", metavar="PATH", help="write the table and the run's state to this .npz at the end")
    ap.add_argument("--resume", metavar="PATH", help="continue the run saved there (the same --tables, --board, --max-steps, --seed, --symmetric, --afterstate) for --rounds more rounds")
    args = ap.parse_args(argv)
    gamma, epsilon, episodes = 0.9, 0.1, 1_000_000
    if args.config:
        import yaml
        with open(args.config) as fh:
            cfg = yaml.safe_load(fh)
        gamma, epsilon, episodes = float(cfg.get("GAMMA", gamma)), float(cfg.get("EPSILON", epsilon)), int(cfg.get("NUM_EPISODES", episodes))
    rounds = args.rounds if args.rounds is not None else max(1, -(-episodes // args.tables))
    agent = run(torch.device("cuda"), rounds, args.tables, args.board, gamma, epsilon, args.seed, args.capacity, args.max_steps, args.log_every,
                symmetric=args.symmetric, eval_every=args.eval_every, eval_games=args.eval_games, grow_at=args.grow_at, save=args.save, resume=args.resume,
                afterstate=args.afterstate)
    print(f"{agent.round * args.tables} games in {agent.round} rounds, gamma {gamma}, epsilon {epsilon}: {len(agent.table())} states stored")


if __name__ == "__main__":
    main()
