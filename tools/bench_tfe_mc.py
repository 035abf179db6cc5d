"""Throughput of on-policy first-visit Monte-Carlo control on 3 x 3 2048 (csrc/tfe_mc.hip, agents/tfe_on_policy_mc_gpu.py), as ONE
JSON line per batch size B (65,536 and 1,048,576 games per round by default):
  cold    : the first timed round on an EMPTY table after one untimed round on a scratch agent of the same shape (code objects
            loaded): every lookup of the roll-out misses at its first slot, every first visit of the learner inserts.
  warm    : --repeats R (5) further rounds after --warmup W (3) untimed ones: the table holds the states of the earlier rounds.
            Median and (min, max) of the roll-out and of the learn launch, each between its own pair of HIP events, and of the
            round (roll-out + learn); episodes/s and board-steps/s from the round's median and the moves the stats words count.
  host    : the path it replaces, on the code of the parent commit: --host-games G (1,024) of the same games stepped through
            TFEBatch.step, every board copied to the host every step, the reference's OnPolicyFirstVisitMC choosing per board and
            learning per game.  Wall clock around a loop that synchronises itself.  A rate (board-steps/s): the number to beat.
  evaluate: the evaluation launch (pulse_tfe_mc_evaluate, epsilon 0, B games, no trajectory) on the table the warm rounds left, --repeats
            times between its own pair of HIP events after one untimed call: median and (min, max), games/s and board-steps/s from the
            moves the launch counts.  (A greedy game that repeats a move which changes nothing on a full board runs to max_steps.)
--symmetric runs everything on the table of canonical states (pulse_tfe_mc_rollout_canon).
max_steps is 256 here (the longest game met while learning for 12 rounds of 4,096 games was 222 moves; cut games are counted in
the line): the per-move buffers are B x max_steps x 9 bytes.  Nothing is asserted about the rates."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed_round(agent, torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    agent.rollout()
    ev[1].record()
    agent.learn()
    ev[2].record()
    agent.round += 1
    ev[2].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3, ev[1].elapsed_time(ev[2]) * 1e-3


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _timed_evaluate(agent, torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    agent.eval_counters(clear=True)
    ev[0].record()
    agent.evaluate_launch()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3, agent.eval_counters()


def device_rounds(dev, games, warmup, repeats, max_steps, capacity, symmetric=False):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    kw = dict(board_size=3, gamma=.9, epsilon=.1, capacity=capacity, max_steps=max_steps, seed=0, symmetric=symmetric)
    OnPolicyFirstVisitMCTFEGPU(dev, games, **kw).learn_batch()              # untimed: code objects, allocator
    torch.cuda.synchronize()
    agent = OnPolicyFirstVisitMCTFEGPU(dev, games, **kw)
    cold = _timed_round(agent, torch)
    cold_steps = agent.stats()["steps"]
    for _ in range(warmup):
        agent.learn_batch()
    before = agent.stats()
    times = [_timed_round(agent, torch) for _ in range(repeats)]
    after = agent.stats()
    steps = (after["steps"] - before["steps"]) / repeats
    rnd = _spread([a + b for a, b in times])
    states, mean_final_score = int((agent.entries[:, 0] != 0).sum().item()), agent.total_score.double().mean().item()
    agent.evaluate()                                                        # untimed: the evaluation kernel's code object
    evals = [_timed_evaluate(agent, torch) for _ in range(repeats)]
    ev_s, e = _spread([s for s, _ in evals]), evals[-1][1]
    return {"games": games, "board": 3, "symmetric": symmetric, "max_steps": max_steps, "capacity": capacity, "warmup": warmup, "repeats": repeats,
            "cold": {"rollout_s": cold[0], "learn_s": cold[1], "steps": cold_steps, "episodes_per_s": games / sum(cold),
                     "board_steps_per_s": cold_steps / sum(cold)},
            "warm": {"rollout_s": _spread([a for a, _ in times]), "learn_s": _spread([b for _, b in times]), "round_s": rnd,
                     "steps_per_round": steps, "episodes_per_s": games / rnd["median"], "board_steps_per_s": steps / rnd["median"]},
            "evaluate": {"seconds": ev_s, "moves": e["moves"], "games_per_s": games / ev_s["median"], "board_steps_per_s": e["moves"] / ev_s["median"],
                         "mean_score": e["mean_score"], "std_score": e["std_score"], "mean_length": e["mean_length"], "truncated": e["truncated"],
                         "coverage": e["coverage"]},
            "states_stored": states, "dropped": after["dropped"], "truncated": after["truncated"], "mean_final_score": mean_final_score}


def host_rounds(dev, games, rounds=2):
    """The interpreter's loop: one TFEBatch.step per move, a host copy of every board, a Python dict per game."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    from pulselib_amd.environments.TFE.TFE import TFEBatch
    random.seed(0)
    agent = OnPolicyFirstVisitMC(.9, .1, n_actions=4)
    steps, seconds = 0, 0.0
    for r in range(rounds + 1):                                             # round 0: untimed
        env = TFEBatch(dev, games, 3, seed=0, board_id0=r * games)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        boards, _ = env.reset()
        states = [tuple(b) for b in boards.cpu().numpy().reshape(games, 9).tolist()]
        episodes, live, n = [[] for _ in range(games)], list(range(games)), 0
        while live:
            actions = [0] * games
            for g in live:
                actions[g] = agent.action(states[g])
            boards, rewards, dones, _, _ = env.step(torch.tensor(actions, dtype=torch.int64))
            nxt, rew, done = boards.cpu().numpy().reshape(games, 9).tolist(), rewards.cpu().tolist(), dones.cpu().tolist()
            for g in live:
                episodes[g].append((states[g], actions[g], rew[g]))
                states[g] = tuple(nxt[g])
            n += len(live)
            live = [g for g in live if not done[g]]
        for ep in episodes:
            agent.learn(ep)
        if r:
            steps, seconds = steps + n, seconds + time.perf_counter() - t0
    return {"host_games": games, "rounds": rounds, "seconds": seconds, "episodes_per_s": games * rounds / seconds, "board_steps_per_s": steps / seconds}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=256)
    ap.add_argument("--host-games", type=int, default=1024, help="0: skip the host path")
    ap.add_argument("--symmetric", action="store_true", help="the table of canonical states")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfe_mc needs the MI355X: no timing is taken on a CPU")
    dev = torch.device("cuda:0")
    for games in args.games:
        # 128 slots per game, 2^25 (4 GB) at the most: a first round of 4,096 games stores ~19 states per game, later ones fewer; `dropped` tells if it was too few
        capacity = 1 << max(16, (games * 128 - 1).bit_length())
        print(json.dumps(device_rounds(dev, games, args.warmup, args.repeats, args.max_steps, min(capacity, 1 << 25), args.symmetric)), flush=True)
    if args.host_games:
        print(json.dumps(host_rounds(dev, args.host_games)), flush=True)


if __name__ == "__main__":
    main()
