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
--table-ops times pulse_tfe_mc_table_merge instead, on the plain table that one cold and --warmup rounds of
--table-games G (65,536) games leave in 2^22 slots, each launch between its own pair of HIP events, --table-untimed U (3) untimed and
--repeats timed repetitions into a freshly zeroed destination: grow (the 2^22 slots into 2^23), fold (the 2^23 slots into a symmetric table of 2^23)
and load (the live rows as a dense array into 2^23).  Per launch: live entries, ms (median, min, max) and source bytes scanned per
second; and, measured in the same run on a 3 x 3 table, the host path the fold replaces: table(), then fold_table_on_host.  One
JSON line per launch, also appended to profiles/tfe_mc/bench_tfe_mc_table.jsonl.
--afterstate times the afterstate mode (pulse_tfe_mc_rollout_after, pulse_tfe_mc_learn_after,
pulse_tfe_mc_evaluate_after, pulse_tfe_mc_table_fold_after) BESIDE the default agent of the same run, shape and seeds: per batch size the
two agents' lines as above under "plain" and "afterstate", the fold of the afterstate table the warm rounds left into a zeroed table
of the same capacity, and per launch the time per move and its ratio to the plain agent's (afterstate games get longer as the policy
improves, so launches are compared per move).  One JSON line per batch size, also appended to profiles/tfe_mc/bench_tfe_mc_after.jsonl.
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


def device_rounds(dev, games, warmup, repeats, max_steps, capacity, symmetric=False, afterstate=False, keep_agent=False):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    kw = dict(board_size=3, gamma=.9, epsilon=.1, capacity=capacity, max_steps=max_steps, seed=0, symmetric=symmetric, afterstate=afterstate)
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
    line = {"games": games, "board": 3, "symmetric": symmetric, "afterstate": afterstate, "max_steps": max_steps, "capacity": capacity, "warmup": warmup, "repeats": repeats,
            "cold": {"rollout_s": cold[0], "learn_s": cold[1], "steps": cold_steps, "episodes_per_s": games / sum(cold),
                     "board_steps_per_s": cold_steps / sum(cold)},
            "warm": {"rollout_s": _spread([a for a, _ in times]), "learn_s": _spread([b for _, b in times]), "round_s": rnd,
                     "steps_per_round": steps, "episodes_per_s": games / rnd["median"], "board_steps_per_s": steps / rnd["median"]},
            "evaluate": {"seconds": ev_s, "moves": e["moves"], "games_per_s": games / ev_s["median"], "board_steps_per_s": e["moves"] / ev_s["median"],
                         "mean_score": e["mean_score"], "std_score": e["std_score"], "mean_length": e["mean_length"], "truncated": e["truncated"],
                         "coverage": e["coverage"]},
            "states_stored": states, "dropped": after["dropped"], "truncated": after["truncated"], "mean_final_score": mean_final_score}
    return (line, agent) if keep_agent else line


def after_rounds(dev, games, warmup, repeats, max_steps, capacity, symmetric, path):
    """The default agent and the afterstate agent, one after the other in this process, and the afterstate table's fold."""
    import torch
    plain = device_rounds(dev, games, warmup, repeats, max_steps, capacity, symmetric)
    torch.cuda.empty_cache()
    after, agent = device_rounds(dev, games, warmup, repeats, max_steps, capacity, symmetric, afterstate=True, keep_agent=True)
    out = {"games": games, "board": 3, "symmetric": symmetric, "max_steps": max_steps, "capacity": capacity, "plain": plain, "afterstate": after}
    if not symmetric:                                                       # (a table of canonical states has no fold)
        sym = agent._like(n_games=1, capacity=1, symmetric=True)            # its _merge_launch is the fold; its own table is not used
        times, st, _ = _timed_merge(sym, torch, agent.entries, capacity, True, 3, repeats)
        out["fold"] = {"seconds": _spread(times), "src_entries": capacity, **st, "src_bytes_per_s": capacity * 128 / statistics.median(times)}

    def per_move(line, launch):
        if launch == "evaluate":
            return line["evaluate"]["seconds"]["median"] / line["evaluate"]["moves"]
        if launch.startswith("cold"):
            return line["cold"][launch[5:] + "_s"] / line["cold"]["steps"]
        return line["warm"][launch + "_s"]["median"] / line["warm"]["steps_per_round"]
    out["per_move"] = {k: {"plain_ns": per_move(plain, k) * 1e9, "afterstate_ns": per_move(after, k) * 1e9, "ratio": per_move(after, k) / per_move(plain, k)}
                       for k in ("cold_rollout", "cold_learn", "rollout", "learn", "evaluate")}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as fh:
        fh.write(json.dumps(out) + "\n")


def _timed_merge(agent, torch, src, capacity, canonical, untimed=3, repeats=5):
    """(seconds per repetition, the counters of the last one): src merged into a zeroed table of `capacity` slots, every time a new one"""
    stats = torch.zeros(4, dtype=torch.int64, device=agent.device)
    dst = agent._new_table(capacity)
    times = []
    for i in range(untimed + repeats):
        dst.zero_()
        stats.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        agent._merge_launch(src, dst, canonical, stats)
        ev[1].record()
        ev[1].synchronize()
        if i >= untimed:
            times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return times, dict(zip(("live", "placed", "dropped"), stats.cpu().tolist())), dst


def table_ops(dev, games, warmup, untimed, repeats, max_steps, path):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import ENTRY_BYTES, fold_table_on_host
    agent = OnPolicyFirstVisitMCTFEGPU(dev, games, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 22, max_steps=max_steps, seed=0)
    for _ in range(1 + warmup):
        agent.learn_batch()
    dropped = agent.stats()["dropped"]
    os.makedirs(os.path.dirname(path), exist_ok=True)

    def emit(entry):
        print(json.dumps(entry), flush=True)
        with open(path, "a") as fh:
            fh.write(json.dumps(entry) + "\n")

    def line(op, src, times, st, **more):
        s = _spread(times)
        emit({"op": op, "board": 3, "games": games, "rounds": 1 + warmup, "untimed": untimed, "repeats": repeats, "src_entries": src.shape[0],
              "live": st["live"], "placed": st["placed"], "dropped": st["dropped"], "ms": {k: v * 1e3 for k, v in s.items()},
              "src_bytes_per_s": src.shape[0] * ENTRY_BYTES / s["median"], "learn_dropped": dropped, **more})

    times, st, grown = _timed_merge(agent, torch, agent.entries, 1 << 23, False, untimed, repeats)
    line("grow 2^22 -> 2^23", agent.entries, times, st, dst_capacity=1 << 23)
    times, st, sym = _timed_merge(agent, torch, grown, 1 << 23, True, untimed, repeats)
    line("fold 2^23 -> symmetric 2^23", grown, times, st, dst_capacity=1 << 23)
    folded = int((sym[:, 0] != 0).sum().item())                              # the canonical states the fold left: the host's count below
    live = grown[grown[:, 0] != 0]
    dense = agent._new_table(live.shape[0])                                  # (128-byte aligned)
    dense.copy_(live)
    del grown, sym, live
    times, st, _ = _timed_merge(agent, torch, dense, 1 << 23, False, untimed, repeats)
    line("load dense -> 2^23", dense, times, st, dst_capacity=1 << 23)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = agent.table()
    t1 = time.perf_counter()
    host = fold_table_on_host(table, 3)
    t2 = time.perf_counter()
    emit({"op": "host: table(), then fold_table_on_host", "board": 3, "games": games, "live": len(table), "canonical": len(host), "table_s": t1 - t0,
          "fold_s": t2 - t1, "canonical_states_on_device": folded})


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
    ap.add_argument("--afterstate", action="store_true", help="the afterstate mode beside the default agent (DESIGN.md section 12.3)")
    ap.add_argument("--after-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tfe_mc", "bench_tfe_mc_after.jsonl"))
    ap.add_argument("--table-ops", action="store_true", help="time the table-merge launch (grow, fold, dense load) instead of the rounds")
    ap.add_argument("--table-games", type=int, default=65536, help="games per round that fill the table for --table-ops")
    ap.add_argument("--table-untimed", type=int, default=3, help="untimed repetitions of each merge launch for --table-ops")
    ap.add_argument("--table-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tfe_mc", "bench_tfe_mc_table.jsonl"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfe_mc needs the MI355X: no timing is taken on a CPU")
    dev = torch.device("cuda:0")
    if args.table_ops:
        table_ops(dev, args.table_games, args.warmup, args.table_untimed, args.repeats, args.max_steps, args.table_out)
        return
    for games in args.games:
        # 128 slots per game, 2^25 (4 GB) at the most: a first round of 4,096 games stores ~19 states per game, later ones fewer; `dropped` tells if it was too few
        capacity = 1 << max(16, (games * 128 - 1).bit_length())
        if args.afterstate:
            after_rounds(dev, games, args.warmup, args.repeats, args.max_steps, min(capacity, 1 << 25), args.symmetric, args.after_out)
            continue
        print(json.dumps(device_rounds(dev, games, args.warmup, args.repeats, args.max_steps, min(capacity, 1 << 25), args.symmetric)), flush=True)
    if args.host_games and not args.afterstate:
        print(json.dumps(host_rounds(dev, args.host_games)), flush=True)


if __name__ == "__main__":
    main()
