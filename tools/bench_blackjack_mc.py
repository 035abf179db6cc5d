"""Throughput of first-visit Monte-Carlo learning on Blackjack, three ways, as ONE JSON line:
  (a) device_learner : scripts/blackjack_fvmc.run_device at 1,048,576 games x 16 episodes per launch -- shuffle, play and count in
      one launch (csrc/blackjack_mc.hip).  HIP events around >= 1 s of back-to-back launches, the first launch excluded, one
      synchronisation at the end.
  (b) host_learner   : the path it replaces, scripts/blackjack_fvmc.run(batches=5, batch_size=1000): env reset + steps with four
      .cpu() copies each, per-game episode lists and FirstVisitMonteCarlo.learn on the host.  Wall clock (it synchronises itself).
  (c) env_floor      : BlackJack.reset() + 12 step() launches at 1,048,576 games with a fixed action tensor and NO learner: what any
      env-stepped learner pays before it has learnt anything.  HIP events.
--device-only: (a) alone; --seconds S: the length of (a)'s timed run (1.0; shorter under a counter pass).
--control: instead, ONE JSON line on the Monte-Carlo control launches (csrc/blackjack_mc.hip, agents/on_policy_first_visit_mc_gpu.py)
at the same 1,048,576 games x 16 episodes per launch, in one process, HIP events around --launches L (200) back-to-back launches
after a warm-up, --repeats R (7) times, the three taking turns within every repeat:
  value_rollout   : pulse_blackjack_mc_rollout under the threshold-17 table -- the baseline, (a) above;
  control_rollout : pulse_blackjack_mc_control_rollout under the same table: the same games, 34 instead of 32 cells per state;
  control_train   : OnPolicyFirstVisitMCGPU.train -- roll-out under the agent's own epsilon-soft table + improve per batch.
control_rollout is accepted at median <= value_rollout's median x (1 + value_rollout's (max - min) / median + 0.05).
PULSE_LIB=<a twin from `make -C pulselib_amd/csrc bjmc-ablate ABL=n`> prices parts of (a)."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMES, EPISODES_PER_LAUNCH = 1 << 20, 16


def device_learner(dev, min_seconds=1.0):
    import torch
    from pulselib_amd.scripts.blackjack_fvmc import run_device
    kw = dict(batch_size=GAMES, gamma=0.9, seed=1, hit_below=17, episodes_per_launch=EPISODES_PER_LAUNCH)
    agent, _ = run_device(dev, batches=1, **kw)                    # the first launch (module load, policy upload): not timed
    torch.cuda.synchronize()
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    run_device(dev, batches=2, agent=agent, **kw)                  # sizes the timed run
    b.record()
    b.synchronize()
    per_launch = a.elapsed_time(b) * 1e-3 / 2
    launches = max(3, math.ceil(1.25 * min_seconds / per_launch))
    b.record()
    _, n = run_device(dev, batches=launches, agent=agent, **kw)
    c.record()
    torch.cuda.synchronize()                                       # the one synchronisation of the timed run
    seconds = b.elapsed_time(c) * 1e-3
    st = agent.stats()
    assert st["games"] == (launches + 3) * GAMES * EPISODES_PER_LAUNCH and st["capped"] == 0
    return {"episodes_per_sec": n / seconds, "ns_per_game": seconds / n * 1e9, "launches": launches, "seconds": seconds,
            "games_per_launch": GAMES, "episodes_per_launch": EPISODES_PER_LAUNCH, "us_per_launch": seconds / launches * 1e6,
            "actions_per_game": st["actions"] / st["games"], "states": len(agent.values)}


def host_learner(dev):
    import torch
    from pulselib_amd.scripts.blackjack_fvmc import run
    run(dev, batches=1, batch_size=1000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, n = run(dev, batches=5, batch_size=1000)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    return {"episodes_per_sec": n / seconds, "ns_per_game": seconds / n * 1e9, "seconds": seconds, "batches": 5, "batch_size": 1000}


def env_floor(dev, reps=20):
    import torch
    from pulselib_amd.environments.blackjack import BlackJack
    env = BlackJack(dev, GAMES, seed=1)
    hit, stand = torch.zeros(GAMES, dtype=torch.long, device=dev), torch.ones(GAMES, dtype=torch.long, device=dev)

    def episode():
        env.reset()
        for s in range(12):
            env.step(hit if s < 11 else stand)
    for _ in range(3):
        episode()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        episode()
    b.record()
    torch.cuda.synchronize()
    seconds = a.elapsed_time(b) * 1e-3
    n = reps * GAMES
    return {"episodes_per_sec": n / seconds, "ns_per_game": seconds / n * 1e9, "seconds": seconds, "episodes": reps, "games": GAMES,
            "launches_per_episode": 13}


def control(dev, launches=200, repeats=7):
    import statistics
    import torch
    from pulselib_amd.agents import FirstVisitMonteCarloGPU, OnPolicyFirstVisitMCGPU
    value = FirstVisitMonteCarloGPU(dev, 0.9, seed=1)
    rollout = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1, seed=1)
    train = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1, seed=1)
    table = value._table(value.threshold_policy(17))
    runs = {"value_rollout": lambda: value.learn_batch(GAMES, table, n_episodes=EPISODES_PER_LAUNCH),
            "control_rollout": lambda: rollout.learn_batch(GAMES, n_episodes=EPISODES_PER_LAUNCH, policy=table),
            "control_train": lambda: train.train(1, GAMES, EPISODES_PER_LAUNCH)}
    for fn in runs.values():                                       # module load, and a policy that has left the uniform start
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in runs}
    for _ in range(repeats):
        for name, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / launches)
    n = (3 + repeats * launches) * GAMES * EPISODES_PER_LAUNCH
    stats = {"value_rollout": value.stats(), "control_rollout": rollout.stats(), "control_train": train.stats()}
    assert all(st["games"] == n and st["capped"] == 0 for st in stats.values())
    assert stats["value_rollout"] == stats["control_rollout"]      # the same games under the same table
    out = {}
    for name, t in us.items():
        med = statistics.median(t)
        out[name] = {"us_per_launch": med, "min": min(t), "max": max(t), "spread": (max(t) - min(t)) / med, "repeats_us": t,
                     "ns_per_game": med * 1e3 / (GAMES * EPISODES_PER_LAUNCH), "episodes_per_sec": GAMES * EPISODES_PER_LAUNCH / (med * 1e-6),
                     "actions_per_game": stats[name]["actions"] / stats[name]["games"], "win_rate": stats[name]["wins"] / stats[name]["games"]}
    bound = out["value_rollout"]["us_per_launch"] * (1.0 + out["value_rollout"]["spread"] + 0.05)
    out.update(launches=launches, repeats=repeats, games_per_launch=GAMES, episodes_per_launch=EPISODES_PER_LAUNCH,
               control_over_value=out["control_rollout"]["us_per_launch"] / out["value_rollout"]["us_per_launch"],
               train_over_value=out["control_train"]["us_per_launch"] / out["value_rollout"]["us_per_launch"],
               bound_us=bound, control_within_bound=out["control_rollout"]["us_per_launch"] <= bound)
    return out


def main():
    import torch
    dev = torch.device("cuda", 0)
    if "--control" in sys.argv:
        arg = lambda flag, default: int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default
        out = {"name": "blackjack_mc_control", "device": torch.cuda.get_device_name(0), "lib": os.environ.get("PULSE_LIB", "libpulse_hip.so")}
        out.update(control(dev, max(20, arg("--launches", 200)), max(5, arg("--repeats", 7))))
        print(json.dumps(out), flush=True)
        return
    out = {"name": "blackjack_first_visit_mc", "device": torch.cuda.get_device_name(0), "lib": os.environ.get("PULSE_LIB", "libpulse_hip.so")}
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 1.0      # (short runs: under a counter pass)
    out["device_learner"] = device_learner(dev, seconds)
    if "--device-only" not in sys.argv:
        out["host_learner"] = host_learner(dev)
        out["env_floor"] = env_floor(dev)
        out["device_over_host"] = out["device_learner"]["episodes_per_sec"] / out["host_learner"]["episodes_per_sec"]
        out["device_ns_per_game_over_env_floor"] = out["device_learner"]["ns_per_game"] / out["env_floor"]["ns_per_game"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
