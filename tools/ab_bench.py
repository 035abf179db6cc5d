"""A/B of kernel builds on ONE box (box-to-box variation is +-2 %, more than most kernel changes): runs bench.py's env-only
leg with each given side in turn, alternating, `--rounds` times (default 2), and prints kernel time / value per run and, at the
end, each side's median and min-max spread; stops at the first run that fails.
    python tools/ab_bench.py pulselib_amd/libpulse_hip.so /path/to/other.so [--rounds 5] [--tables N] [--active-players sampled|10] [--steps 20 --warmup 5]
A side is a library (selected through the PULSE_LIB environment variable, which pulselib_amd/_native.py honours -- diagnostic;
the host code is this checkout's) or a DIRECTORY: another checkout with its own built library, whose bench.py and host code
run (for a change that moves the host code along with the library, e.g. a new exported symbol)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
rounds = 2
if "--rounds" in args:
    i = args.index("--rounds")
    rounds = int(args[i + 1])
    del args[i:i + 2]
sides = [a for a in args if a.endswith(".so") or os.path.isdir(a)]
extra = [a for a in args if a not in sides]
if "--active-players" not in extra:
    extra = ["--active-players", "sampled", *extra]
runs = {s: [] for s in sides}
for rnd in range(rounds):
    for side in sides:
        tree = os.path.abspath(side) if os.path.isdir(side) else ROOT
        env = dict(os.environ) if os.path.isdir(side) else dict(os.environ, PULSE_LIB=os.path.abspath(side))
        p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--full", "--inproc", "--no-cpu-baseline", "--trainer-loop", "off", "--other-envs", "off",
                            "--census", "off", "--min-timed-ms", "600", *extra], env=env, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            # nothing more is started on a card after a run has failed (a fault or a time-out may be what ended it)
            sys.exit(f"{side}: FAILED rc={p.returncode}; stopping")
        d = json.loads(lines[-1])
        r, c = d["roofline"], d["config"]
        runs[side].append(d)
        print(f"round {rnd} {os.path.basename(os.path.normpath(side)):40s} value {d['value']:.4g}  ms_per_step {d.get('ms_per_step', float('nan')):.5f}  kernel {r['kernel_us']:.2f} us / {r['steps_per_launch']:.1f} steps  frac {r['frac']:.3f}"
              f"  timeouts {c.get('verdict_timeouts')} paired {c.get('paired_launches')} episodes {c.get('episodes_timed')} stats {json.dumps(c.get('episode_stats'))}", flush=True)
for side in sides:
    v = [d["value"] for d in runs[side]]
    m = [d.get("ms_per_step", float("nan")) for d in runs[side]]
    print(f"{os.path.basename(os.path.normpath(side)):40s} value median {statistics.median(v):.5g} min {min(v):.5g} max {max(v):.5g} (max/min {max(v) / min(v):.4f})"
          f"  ms_per_step median {statistics.median(m):.5f} min {min(m):.5f} max {max(m):.5f}", flush=True)
if len(sides) == 2:
    a, b = (statistics.median(d["value"] for d in runs[s]) for s in sides)
    print(f"ratio of medians (first / second): {a / b:.4f}", flush=True)
