"""bench.py's command line: a plain run times exactly --steps steps of the headline workload and nothing else; --full adds
the other measurements; --dump-outputs writes what the timed window computed, float32 / float64, capped, the same on every
run with the same arguments."""
import json
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parent.parent


def test_plain_run_times_the_headline_workload_only():
    plain = bench.parse_args(["--steps", "40", "--warmup", "3"])
    assert (plain.steps, plain.warmup, plain.full) == (40, 3, False)
    assert bench.headline_modes(plain) == ["sampled"]
    full = bench.parse_args(["--full"])
    assert bench.headline_modes(full) == ["sampled", "10"]
    assert bench.headline_modes(bench.parse_args(["--active-players", "10"])) == ["10"]
    assert bench.headline_modes(bench.parse_args(["--active-players", "both"])) == ["sampled", "10"]


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def _fake_env(n, table_id0):
    g = torch.Generator().manual_seed(3)
    return types.SimpleNamespace(obs=torch.rand(n, 40, generator=g), _rewards=[torch.rand(n, generator=g), torch.rand(n, generator=g)], _pp=0,
                                 is_done=torch.rand(n, generator=g) < .5, stacks=torch.randint(0, 1000, (n, 10), dtype=torch.int32, generator=g),
                                 n_games=n, device=torch.device("cpu"), table_id0=table_id0)


@pytest.mark.parametrize("world", [1, 8])
def test_dump_outputs_writes_the_last_step_within_the_cap(tmp_path, world):
    n, rank = 65536, world - 1
    env = _fake_env(n, rank * n)
    actions = torch.randint(0, 13, (n,), generator=torch.Generator().manual_seed(4))
    sums = {"last_step_reward_sum": 1.5, "tables_done_at_episode_end": 7.0}
    bench.dump_outputs(tmp_path / "a", env, actions, sums, rank, world)
    bench.dump_outputs(tmp_path / "b", env, actions, sums, rank, world)
    files = sorted((tmp_path / "a").iterdir())
    sfx = "" if world == 1 else f"_rank{rank}"
    assert [f.name for f in files] == sorted(f"{k}{sfx}.npy" for k in ("obs", "reward", "done", "action", "stacks", "table_id", "episode_stats"))
    assert sum(f.stat().st_size for f in files) * world <= bench.DUMP_LIMIT_BYTES
    for f in files:
        a, b = np.load(f), np.load(tmp_path / "b" / f.name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f.name
    rows = np.load(tmp_path / "a" / f"table_id{sfx}.npy").astype(np.int64) - rank * n
    assert (len(rows) == n) == (world == 1) and np.all(np.diff(rows) > 0)
    load = lambda k: np.load(tmp_path / "a" / f"{k}{sfx}.npy")
    assert np.array_equal(load("obs"), env.obs.numpy()[rows])
    assert np.array_equal(load("reward"), env._rewards[1].numpy()[rows])          # the buffer the last step wrote
    assert np.array_equal(load("done"), env.is_done.numpy()[rows].astype(np.float32))
    assert np.array_equal(load("action"), actions.numpy()[rows].astype(np.float32))
    assert np.array_equal(load("stacks"), env.stacks.numpy()[rows].astype(np.float32))
    assert load("episode_stats").tolist() == [1.5, 7.0]


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--inproc", "--tables", "4096", "--steps", "60", "--warmup", "10",
                            "--dump-outputs", str(out)], cwd=str(ROOT), stdout=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 60 and line["warmup"] == 10 and line["full"] is False and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(4096 * 60 / (line["ms_per_step"] * 60e-3))
        assert line["roofline"] is None and line["trainer_loop"] is None and "active_players_10" not in line
        runs.append({f.name: np.load(f) for f in out.iterdir()})
    assert sorted(runs[0]) == sorted(runs[1]) and len(runs[0]) == 7
    for name, a in runs[0].items():
        assert np.array_equal(a, runs[1][name]), name
    assert runs[0]["obs.npy"].shape == (4096, 40) and runs[0]["episode_stats.npy"][1] > 0
