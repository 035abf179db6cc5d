"""utils/stability.py against the reference's own (tests/golden/stability.npz, tests/golden/make_stability_golden.py): the
per-step metrics of the CPU torch path on seeded batches (one without a valid row), the episode and final aggregations
(empty and single-episode cases included); and the C ABI of the metrics (PulseQNetTrain.stability, the slice pitch)."""
import ctypes as C

import numpy as np
import pytest
import torch

METRICS = ("loss", "td_error", "grad_norm", "clip_rate", "q_mean", "q_min", "q_max")
EPISODE = ("reward", "q_mean", "q_min", "q_max", "td_error", "clip_rate")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "stability.npz")


def test_fixture_names(g):
    assert tuple(g["metric_names"]) == METRICS and tuple(g["episode_names"]) == EPISODE


def test_cpu_steps_reproduce_the_reference(g):
    from pulselib_amd.environments.Poker import PokerQNetwork
    from pulselib_amd.utils.stability import run_stability_measured_q_learning_step
    q = PokerQNetwork(None, torch.device("cpu"), gamma=.95, update_freq=2, state_dim=40, action_dim=13, learning_rate=2e-4,
                      weight_decay=1e-5)
    q.network.load_state_dict({k.split("/")[-1]: torch.from_numpy(g[k]) for k in g.files if k.startswith("steps/w0/")})
    q.target_network.load_state_dict(q.network.state_dict())
    want, valid = g["steps/metrics"], g["steps/valid"]
    assert valid.sum() < valid.size, "premise: one batch without a valid row"
    for i in range(valid.size):
        b = {k: torch.from_numpy(g[f"steps/b{i}/{k}"]) for k in ("states", "next_states", "actions", "rewards", "dones")}
        torch.manual_seed(int(g[f"steps/b{i}/seed"]))
        m = run_stability_measured_q_learning_step(q, b["states"], b["actions"], b["rewards"], b["next_states"], b["dones"])
        if not valid[i]:
            assert m is None, f"batch {i}: no valid row -> None"
            continue
        assert set(m) == set(METRICS)
        got = np.array([float(m[k]) for k in METRICS])
        # (the fused CPU AdamW of the reference against the unfused one here: a few ulp per step, compounded over the steps)
        np.testing.assert_allclose(got, want[i], rtol=2e-5, atol=2e-6, err_msg=f"batch {i}")
        assert all(v.dim() == 0 for v in m.values())
    assert q.step_count == int(g["steps/step_count"])


def test_episode_summaries_reproduce_the_reference(g):
    from pulselib_amd.utils.stability import summarize_episode_stability_metrics
    for e in range(int(g["episode/count"])):
        seq = g[f"episode/e{e}/steps"]
        steps = [{k: torch.tensor(seq[s, j]) for j, k in enumerate(METRICS)} for s in range(seq.shape[0])]
        out = summarize_episode_stability_metrics(torch.tensor(g[f"episode/e{e}/reward"]), steps)
        np.testing.assert_allclose([float(out[k]) for k in EPISODE], g[f"episode/e{e}/out"], rtol=1e-6, atol=1e-7, err_msg=f"episode {e}")


def test_final_metrics_reproduce_the_reference(g):
    from pulselib_amd.utils.stability import calculate_final_stability_metrics, calculate_td_error_trend
    for c in range(int(g["final/count"])):
        ep = g[f"final/c{c}/episodes"]
        cols = {k: [torch.tensor(ep[i, j]) for i in range(ep.shape[0])] for j, k in enumerate(EPISODE)}
        f = calculate_final_stability_metrics(epoch_rewards=cols["reward"], epoch_q_means=cols["q_mean"], epoch_q_mins=cols["q_min"],
                                              epoch_q_maxs=cols["q_max"], epoch_td_errors=cols["td_error"],
                                              epoch_clip_rates=cols["clip_rate"], elapsed_seconds=float(g[f"final/c{c}/elapsed"]))
        assert set(f) == {"reward_std", "mean_reward", "q_bounds", "td_error_trend", "average_clip_rate", "total_time_seconds"}
        assert set(f["q_bounds"]) == {"global_min", "global_max", "mean_q"}
        got = [float(f["reward_std"]), float(f["mean_reward"]), float(f["q_bounds"]["global_min"]), float(f["q_bounds"]["global_max"]),
               float(f["q_bounds"]["mean_q"]), float(f["td_error_trend"]), float(f["average_clip_rate"]), float(f["total_time_seconds"])]
        np.testing.assert_allclose(got, g[f"final/c{c}/out"], rtol=1e-6, atol=1e-6, err_msg=f"case {c} ({ep.shape[0]} episodes)")
        assert abs(float(calculate_td_error_trend(cols["td_error"])) - float(g[f"final/c{c}/trend"])) <= 1e-6
        if ep.shape[0] == 1:
            assert float(f["td_error_trend"]) == 0.0


def test_accumulator_values_give_the_episode_summary():
    """episode_from_accumulator (what StabilityMetrics reads back) == summarize_episode_stability_metrics over the steps the
    accumulator summed, and the cleared accumulator (+inf / -inf) gives the empty episode."""
    from pulselib_amd.utils.stability import episode_from_accumulator, summarize_episode_stability_metrics
    rng = np.random.default_rng(3)
    seq = rng.standard_normal((6, len(METRICS))).astype(np.float32)
    seq[:, METRICS.index("clip_rate")] = [1, 0, 0, 1, 1, 0]
    steps = [{k: torch.tensor(seq[s, j]) for j, k in enumerate(METRICS)} for s in range(6)]
    col = {k: seq[:, j].astype(np.float64) for j, k in enumerate(METRICS)}
    acc = [6.0, col["td_error"].sum(), col["q_mean"].sum(), col["q_min"].min(), col["q_max"].max(), col["clip_rate"].sum(),
           col["loss"].sum(), 0.0]
    want = summarize_episode_stability_metrics(torch.tensor(2.5), steps)
    got = episode_from_accumulator(2.5, acc)
    np.testing.assert_allclose([got[k] for k in EPISODE], [float(want[k]) for k in EPISODE], rtol=1e-6, atol=1e-7)
    empty = episode_from_accumulator(-1.0, [0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, 0.0, 0.0])
    want0 = summarize_episode_stability_metrics(torch.tensor(-1.0), [])
    assert [empty[k] for k in EPISODE] == [float(want0[k]) for k in EPISODE]


def test_abi_stability_field_and_slice_pitch():
    from pulselib_amd import _native
    names = [f[0] for f in _native.QNetTrain._fields_]
    assert names[-2:] == ["reserved0", "stability"]
    assert _native.QNetTrain.stability.offset == C.sizeof(_native.QNetTrain) - C.sizeof(C.c_void_p)
    floats = _native.lib().pulse_qnet_slice_floats()
    assert floats % 4 == 0
    # 35 gradient blocks of 32 x 32, 384 bias slots, 8 statistics (pulse_env.h: PulseQNetTrain.stability)
    assert floats == 35 * 1024 + 384 + 8


def test_stability_needs_the_native_learner():
    from pulselib_amd.scripts.trainGPU import train_agent_fused
    from pulselib_amd.environments.Poker.utils import PokerAgentType

    class Learner:
        act_into = train_step_masked = train_step_native = None
    with pytest.raises(ValueError, match="stability_metrics needs learner='native'"):
        train_agent_fused(None, [Learner()], [PokerAgentType.QLEARNING], 1, 4, "cpu", learner="torch", stability_metrics=object())
