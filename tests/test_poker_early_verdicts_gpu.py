"""Early verdicts of a long launch (PULSE_STOPRULE_OPT_EARLY_VERDICTS): the launch's first check point is
no end, and in front of the two closing steps of every later check point a wavefront looks -- one load, no loop -- whether the
verdict that check point will read is settled; behind a settled "go on" the two closing steps run dead and the check point reads nothing.  Which
steps a wavefront runs live may differ from run to run; what a call returns and leaves in memory must not: held here, on
poisoned outputs, across the option's four values and against the loop with one check interval per launch."""
import numpy as np
import pytest
import torch

from tests.helpers import to_np
from tests.test_long_launch_gpu import ACTIVE, EPISODES, TYPES, expected_of_paired_loop
from tests.test_poker_gpu_parity import DEV, _gpu_env
from tests.test_poker_live_outputs_gpu import _assert_same_memory, _poison_outputs

pytestmark = pytest.mark.gpu

# Tables that finished / dealt a street / reached showdown on the two steps in front of a check point a long launch went on
# past (steps the parent ran live): in front of the launch's first check point (dead in every wavefront now) and of later ones
# (dead wherever the look found its word).  Floors for the 4,096-table run, counted by the singly-stepped environment alone:
# six-seat tables finish a hand in ~15 steps, so each of ~25 such step pairs sees a few per cent of 4,096 tables do each.
FLOORS = {"first: finished": 100, "first: street": 100, "first: showdown": 10, "later: finished": 100, "later: street": 100, "later: showdown": 10}


def _probe_state(env):
    return to_np(env.stages).copy(), to_np(env.is_done).astype(bool).copy()


def _census_of_call(census, probe, acts, steps, gstep, launch_steps):
    """Steps the probe singly through the call's `steps` steps; the call's first launch was a long one that ran `launch_steps`
    of them (0: it was none).  Counts the events of steps 5q - 2 and 5q - 1 for every check point q with 5q < launch_steps."""
    stage, done = _probe_state(probe)
    for i in range(steps):
        probe.rollout(TYPES, acts, 1, gstep + i)
        stage1, done1 = _probe_state(probe)
        q = (i + 2) // 5 if i % 5 >= 3 else 0                 # the check point this step closes in on
        if q >= 1 and 5 * q < launch_steps:
            fin = done1 & ~done
            which = "first" if q == 1 else "later"
            census[f"{which}: finished"] += int(fin.sum())
            census[f"{which}: street"] += int((~done1 & (stage1 == stage + 1) & (stage1 >= 1) & (stage1 <= 3)).sum())
            census[f"{which}: showdown"] += int((fin & (stage1 == 5)).sum())
        stage, done = stage1, done1


@pytest.mark.parametrize("N", [64, 4096, 4099], ids=["64-one-workgroup", "4096", "4099-ragged-direct-stores"])
def test_every_option_leaves_the_memory_and_the_steps_of_one_interval_per_launch(N):
    """Four environments through EPISODES (calls of 60, 40, 23 and 7 steps from a reset, 40-step calls that start mid-episode)
    under thresholds 0.8, 0.05 (the verdict the first look finds is "over": exactly two chunks) and 1.0 (to the cap): long launches
    with the option at 2, 3 and 0, and the loop with one check interval per launch.  Every output word a call does not read is
    poisoned before it.  After every call the three return the same (steps, over) -- the other loop's but for the late `over`
    of expected_of_paired_loop -- and all four hold the same memory bit for bit: state words, equities, equity_dirty, both
    observation / reward / done sets, actions.
    Not vacuous: option 2 finds settled verdicts under every threshold; under 0.05 a launch of exactly two chunks was ended
    by an in-launch verdict its wavefronts had from the look; option 3 has looks that found and looks that did not in one launch;
    option 0 counts neither.  At 4,096 tables a fifth environment, stepped singly, counts what happened on steps that run dead
    now and ran live before (FLOORS)."""
    from pulselib_amd.stoprule import LaggedDoneCount
    dev = torch.device(DEV)
    kw = dict(n_players=6, max_players=10, n_games=N, seed=21, table_id0=3)
    envs = [_gpu_env(**kw) for _ in range(4)]
    probe = _gpu_env(**kw) if N == 4096 else None
    for env in envs + ([probe] if probe else []):
        env.double_buffer_obs = True
    assert all(env.long_launches and env.paired_launches for env in envs)
    envs[3].long_launches = envs[3].paired_launches = False
    if probe:
        probe.chunked_rollout = False
    acts = [torch.zeros(N, dtype=torch.long, device=dev) for _ in range(5)]
    census = {k: 0 for k in FLOORS}
    gstep = 0
    for threshold in (0.8, 0.05, 1.0):
        rules = [LaggedDoneCount(dev, N, threshold, lag=1) for _ in range(4)]
        for rule, option in zip(rules[:3], (2, 3, 0)):
            rule.set_option(LaggedDoneCount.OPT_EARLY_VERDICTS, option)
        two_chunks_by_a_look = mixed_launch = False
        for e, caps in enumerate(EPISODES):
            for env, rule in zip(envs, rules):
                env.reset(options={"active_players": ACTIVE[e % len(ACTIVE)], "rotation": e})
                rule.drain()
            if probe:
                probe.reset(options={"active_players": ACTIVE[e % len(ACTIVE)], "rotation": e})
            total = 0
            for cap in caps:
                for env in envs:
                    _poison_outputs(env)
                before = [rule.stats() for rule in rules[:3]]
                got = [env.rollout_until(TYPES, a, 5, cap, gstep + total, rule) for env, a, rule in zip(envs, acts, rules)]
                after = [rule.stats() for rule in rules[:3]]
                ctx = f"N={N} threshold {threshold} episode {e} cap {cap}: option 2 / 3 / 0 / one interval per launch {got}"
                assert got[0] == got[1] == got[2] == expected_of_paired_loop(got[3], cap), ctx
                for k in (1, 2, 3):
                    _assert_same_memory(envs[0], envs[k], (acts[0], acts[k]), None, f"{ctx} (environment {k})")
                steps, over = got[0]
                delta = [{k: after[r][k] - before[r][k] for k in ("long_launches", "in_launch_verdicts", "early_hits", "early_misses")} for r in range(3)]
                assert delta[0]["long_launches"] == delta[1]["long_launches"] == delta[2]["long_launches"] == (1 if cap >= 20 else 0), (ctx, delta)
                if over and steps == 10 and delta[0]["in_launch_verdicts"] == 1 and delta[0]["early_hits"] > 0:
                    two_chunks_by_a_look = True
                mixed_launch = mixed_launch or (delta[1]["early_hits"] > 0 and delta[1]["early_misses"] > 0)
                if probe and steps > 0:
                    launch_steps = min(steps, 10 * (cap // 10)) if delta[0]["long_launches"] else 0
                    _census_of_call(census, probe, acts[4], steps, gstep + total, launch_steps)
                    np.testing.assert_array_equal(to_np(probe.stages), to_np(envs[3].stages), err_msg=f"{ctx}: the probe left the games")
                if got[0] != got[3]:
                    # the late `over`: the very next launch brings it and runs nothing
                    for env, a, rule in zip(envs[:3], acts, rules):
                        assert env.rollout_until(TYPES, a, 5, 5, gstep + total + steps, rule) == (0, True), ctx
                    over = True
                total += steps
                if over:
                    break
            gstep += total
        st = [rule.stats() for rule in rules]
        print(f"N={N} threshold {threshold}: option 2 hits / misses {st[0]['early_hits']} / {st[0]['early_misses']}, "
              f"option 3 {st[1]['early_hits']} / {st[1]['early_misses']}, long launches {st[0]['long_launches']}")
        for s in st[:3]:
            assert s["called_off"] == 0 and s["verdict_timeouts"] == 0 and s["long"] and s["long_launches"] >= 3, s
        assert st[3]["paired_launches"] == 0
        assert st[0]["early_hits"] > 0, st[0]
        assert st[1]["early_hits"] > 0 and st[1]["early_misses"] > 0 and mixed_launch, st[1]
        assert st[2]["early_hits"] == 0 and st[2]["early_misses"] == 0, st[2]
        assert threshold != 0.05 or two_chunks_by_a_look
        for rule in rules:
            rule.close()
    if probe:
        print(f"census of steps cp - 2, cp - 1 in front of check points the launches went on past: {census}")
        assert all(census[k] >= FLOORS[k] for k in FLOORS), census


def test_one_launch_of_40_steps_equals_eight_of_5_without_a_rule():
    """The step loop's own path (no long launch, so no look): rollout(.., 40, ..) against 8 x rollout(.., 5, ..) at 4,099 tables
    (a ragged last wavefront, no observation staging), on poisoned outputs."""
    kw = dict(n_players=6, max_players=10, n_games=4099, seed=5, table_id0=3)
    a, b = _gpu_env(**kw), _gpu_env(**kw)
    a.double_buffer_obs = b.double_buffer_obs = True
    acts = [torch.zeros(4099, dtype=torch.long, device=torch.device(DEV)) for _ in range(2)]
    for e in range(2):
        for env in (a, b):
            env.reset(options={"active_players": 6 - e, "rotation": e})
            _poison_outputs(env)
        a.rollout(TYPES, acts[0], 40, 100 * e)
        for c in range(8):
            b.rollout(TYPES, acts[1], 5, 100 * e + 5 * c)
        _assert_same_memory(a, b, acts, None, f"episode {e}")
