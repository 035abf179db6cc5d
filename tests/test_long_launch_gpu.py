"""Long launches: pulse_poker_rollout_until enqueues all the check intervals the pairs of a call would
cover as one launch that takes the stop rule's verdicts itself -- held, call by call and bit for bit, to the same loop with
one check interval per launch AND to the loop with pairs; the step loop of one 40-step launch to eight launches of five; the
called-off check point; the gate."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests.helpers import to_np
from tests.test_poker_gpu_parity import DEV, ROLLOUT_MEMORY, _gpu_env

pytestmark = pytest.mark.gpu

TYPES = [1, 3, 2, 4, 5, 1]
# episodes as the caps of their calls: long launches that start an episode and that start mid-episode (behind a pair and a
# one-chunk launch, behind two pairs, behind another long launch), a short last chunk behind a long launch (23: the long
# launch covers the chunks pairs would, 20 steps; the last 3 run as a launch of their own), calls that stay pairs (7, 10, 10)
EPISODES = ((60,), (40,), (23,), (7,), (15, 40), (10, 10, 40), (20, 20))
ACTIVE = (6, 5, 2, 4, 6, 3, 5)


def _assert_same_memory(a, b, acts, ctx):
    for name in ROLLOUT_MEMORY:
        np.testing.assert_array_equal(to_np(getattr(a, name)), to_np(getattr(b, name)), err_msg=f"{ctx} {name}")
    for k in range(2):
        np.testing.assert_array_equal(to_np(a._obs_bufs[k]), to_np(b._obs_bufs[k]), err_msg=f"{ctx} obs buffer {k}")
        np.testing.assert_array_equal(to_np(a._rewards[k]), to_np(b._rewards[k]), err_msg=f"{ctx} rewards buffer {k}")
        np.testing.assert_array_equal(to_np(a._done_bufs[k]), to_np(b._done_bufs[k]), err_msg=f"{ctx} done buffer {k}")
    assert a._pp == b._pp, ctx
    np.testing.assert_array_equal(to_np(acts[0]), to_np(acts[1]), err_msg=f"{ctx} actions")


def _envs(N, seed=21):
    kw = dict(n_players=6, max_players=10, n_games=N, seed=seed, table_id0=3)
    a, b = _gpu_env(**kw), _gpu_env(**kw)
    assert a.long_launches and a.paired_launches
    b.paired_launches = False
    acts = [torch.zeros(N, dtype=torch.long, device=torch.device(DEV)) for _ in range(2)]
    return a, b, acts


def expected_of_paired_loop(unpaired, cap):
    """What a call of `cap` steps returns with pairs (and so with long launches), from what the loop with one check interval
    per launch returns.  The steps are the same.  `over` is the same EXCEPT where the call's last launch is a pair that ran
    both its chunks: the unpaired loop has then read the count of the call's last check point but one, which is that pair's
    own first check point -- "a launch that runs both its chunks never ends the episode itself: `over` comes with the launch
    that is cut or cancelled" (pinned by test_paired_launches_match_the_oracle_after_every_launch).  The last launch is such
    a pair exactly when the call ran to its cap and the cap is whole pairs (a multiple of 10 steps); any other call ends
    with a cut launch or with a one-chunk launch, whose host knows that count."""
    steps, over = unpaired
    return (steps, over and not (steps == cap and cap % 10 == 0))


def _play(a, b, ra, rb, acts, episodes, gstep, seen, ctx, first_episode=0, pairs_only=None):
    """Plays `episodes` on both environments, comparing after every call; records in `seen` what the long launches did.
    `pairs_only` = (env, rule, actions): the loop with pairs but without long launches plays along, and every call of `a`
    must return exactly what its call returns and leave exactly its memory."""
    for e, caps in enumerate(episodes, start=first_episode):
        for env, rule in ((a, ra), (b, rb)) + (((pairs_only[0], pairs_only[1]),) if pairs_only else ()):
            env.reset(options={"active_players": ACTIVE[e % len(ACTIVE)], "rotation": e})
            rule.drain()
        total = 0
        for cap in caps:
            before = ra.stats()
            got = a.rollout_until(TYPES, acts[0], 5, cap, gstep + total, ra)
            unpaired = b.rollout_until(TYPES, acts[1], 5, cap, gstep + total, rb)
            after = ra.stats()
            want = expected_of_paired_loop(unpaired, cap)
            assert got == want, f"{ctx} episode {e} cap {cap}: long {got}, expected {want} (one check interval per launch: {unpaired})"
            _assert_same_memory(a, b, acts, f"{ctx} episode {e} cap {cap}")
            if pairs_only:
                c, rc, acts_c = pairs_only
                assert c.rollout_until(TYPES, acts_c, 5, cap, gstep + total, rc) == got, f"{ctx} episode {e} cap {cap}: long {got} differs from pairs"
                _assert_same_memory(a, c, (acts[0], acts_c), f"{ctx} episode {e} cap {cap} (against pairs)")
            if got != unpaired:
                # the late `over`: the very next launch brings it, runs nothing and leaves no trace
                again = a.rollout_until(TYPES, acts[0], 5, 5, gstep + total + got[0], ra)
                assert again == (0, True), f"{ctx} episode {e} cap {cap}: the launch after the pair gave {again}"
                _assert_same_memory(a, b, acts, f"{ctx} episode {e} cap {cap} (after the cancelled launch)")
                if pairs_only:
                    assert c.rollout_until(TYPES, acts_c, 5, 5, gstep + total + got[0], rc) == (0, True)
                got = unpaired
            total += got[0]
            if after["long_launches"] > before["long_launches"]:
                assert after["long_launches"] == before["long_launches"] + 1 and cap > 10
                steps, over = got
                if over and steps == 10 and after["in_launch_verdicts"] == before["in_launch_verdicts"] + 1:
                    seen.add("first check point")
                if over and steps > 10:
                    seen.add("later check point")
                if not over and steps == cap:
                    seen.add("cap")
            else:
                assert after["in_launch_verdicts"] == before["in_launch_verdicts"]
            if got[1]:
                seen.add(("even", "odd")[(total // 5) % 2])
                break
        gstep += total
    return gstep


@pytest.mark.parametrize("N", [64, 4096, 4099, 65536], ids=["64-one-workgroup", "4096", "4099-ragged", "65536-residency-at-the-gate"])
def test_long_launches_run_the_episodes_of_one_chunk_per_launch(N):
    """Every episode of EPISODES under thresholds 0.8 (the rule ends the episode somewhere inside a launch), 0.05 (the
    launch's first check point is already over: it runs exactly two chunks) and 1.0 (never over: it runs to its cap)
    -- the bench size under 0.8 and 1.0, for time.  After every call: bit-identical memory and the same steps as the loop
    with one check interval per launch, its `over` too except where expected_of_paired_loop says why not, and (up to 4,099
    tables) exactly the loop with pairs.  Not vacuous: the stats and step counts must show an episode ended by an in-launch verdict at the first check point of its
    launch, one at a later check point, one that ran to its cap, and ends after even and odd numbers of chunks."""
    from pulselib_amd.stoprule import LaggedDoneCount
    dev = torch.device(DEV)
    a, b, acts = _envs(N)
    c = None
    if N != 65536:
        c = _gpu_env(n_players=6, max_players=10, n_games=N, seed=21, table_id0=3)
        c.long_launches = False
        acts_c = torch.zeros(N, dtype=torch.long, device=dev)
    seen, gstep = set(), 0
    for threshold in ((0.8, 1.0) if N == 65536 else (0.8, 0.05, 1.0)):
        ra, rb = LaggedDoneCount(dev, N, threshold, lag=1), LaggedDoneCount(dev, N, threshold, lag=1)
        rc = LaggedDoneCount(dev, N, threshold, lag=1) if c is not None else None
        assert ra.stats()["long"]
        gstep = _play(a, b, ra, rb, acts, EPISODES, gstep, seen, f"N={N} threshold {threshold}", pairs_only=(c, rc, acts_c) if c is not None else None)
        if rc is not None:
            assert rc.stats()["long_launches"] == 0 and rc.stats()["paired_launches"] > 0
            rc.close()
        st = ra.stats()
        assert st["called_off"] == 0 and st["verdict_timeouts"] == 0 and st["long"] and st["pairs"], st
        assert st["long_launches"] >= 3 and st["paired_launches"] > st["long_launches"], st      # (calls of < 20 steps stay pairs)
        assert st["in_launch_verdicts"] > 0, st
        assert rb.stats()["paired_launches"] == 0
        ra.close(); rb.close()
    if N == 65536:
        assert seen & {"first check point", "later check point"} and "cap" in seen, seen
    else:
        assert seen >= {"first check point", "later check point", "cap", "even", "odd"}, seen


def test_one_launch_of_40_steps_equals_eight_of_5():
    """The step loop itself, without a rule: rollout(.., 40, ..) against 8 x rollout(.., 5, ..) at 4,099 tables (a ragged last
    wavefront, no observation staging)."""
    a, b, acts = _envs(4099, seed=5)
    for e in range(2):
        for env in (a, b):
            env.reset(options={"active_players": 6 - e, "rotation": e})
        a.rollout(TYPES, acts[0], 40, 100 * e)
        for c in range(8):
            b.rollout(TYPES, acts[1], 5, 100 * e + 5 * c)
        _assert_same_memory(a, b, acts, f"episode {e}")


def test_a_check_point_nobody_decides_is_called_off_and_the_episode_goes_on_in_pairs():
    """With the wait cut to 50 ms and the first check point of the second episode's launch left undecided (test hook), its
    waiters run into the bound and call it off: the launch ends behind its second chunk as if planned that long, the
    native loop goes on with pairs, the handle counts the call-off and plans no long launch again -- every episode,
    before and after, equals the loop that never paired, bit for bit."""
    from pulselib_amd.stoprule import LaggedDoneCount
    dev = torch.device(DEV)
    N = 4096
    a, b, acts = _envs(N, seed=33)
    ra, rb = LaggedDoneCount(dev, N, 0.8, lag=1), LaggedDoneCount(dev, N, 0.8, lag=1)
    ra.set_option(LaggedDoneCount.OPT_VERDICT_WAIT_TICKS, 5_000_000)
    gstep = 0
    for e in range(4):
        for env, rule in ((a, ra), (b, rb)):
            env.reset(options={"active_players": (6, 5, 4, 6)[e], "rotation": e})
            rule.drain()
        if e == 1:
            st = ra.stats()
            assert st["long_launches"] == 1 and st["called_off"] == 0 and st["long"], st
            ra.set_option(LaggedDoneCount.OPT_DEBUG_SKIP_DECISION, 1)
        t0 = time.perf_counter()
        got = a.rollout_until(TYPES, acts[0], 5, 60, gstep, ra)
        torch.cuda.synchronize()
        assert time.perf_counter() - t0 < 5.0
        want = b.rollout_until(TYPES, acts[1], 5, 60, gstep, rb)
        assert got == want, f"episode {e}: {got} vs unpaired {want}"
        _assert_same_memory(a, b, acts, f"episode {e}")
        gstep += got[0]
        st = ra.stats()
        assert st["verdict_timeouts"] == 0 and st["pairs"], st
        if e == 0:
            assert st["long_launches"] == 1 and st["called_off"] == 0 and st["long"], st
        else:
            assert st["long_launches"] == 2 and st["called_off"] == 1 and not st["long"], st
    ra.close(); rb.close()


@pytest.mark.parametrize("how", ["resident-blocks-1", "shm-world-1", "lag-0", "lag-2", "option-off"])
def test_the_gate_issues_no_long_launch(how):
    """No long launch where wavefronts might wait for one that is not on the device (the occupancy answer overridden to one
    workgroup per compute unit: minus the margin, none), where the count is not the device's own to take (a handle made for
    a shared-memory exchange, here of one rank), or where the rule is not lag 1 -- the episodes are the unpaired loop's."""
    from pulselib_amd import _native
    from pulselib_amd.stoprule import LaggedDoneCount
    dev = torch.device(DEV)
    N = 4096
    lag = {"lag-0": 0, "lag-2": 2}.get(how, 1)
    a, b, acts = _envs(N, seed=9)
    ra, rb = LaggedDoneCount(dev, N, 0.8, lag=lag), LaggedDoneCount(dev, N, 0.8, lag=lag)
    if how == "resident-blocks-1":
        ra.set_option(LaggedDoneCount.OPT_DEBUG_RESIDENT_BLOCKS, 1)
    if how == "option-off":
        ra.set_option(LaggedDoneCount.OPT_LONG_LAUNCHES, 0)
    if how == "shm-world-1":
        lib = _native.lib()
        lib.pulse_stoprule_destroy(ra.handle)
        h = C.c_void_p()
        name = f"/pulse_long_gate_{time.time_ns():x}".encode()
        with torch.cuda.device(dev):
            _native.check(lib.pulse_stoprule_create(N, N, 0.8, 1, None, name, 0, 1, C.byref(h)), "pulse_stoprule_create")
        ra.handle = h
        assert not ra.stats()["long"]
    seen = set()
    _play(a, b, ra, rb, acts, ((60,), (15, 40), (23,)), 0, seen, how)
    st = ra.stats()
    assert st["long_launches"] == 0 and st["in_launch_verdicts"] == 0 and st["called_off"] == 0, st
    assert (st["paired_launches"] > 0) == (lag == 1)
    ra.close(); rb.close()
