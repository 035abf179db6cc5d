"""The chunk kernel stores only the step outputs a launch can leave ("live steps"): step i of a launch
writes its reward, observation and done flag into buffer set i mod 2, so only the last two steps before a possible end of the
launch are materialised.  What a caller can observe must not change: after every call the memory is, bit for bit, that of the
same steps taken as single launches -- checked with every output word the call does not read poisoned beforehand, for every
chunk form and for every end a launch can take."""
import numpy as np
import pytest
import torch

from tests.helpers import to_np
from tests.test_long_launch_gpu import ACTIVE, EPISODES, TYPES
from tests.test_poker_gpu_parity import DEV, ROLLOUT_MEMORY, _gpu_env

pytestmark = pytest.mark.gpu

POISON_I32 = 0x7FC0DEAD          # a NaN no step computes (observations and rewards); 0xAB for the done flags
POISON_U8 = 0xAB


def _bits(t):
    """The tensor's words as integers: NaNs and the bytes of a bool compare bit for bit."""
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return to_np(t)


def _poison_outputs(env):
    """Every output word a call is not defined to read: both observation buffers, both reward buffers, and the done buffer of
    the side that is not current (the current one holds the flags the first step reads)."""
    env._view()                                              # (re)binds the ping-pong buffers if the env was touched
    for k in range(2):
        env._obs_bufs[k].view(torch.int32).fill_(POISON_I32)
        env._rewards[k].view(torch.int32).fill_(POISON_I32)
    env._done_bufs[1 - env._pp].view(torch.uint8).fill_(POISON_U8)


def _assert_same_memory(a, b, acts, outs, ctx):
    for name in ROLLOUT_MEMORY:
        np.testing.assert_array_equal(_bits(getattr(a, name)), _bits(getattr(b, name)), err_msg=f"{ctx} {name}")
    for k in range(2):
        np.testing.assert_array_equal(_bits(a._obs_bufs[k]), _bits(b._obs_bufs[k]), err_msg=f"{ctx} obs buffer {k}")
        np.testing.assert_array_equal(_bits(a._rewards[k]), _bits(b._rewards[k]), err_msg=f"{ctx} rewards buffer {k}")
        np.testing.assert_array_equal(_bits(a._done_bufs[k]), _bits(b._done_bufs[k]), err_msg=f"{ctx} done buffer {k}")
    assert a._pp == b._pp, ctx
    np.testing.assert_array_equal(to_np(acts[0]), to_np(acts[1]), err_msg=f"{ctx} actions")
    if outs is not None:
        for x, y in zip(outs[0][:3], outs[1][:3]):          # what the call returns: last observation, rewards, dones
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{ctx} returned")


SHAPES = [(32, 10, 10, False, False), (32, 10, 10, False, True), (64, 10, 10, False, True), (50, 10, 10, False, True), (1, 2, 2, False, True),
          (64, 10, 10, True, True), (48, 12, 12, False, True), (32, 16, 16, False, True), (98304, 10, 10, False, True)]
IDS = ["32x10-one-wavefront-staged-one-obs-buffer", "32x10-one-wavefront-staged", "64x10", "50x10-ragged-direct-stores", "1x2", "64x10-four-lanes",
       "48x12-four-lanes-spl3", "32x16-four-lanes-spl4", "98304x10-slim-lds-image"]


@pytest.mark.parametrize("N,P,MP,four,dbl", SHAPES, ids=IDS)
def test_a_chunk_leaves_the_memory_of_single_launches_in_poisoned_outputs(N, P, MP, four, dbl):
    """rollout(.., n, ..) as ONE launch against the same call as n single-step launches (chunked_rollout = False), both on
    outputs poisoned before the call: n = 1..12 and 19 (the slim image: 1, 2, 7, 12), twice over so that every n starts from
    odd and even step counters and from both ping-pong sides.  Equal bit for bit afterwards: every state tensor, both
    observation, reward and done buffers, the actions, the returned triple and the ping-pong side; after n = 1 the set the
    step did not write still holds the poison in both environments."""
    kw = dict(n_players=P, max_players=MP, n_games=N, w1=.5, w2=.3, K=100, alpha=50, seed=91, table_id0=7)
    one, per = _gpu_env(**kw), _gpu_env(**kw)
    per.chunked_rollout = False
    one.chunk_four_lanes = four
    one.double_buffer_obs = per.double_buffer_obs = dbl
    types = ([0, 3, 2, 2, 4, 3, 1, 4, 5, 3, 1, 2, 3, 4, 5, 1])[:P]          # seat 0 external
    rng = np.random.default_rng(5)
    lengths = (1, 2, 7, 12) if N == 98304 else tuple(range(1, 13)) + (19,)
    gstep, in_episode, e, parities, finished = 3, None, 0, set(), 0.0
    for rnd in range(2):
        for n in (lengths if rnd == 0 else lengths[::-1]):
            if in_episode is None or in_episode > 24:        # a fresh episode before the tables have all finished
                for env in (one, per):
                    env.reset(options={"active_players": (P, max(2, P // 2))[e % 2], "rotation": e})
                in_episode, e = 0, e + 1
            gstep += (gstep ^ rnd ^ 1) & 1                   # first round: odd step counters, second round: even ones
            ext = torch.from_numpy(rng.integers(0, 13, N)).to(DEV)
            acts = [ext.clone(), ext.clone()]
            for env in (one, per):
                _poison_outputs(env)
            pp0 = one._pp
            assert per._pp == pp0
            outs = [env.rollout(types, a, n, gstep) for env, a in zip((one, per), acts)]
            parities.add((n, gstep & 1))
            ctx = f"N{N} episode {e} chunk of {n} from step {gstep} side {pp0}"
            gstep += n
            in_episode += n
            _assert_same_memory(one, per, acts, outs, ctx)
            finished = max(finished, float(to_np(one.is_done).mean()))
            for env in (one, per):
                written = {0, 1} if n >= 2 else {pp0}
                for k in {0, 1} - written:                  # step 0 writes reward buffer pp0 and observation / done buffer 1 - pp0
                    assert (_bits(env._rewards[k]) == POISON_I32).all(), f"{ctx}: reward buffer {k} was written"
                    if dbl:
                        assert (_bits(env._obs_bufs[1 - k]) == POISON_I32).all(), f"{ctx}: observation buffer {1 - k} was written"
                for k in written:
                    assert not (_bits(env._rewards[k]) == POISON_I32).any(), f"{ctx}: reward buffer {k} keeps poison"
                for k in range(2):
                    assert not (_bits(env._done_bufs[k]) == POISON_U8).any(), f"{ctx}: done buffer {k} keeps poison"
                    if n >= 2 or not dbl or k == 1 - pp0:
                        assert not (_bits(env._obs_bufs[k]) == POISON_I32).any(), f"{ctx}: observation buffer {k} keeps poison"
    assert all((n, 0) in parities and (n, 1) in parities for n in lengths), sorted(parities)
    assert finished > 0.3 or N == 1, finished          # the calls ran into finished tables too


@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("long", [True, False], ids=["long-launches", "pairs-only"])
def test_every_end_a_launch_can_take_leaves_the_memory_of_single_launches(N, long):
    """rollout_until under a lag-1 rule, on poisoned outputs, against the per-step environment stepped for the steps each
    call returned.  Episodes and seats as in test_long_launch_gpu (plus a cap of 13), thresholds 0.8 and 0.5 (the rule ends
    the episode inside a launch), 0.05 (over at the first check point) and 1.0 (never over).  With long launches: launches
    ended by an in-launch verdict behind their second chunk and behind a later one, launches that run to their cap, caps
    that are no multiple of the check interval (7, 13, 23).  With long launches switched off on the rule: pairs cut at their
    middle and pairs that run through.  Not vacuous: the stats and step counts must show each of these ends."""
    from pulselib_amd.stoprule import LaggedDoneCount
    dev = torch.device(DEV)
    kw = dict(n_players=6, max_players=10, n_games=N, seed=21, table_id0=3)
    a, per = _gpu_env(**kw), _gpu_env(**kw)
    per.chunked_rollout = False
    a.double_buffer_obs = per.double_buffer_obs = True
    assert a.long_launches and a.paired_launches
    acts = [torch.zeros(N, dtype=torch.long, device=dev) for _ in range(2)]
    episodes = EPISODES + ((13,),)
    seen, gstep = set(), 0
    for threshold in (0.8, 0.05, 1.0, 0.5):
        rule = LaggedDoneCount(dev, N, threshold, lag=1)
        if not long:
            rule.set_option(LaggedDoneCount.OPT_LONG_LAUNCHES, 0)
        for e, caps in enumerate(episodes):
            for env in (a, per):
                env.reset(options={"active_players": ACTIVE[e % len(ACTIVE)], "rotation": e})
            rule.drain()
            total = 0
            for cap in caps:
                for env in (a, per):
                    _poison_outputs(env)
                before = rule.stats()
                steps, over = a.rollout_until(TYPES, acts[0], 5, cap, gstep + total, rule)
                after = rule.stats()
                if steps > 0:
                    per.rollout(TYPES, acts[1], steps, gstep + total)
                ctx = f"N={N} threshold {threshold} episode {e} cap {cap}: {steps} steps, over {over}"
                _assert_same_memory(a, per, acts, None, ctx)
                total += steps
                n_long = after["long_launches"] - before["long_launches"]
                n_pairs = after["paired_launches"] - before["paired_launches"]
                assert long or n_long == 0, ctx
                if n_long:
                    assert n_long == 1 and cap > 10, ctx
                    if over and after["in_launch_verdicts"] > before["in_launch_verdicts"]:
                        seen.add("long: verdict behind the second chunk" if steps == 10 else "long: verdict behind a later chunk")
                    if not over and steps == cap:
                        seen.add("long: cap")
                    if cap % 5 and steps >= 20:
                        seen.add("long: cap no multiple of the check interval")
                elif n_pairs:
                    if over and steps % 10 == 5:
                        seen.add("pair: cut at its middle")
                    if steps == cap and cap % 10 == 0:
                        seen.add("pair: ran through")
                    if steps == cap and cap % 5:
                        seen.add("pair: cap no multiple of the check interval")
                if over:
                    break
            gstep += total
        st = rule.stats()
        assert st["called_off"] == 0 and st["verdict_timeouts"] == 0, st
        rule.close()
    want = {"pair: cut at its middle", "pair: ran through", "pair: cap no multiple of the check interval"}
    if long:
        want |= {"long: verdict behind the second chunk", "long: verdict behind a later chunk", "long: cap", "long: cap no multiple of the check interval"}
    assert seen >= want, (sorted(seen), sorted(want - seen))
