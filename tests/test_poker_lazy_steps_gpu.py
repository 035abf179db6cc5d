"""Dead steps of a chunk launch run only the betting state machine and the deal ("lazy steps"): the
equity refresh, the payouts and the clearing of finished tables wait for the next live step.  What a caller can observe must
not change: after every call, with every output word the call does not read poisoned beforehand, memory is bit for bit that of
the same steps taken as single launches -- the yardstick of tests/test_poker_live_outputs_gpu.py, whose helpers these tests
use.  A census taken from a third environment stepped singly shows that the deferred work did happen in the calls compared."""
import numpy as np
import pytest
import torch

from tests.helpers import to_np
from tests.test_poker_gpu_parity import DEV, _gpu_env
from tests.test_poker_live_outputs_gpu import _assert_same_memory, _poison_outputs

pytestmark = pytest.mark.gpu

ACTIVE_ST, ALLIN_ST = 0, 2                                  # include/pulse_env.h
TYPES16 = [0, 3, 2, 2, 4, 3, 1, 4, 5, 3, 1, 2, 3, 4, 5, 1]  # seat 0 external (as in test_poker_live_outputs_gpu)
LENGTHS = tuple(range(1, 13)) + (19,)
FLOORS = {"c1": 10, "c2": 10, "c3": 10, "c4": 10, "c5": 10, "c6": 10, "c7": 10, "c8": 5, "c9": 10}


def _envs(N, P, MP, four, cache, n_envs):
    kw = dict(n_players=P, max_players=MP, n_games=N, w1=.5, w2=.3, K=100, alpha=50, seed=91, table_id0=7)
    envs = [_gpu_env(**kw) for _ in range(n_envs)]
    for env in envs[1:]:
        env.chunked_rollout = False                          # the yardstick and the probe: one launch per step
    envs[0].chunk_four_lanes = four
    for env in envs:
        env.double_buffer_obs = True
        env.use_eval_cache = cache
    return envs


def _probe_state(env):
    return dict(stage=to_np(env.stages).copy(), done=to_np(env.is_done).astype(bool).copy(), inv=to_np(env.total_invested).copy(),
                status=to_np(env.status).copy(), idx=to_np(env.idx).copy(), dirty=to_np(env.equity_dirty).astype(bool).copy())


def _census_of_call(census, probe, types, acts, n, gstep, after_reset, prev_trans):
    """Steps the probe singly through the call's n steps and counts, per table, the events of the classes c1..c9 (the
    module's table below).  Step i of a call of n is dead iff i + 2 < n.  Returns the transition mask of the call's last step."""
    s = _probe_state(probe)
    if n >= 3:
        census["c8"] += 1 if after_reset else 0
        if not after_reset:
            census["c9"] += int((s["dirty"] & ~s["done"]).sum())
    trans_prev_in_call = None
    for i in range(n):
        probe.rollout(types, acts, 1, gstep + i)
        t = _probe_state(probe)
        dead = i + 2 < n
        fin = t["done"] & ~s["done"]
        trans = ~t["done"] & (t["stage"] == s["stage"] + 1) & (t["stage"] >= 1) & (t["stage"] <= 3)
        showdown = fin & (t["stage"] == 5)                    # only the showdown leaves stage 5; a fold-win keeps the stage
        foldwin = fin & (t["stage"] < 5)
        if dead:
            census["c1"] += int(foldwin.sum())
            if trans_prev_in_call is not None:
                census["c2"] += int((showdown & trans_prev_in_call).sum())
                census["c4"] += int((trans & trans_prev_in_call).sum())
            census["c3"] += int((showdown & ~prev_trans).sum())
            if n - 1 - i >= 3:
                census["c5"] += int(fin.sum())
            # commitment levels of the contenders that did not act on this step (their total_invested cannot have changed in
            # it; the finished table's is cleared afterwards): two distinct ones among them are two distinct ones at the showdown
            for g in np.flatnonzero(showdown):
                seats = [k for k in range(t["status"].shape[1]) if t["status"][g, k] in (ACTIVE_ST, ALLIN_ST) and k != (s["idx"][g] & 15)]
                census["c6"] += 1 if len({int(s["inv"][g, k]) for k in seats}) >= 2 else 0
        if i == n - 1:
            census["c7"] += int(trans.sum())
        s, prev_trans, trans_prev_in_call = t, trans, trans
    return prev_trans


# | c1 | fold-win finish on a dead step                                   | c6 | a dead-step showdown with >= 2 commitment levels      |
# | c2 | showdown on a dead step right after a dead-step street transition | c7 | a transition on the call's last step                  |
# | c3 | showdown on a dead step with no transition on the step before     | c8 | a call right after a reset whose first step is dead   |
# | c4 | transitions on two dead steps in a row                            | c9 | a table left dirty by the previous call, first step   |
# | c5 | a finish on a dead step with at least 3 steps of the call to go   |    | of this call dead                                     |
SHAPES = [(64, 10, 10, False, True), (50, 10, 10, False, True), (64, 10, 10, True, True), (48, 12, 12, False, True), (32, 16, 16, False, True),
          (64, 10, 10, False, False)]
IDS = ["64x10-two-lanes-staged", "50x10-ragged-direct-stores", "64x10-four-lanes", "48x12-four-lanes-spl3", "32x16-four-lanes-spl4",
       "64x10-no-eval-cache-walk7"]


@pytest.mark.parametrize("N,P,MP,four,cache", SHAPES, ids=IDS)
def test_deferred_work_leaves_the_memory_of_single_launches(N, P, MP, four, cache):
    """rollout(.., n, ..) as one launch against n single launches, n = 1..12 and 19 forwards then backwards, on poisoned
    outputs: equal bit for bit after every call.  The census (a third environment, stepped singly through the same calls)
    must show every class of deferred work at least 10 times (c8: 5) in the calls compared."""
    one, per, probe = _envs(N, P, MP, four, cache, 3)
    types = TYPES16[:P]
    rng = np.random.default_rng(5)
    census = {k: 0 for k in FLOORS}
    gstep, in_episode, e, prev_trans = 3, None, 0, np.zeros(N, bool)
    for rnd in range(2):
        for n in (LENGTHS if rnd == 0 else LENGTHS[::-1]):
            after_reset = in_episode is None or in_episode > 24
            if after_reset:
                for env in (one, per, probe):
                    env.reset(options={"active_players": (P, P // 2, 3)[e % 3], "rotation": e})
                in_episode, e, prev_trans = 0, e + 1, np.zeros(N, bool)
            ext = torch.from_numpy(rng.integers(0, 13, N)).to(DEV)
            acts = [ext.clone(), ext.clone(), ext.clone()]
            for env in (one, per):
                _poison_outputs(env)
            outs = [env.rollout(types, a, n, gstep) for env, a in zip((one, per), acts)]
            ctx = f"N{N} episode {e} chunk of {n} from step {gstep}"
            _assert_same_memory(one, per, acts[:2], outs, ctx)
            prev_trans = _census_of_call(census, probe, types, acts[2], n, gstep, after_reset, prev_trans)
            np.testing.assert_array_equal(to_np(probe.stages), to_np(per.stages), err_msg=f"{ctx}: the probe left the games")
            gstep += n
            in_episode += n
    print(f"census {IDS[SHAPES.index((N, P, MP, four, cache))]}: {census}")
    assert all(census[k] >= FLOORS[k] for k in FLOORS), census


def test_slim_image_leaves_the_memory_of_single_launches():
    """98,304 x 10 (the slim LDS image: the river's equity from the cached rank in the deferred refresh), lengths 7 and 12,
    two episodes: memory equality only."""
    N, P = 98304, 10
    one, per = _envs(N, P, P, False, True, 2)
    rng = np.random.default_rng(5)
    gstep = 3
    for e in range(2):
        for env in (one, per):
            env.reset(options={"active_players": (P, P // 2)[e], "rotation": e})
        for n in ((7, 12), (12, 7))[e]:
            ext = torch.from_numpy(rng.integers(0, 13, N)).to(DEV)
            acts = [ext.clone(), ext.clone()]
            for env in (one, per):
                _poison_outputs(env)
            outs = [env.rollout(TYPES16[:P], a, n, gstep) for env, a in zip((one, per), acts)]
            _assert_same_memory(one, per, acts, outs, f"slim episode {e} chunk of {n} from step {gstep}")
            gstep += n


@pytest.mark.parametrize("n", [7, 12])
def test_poked_states_leave_the_memory_of_single_launches(n):
    """Nine steps into an episode the same values are poked into both environments: on done tables nonzero bets, investments
    and `highest` with a pot of 11 below stage 5 (cleared on the first live step instead of step 0, no payout, the pot stays),
    a raised equity flag on running tables at stages 1 to 3 and on done tables.  Then one call of n."""
    N, P = 64, 10
    one, per = _envs(N, P, P, False, True, 2)
    types = TYPES16[:P]
    ext = torch.from_numpy(np.random.default_rng(5).integers(0, 13, N)).to(DEV)
    acts = [ext.clone(), ext.clone()]
    for env in (one, per):
        env.reset(options={"active_players": P // 2, "rotation": 0})      # five in the hand: nine steps in, a third of the tables is done
    for env, a in zip((one, per), acts):
        env.rollout(types, a, 9, 3)
    _assert_same_memory(one, per, acts, None, "nine steps in")
    done, stage = to_np(one.is_done).astype(bool), to_np(one.stages)
    done_t = np.flatnonzero(done)
    by_stage = [np.flatnonzero(~done & (stage == st)) for st in (1, 2, 3)]
    assert len(done_t) >= 4 and all(len(x) >= 2 for x in by_stage), (len(done_t), [len(x) for x in by_stage])
    cleared, done_dirty, run_dirty = done_t[0::2], done_t[1::2], np.concatenate([x[0::2] for x in by_stage])
    stacks0 = to_np(one.stacks)[cleared].copy()
    for env in (one, per):
        ix = torch.from_numpy(cleared).to(DEV)
        env.current_round_bet[ix, 1] = 3
        env.current_round_bet[ix, 4] = 7
        env.total_invested[ix, 1] = 5
        env.total_invested[ix, 2] = 9
        env.total_invested[ix, 4] = 9
        env.highest[ix] = 7
        env.pots[ix] = 11
        env.stages[ix] = torch.from_numpy(np.arange(len(cleared)) % 5).to(device=DEV, dtype=torch.int32)
        env.equity_dirty[torch.from_numpy(done_dirty).to(DEV)] = True
        env.equity_dirty[torch.from_numpy(run_dirty).to(DEV)] = True
        _poison_outputs(env)
    outs = [env.rollout(types, a, n, 12) for env, a in zip((one, per), acts)]
    _assert_same_memory(one, per, acts, outs, f"poked, chunk of {n}")
    for env in (one, per):
        assert not to_np(env.current_round_bet)[cleared].any() and not to_np(env.total_invested)[cleared].any()
        assert not to_np(env.highest)[cleared].any()
        assert (to_np(env.pots)[cleared] == 11).all()
        np.testing.assert_array_equal(to_np(env.stacks)[cleared], stacks0)
        np.testing.assert_array_equal(to_np(env.stages)[cleared], np.arange(len(cleared)) % 5)
        assert not to_np(env.equity_dirty)[done_dirty].any()
