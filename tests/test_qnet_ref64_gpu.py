"""The learner's kernels (csrc/qnet.hip) against the float64 reference and its bounds (tests/qnet_ref64.py): Q values
entrywise within the bound, actions by the rules of check_actions, the training step's gradient sum, report and AdamW
step (from the device's own gradient, moments and parameters) within theirs.  The table below names a case for each
branch of launch(), act_rows16_ok() and the training dispatch, and for the trainer's step (act launch + training launch
on the act launch's row lists, fused or not).  Not covered here: a replay of whole episodes of train_agent_fused
against the host oracle (episode sums, stop index, epsilon over many calls).

Inputs: real observation rows of PokerGPU roll-outs (10 seats, state_dim 40; max_players 6, state_dim 28; raw chip counts
in the pot / stack / bet columns, stacks carried over resets) and synthetic extremes (all-zero rows, rows of +-1e4, a row
stride larger than state_dim, a base pointer 4-byte but not 16-byte aligned).

Dispatch table (qnet.hip: launch(), act_call(), act_rows16_ok(), train_launches()); VEC = state_dim % 8 == 0, row stride
% 4 == 0, states and w1 16-byte aligned:
  case                                   branch                                   condition that sends it there
  forward sd 40 / 64 / 128 / 1000 / 4096 qnet_kernel<false, true>                 no seat_idx, VEC
  forward sd 1 / 12 / 13 / 27 / 65 / 100 qnet_kernel<false, false>                no seat_idx, not VEC
  forward sd 40, base + 4 bytes          qnet_kernel<false, false>                states not 16-byte aligned
  act sd 40 / 24, n_actions <= 16        qnet_act_r16_kernel<3, 256>              act_rows16_ok, sd <= 48, n < 1024 CUs
  act sd 64 / 52                         qnet_act_r16_kernel<4, 256>              act_rows16_ok, sd > 48
  act sd 40, 1,024 CUs + 1,000 rows      qnet_act_r16_kernel<3, 1024>             act_rows16_ok, n >= 1024 CUs
  act sd 40, PULSE_ACT_TILES=1           qnet_act4_kernel<true, 128, 5>           tiles, VEC, sd <= 40
  act sd 64, n_actions 17                qnet_act4_kernel<true, 128, 8>           n_actions > 16, VEC, sd > 40
  act sd 28, PULSE_ACT_TILES=1           qnet_act4_kernel<false, 128, 8>          tiles, not VEC (28 % 8 != 0)
  act sd 40, tiles, 262,144 + 77 rows    + qnet_act_rows_kernel<true, 128, 5>     act_select, n >= 262,144, big scratch
  act sd 100 / 128                       qnet_kernel<true, false / true>          seat_idx, sd > 64
  train sd 24 (<= 32)                    qnet_train8_kernel<true, 5>              VEC, sd <= 40; K1 <= 32 epilogue
  train sd 28 (<= 32) / 36               qnet_train8_kernel<false, 8>             not VEC
  train sd 40                            qnet_train8_kernel<true, 5>              VEC, sd <= 40, K1 > 32
  train sd 64                            qnet_train8_kernel<true, 8>              VEC, sd > 40
  train PULSE_TRAIN_WAVES=4 (child)      qnet_train_kernel<·, ·>                  four wavefronts
  train fused / separate_apply           qnet_grad_reduce_kernel<true> / <false> + qnet_adamw_kernel
  train (every case above)               qnet_select_kernel lists (win_shift 8)   select_from_act == 0
  trainer step, act_into(select=True)    act launch's lists (win_shift 7, book)   select_from_act == 1: same states, stride, mask
  trainer step, act_policy_step N 4096   pulse_poker_act_policy_step + book       fits: N % 128 == 0, sd 16..40 % 8 == 0, ...
  trainer step, act_policy_step N 4099   act_into + policy_step fallback          not fits (N % 128 != 0, sd 28)
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import qnet_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIN = (0, 2, 5, 8, 10)
RATIOS = {}


def _record(name, r):
    med, mx = R.ratio_stats(r)
    prev = RATIOS.get(name, (0.0, 0.0))
    RATIOS[name] = (max(prev[0], med), max(prev[1], mx))
    print(f"[ratio] {name}: median {med:.3g} max {mx:.3g}")


def _qnet(sd, na, seed=0, **kw):
    from pulselib_amd.environments.Poker import PokerQNetwork
    torch.manual_seed(seed)
    return PokerQNetwork(None, torch.device(DEV), gamma=.95, update_freq=2, state_dim=sd, action_dim=na, learning_rate=2e-4,
                         weight_decay=1e-5, seed=seed + 100, table_id0=5000, **kw)


def _flat(q, target=False):
    return (q._flat_target if target else q._flat).detach().cpu().numpy().copy()


_OBS = {}


def real_obs(max_players, n_games=2048, steps=6):
    """(states, next_states, rewards, dones) of PokerGPU roll-outs with random actions, stacks carried over 3 resets."""
    key = (max_players, n_games, steps)
    if key not in _OBS:
        from pulselib_amd.environments.Poker import PokerGPU
        dev = torch.device(DEV)
        env = PokerGPU(device=dev, agents=[], n_players=max_players, max_players=max_players, n_games=n_games, starting_bbs=100,
                       max_bbs=1000, w1=.5, w2=.3, K=100, alpha=50)
        g = torch.Generator(device="cpu"); g.manual_seed(max_players)
        S, NS, Rw, D = [], [], [], []
        for ep in range(3):
            decks = (torch.rand((n_games, 52), generator=g).argsort(dim=1) + 1).to(torch.int32)
            obs, _ = env.reset(options={"prefixed_decks": decks})
            for _ in range(steps):
                before = obs.clone()
                obs, rew, done, _, _ = env.step(torch.randint(0, 13, (n_games,), generator=g).to(dev))
                if ep == 2:
                    S.append(before.cpu()); NS.append(obs.clone().cpu()); Rw.append(rew.cpu()); D.append(done.cpu())
        _OBS[key] = tuple(torch.cat(x).numpy() for x in (S, NS, Rw, D))
    return _OBS[key]


def _states(kind, n, sd, seed):
    rng = np.random.default_rng(seed)
    if kind == "real40":
        return real_obs(10)[0][:n]
    if kind == "real28":
        return real_obs(6)[0][:n]
    x = (rng.standard_normal((n, sd)) * 3).astype(np.float32)
    x[:, :min(sd, 4)] *= 100                                          # chip-count-sized columns
    if kind == "extreme":
        x[:5] = 0.0
        x[5:10] = np.where(rng.random((5, sd)) < 0.5, -1e4, 1e4)
    return x


def _device_rows(x, stride_extra=0, misalign=False):
    """x on the GPU as rows of a wider buffer (stride > state_dim) and/or at a base 4 bytes past a 16-byte boundary."""
    n, sd = x.shape
    pad = 1 if misalign else 0
    buf = torch.zeros(n * (sd + stride_extra) + pad + 4, device=DEV)
    view = buf[pad:pad + n * (sd + stride_extra)].view(n, sd + stride_extra)[:, :sd]
    view.copy_(torch.from_numpy(x))
    assert (view.data_ptr() % 16 != 0) == misalign
    return view


def _check_q(q, x, got, name):
    ws, bs = R.split(_flat(q).astype(np.float64), q.state_dim, q.action_dim)
    fw = R.forward(ws, bs, x)
    _record(name, R.assert_within(got, fw["q"], fw["e_q"], name))
    return fw


# ---- forward (pulse_qnet_forward) -------------------------------------------------------------------------------------
FWD = [(1, 1, 1000, "syn"), (12, 2, 33, "syn"), (13, 13, 31, "extreme"), (27, 16, 32, "syn"), (28, 13, 1000, "real28"),
       (40, 13, 1000, "real40"), (40, 17, 1, "syn"), (64, 32, 1000, "extreme"), (65, 13, 33, "syn"), (100, 2, 31, "syn"),
       (128, 1, 1000, "syn"), (1000, 13, 32, "extreme"), (4096, 32, 33, "syn")]


@pytest.mark.parametrize("sd,na,n,kind", FWD)
def test_forward_every_shape_against_float64(sd, na, n, kind):
    q = _qnet(sd, na, seed=sd + na)
    x = _states(kind, n, sd, sd)
    got = q.q_values(torch.from_numpy(x).to(DEV)).cpu().numpy()
    _check_q(q, x, got, f"forward sd{sd} na{na} n{n} {kind}")


@pytest.mark.parametrize("stride_extra,misalign", [(8, False), (3, False), (0, True), (5, True)])
def test_forward_strided_and_misaligned_rows(stride_extra, misalign):
    q = _qnet(40, 13, seed=3)
    x = _states("real40", 1000, 40, 0)
    got = q.q_values(_device_rows(x, stride_extra, misalign)).cpu().numpy()
    _check_q(q, x, got, f"forward stride+{stride_extra} misaligned={misalign}")


# ---- act (pulse_qnet_act / pulse_qnet_act_select) ---------------------------------------------------------------------
def _act(q, x_dev, seat, eps, step, select=False):
    from pulselib_amd import _native
    n = x_dev.shape[0]
    acts = torch.full((n,), -1, dtype=torch.long, device=DEV)
    qrows = torch.zeros((n, q.action_dim), device=DEV)
    net = q._net_struct(q.network)
    st = torch.cuda.current_stream().cuda_stream
    if select:
        q._native_state(n)
        scratch = q._native["select"]
        mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
        _native.check(_native.lib().pulse_qnet_act_select(C.byref(net), x_dev.data_ptr(), x_dev.stride(0), n, seat.data_ptr(), 2, float(eps),
                                                          q.seed, step, q.table_id0, acts.data_ptr(), None, mask.data_ptr(),
                                                          scratch.data_ptr(), scratch.numel(), st), "pulse_qnet_act_select")
        return acts.cpu().numpy(), None
    _native.check(_native.lib().pulse_qnet_act(C.byref(net), x_dev.data_ptr(), x_dev.stride(0), n, seat.data_ptr(), 2, float(eps), q.seed,
                                               step, q.table_id0, acts.data_ptr(), qrows.data_ptr(), None, None, st), "pulse_qnet_act")
    return acts.cpu().numpy(), qrows.cpu().numpy()


ACT = [  # (sd, na, n, kind, tiles, select, eps)
    (40, 13, 5000, "real40", "0", False, 0.0), (40, 13, 5000, "real40", "0", True, 0.3), (24, 13, 700, "syn", "0", False, 1.0),
    (64, 13, 3000, "extreme", "0", False, 0.3), (52, 16, 700, "syn", "0", True, 0.0),
    (40, 13, "wide", "syn", "0", True, 0.3),
    (40, 13, 3000, "real40", "1", False, 0.3), (64, 17, 3000, "syn", "0", False, 0.0), (28, 13, 3000, "real28", "1", True, 0.3),
    (40, 13, 262144 + 77, "syn", "1", True, 0.3),
    (100, 13, 1000, "syn", "0", False, 0.3), (128, 32, 1000, "extreme", "0", False, 0.0)]


@pytest.mark.parametrize("sd,na,n,kind,tiles,select,eps", ACT)
def test_act_every_branch_against_float64(sd, na, n, kind, tiles, select, eps, monkeypatch):
    monkeypatch.setenv("PULSE_ACT_TILES", tiles)
    if n == "wide":                                                   # the 1,024-row windows: n_rows >= 1024 * CUs (launch())
        n = 1024 * torch.cuda.get_device_properties(0).multi_processor_count + 1000
    q = _qnet(sd, na, seed=sd * 7 + na)
    if n > 100_000:
        base = _states(kind, 4096, sd, 5)
        x = base[np.arange(n) % 4096]                                 # a large batch of repeated rows: the reference runs once
    else:
        x = _states(kind, n, sd, 5)
    rng = np.random.default_rng(n)
    seat_np = rng.integers(0, 4, n).astype(np.int32)
    seat = torch.from_numpy(seat_np).to(DEV)
    step = 31 + n
    got, qrows = _act(q, torch.from_numpy(x).to(DEV), seat, eps, step, select)
    mine = np.flatnonzero(seat_np == 2)
    assert (got[seat_np != 2] == -1).all()
    ws, bs = R.split(_flat(q).astype(np.float64), sd, na)
    check = mine if n <= 100_000 else mine[rng.choice(mine.size, 4096, replace=False)]
    fw = R.forward(ws, bs, x[check])
    if qrows is not None:
        _record(f"act Q sd{sd} na{na}", R.assert_within(qrows[check], fw["q"], fw["e_q"], "act Q rows"))
    ex, un = R.explore_draws(n, na, eps, q.seed, step, q.table_id0)
    exact = R.check_actions(got[check], fw["q"], fw["e_q"], ex[check], un[check], ctx=f"act sd{sd} na{na} n{n}")
    if eps < 1.0 and na > 1:
        assert exact > 0.8 * (~ex[check]).sum()
    if eps == 1.0:
        assert ex[check].all()


@pytest.mark.parametrize("tiles", ["0", "1"])
def test_act_exact_tie_takes_the_lower_index(tiles, monkeypatch):
    monkeypatch.setenv("PULSE_ACT_TILES", tiles)
    q = _qnet(40, 13, seed=9)
    with torch.no_grad():
        w5, b5 = q.network[10].weight, q.network[10].bias
        w5[7].copy_(w5[2]); b5[2] = 5.0; b5[7] = 5.0
    x = _states("real40", 2000, 40, 1)
    seat = torch.full((2000,), 2, dtype=torch.int32, device=DEV)
    got, qrows = _act(q, torch.from_numpy(x).to(DEV), seat, 0.0, 3)
    assert np.array_equal(qrows[:, 2], qrows[:, 7]), "premise: identical W5 rows give bit-equal Q"
    top = qrows.max(axis=1)
    assert (qrows[:, 2] == top).all(), "premise: the tied pair is the maximum"
    assert (got == 2).all()


# ---- training (train_step_native) -------------------------------------------------------------------------------------
def _train_batch(kind, n, sd, na, seed, valid=None):
    rng = np.random.default_rng(seed)
    if kind.startswith("real"):
        S, NS, Rw, D = real_obs(10 if sd == 40 else 6)
        idx = rng.choice(S.shape[0], n, replace=n > S.shape[0])
        s, ns, r, d = S[idx].copy(), NS[idx].copy(), Rw[idx].copy(), D[idx] | (rng.random(n) < 0.2)
    else:
        s = (rng.standard_normal((n, sd)) * 0.05).astype(np.float32)
        ns = (rng.standard_normal((n, sd)) * 0.05).astype(np.float32)
        r = (rng.standard_normal(n) * 0.01).astype(np.float32); d = rng.random(n) < 0.3
        s[:, 12] = rng.integers(0, 4, n)
    mask = rng.random(n) < 0.8
    if valid is not None:
        s[:, 12] = 1.0
        s[:valid, 12] = 0.0
        mask[:] = True
    return dict(states=s, actions=rng.integers(0, na, n).astype(np.int64), rewards=r.astype(np.float32), next_states=ns,
                dones=d, row_mask=mask)


def _pre(q):
    """The learner's state before an update: parameters, target, moments, optimizer step."""
    nat = q._native
    return _flat(q), _flat(q, True), nat["m"].cpu().numpy().copy(), nat["v"].cpu().numpy().copy(), int(nat["step"].item())


def _check_update(q, pre, b, rep, step_counter, ctx, label):
    """One native update against the reference: row count, gradient sum, loss, norm; AdamW from the device's own gradient;
    target sync.  Returns the reference's train_grads (None when nothing was valid)."""
    p0, tp0, m0, v0, t0 = pre
    nat = q._native
    ref = R.train_grads(p0, tp0, q.state_dim, q.action_dim, b["states"], b["actions"], b["rewards"], b["next_states"], b["dones"],
                        b["row_mask"], 0.95, 0.1 if q.network.training else 0.0, q.seed, step_counter, q.table_id0)
    assert rep[0] == ref["count"], ctx + " row count"
    t = int(nat["step"].item())
    if ref["count"] == 0:
        assert t == t0 and np.array_equal(_flat(q), p0) and np.array_equal(_flat(q, True), tp0), ctx + ": no valid row, nothing moves"
        return None
    assert t == t0 + 1
    G = nat["grad"].cpu().numpy().copy()
    _record(f"train gradient {label}", R.assert_within(G, ref["grad"], ref["e_grad"], ctx + " gradient sum"))
    R.assert_within(rep[1], ref["loss"], ref["e_loss"], ctx + " loss")
    R.assert_within(rep[2], ref["norm"], ref["e_norm"], ctx + " gradient norm")
    ad = R.adamw(p0, tp0, G, m0, v0, int(rep[0]), t, q.lr, q.wd, update_freq=q.update_freq)
    _record(f"train params {label}", R.assert_within(_flat(q), ad["params"], ad["e_params"], ctx + " parameters"))
    R.assert_within(nat["m"].cpu().numpy(), ad["m"], ad["e_m"], ctx + " exp_avg")
    R.assert_within(nat["v"].cpu().numpy(), ad["v"], ad["e_v"], ctx + " exp_avg_sq")
    if ad["synced"]:
        assert np.array_equal(_flat(q, True), _flat(q)), ctx + " target sync"
    else:
        assert np.array_equal(_flat(q, True), tp0), ctx + " target untouched"
    return ref


def _train_and_check(q, b, steps=3, label=""):
    for it in range(steps):
        q._native_state(b["states"].shape[0])
        pre = _pre(q)
        dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
        rep = q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"],
                                  step_counter=700 + it).cpu().numpy().copy()
        assert q._struct_cache["train"].select_from_act == 0
        ref = _check_update(q, pre, b, rep, 700 + it, f"{label} step {it}", label)
        if ref is not None:
            yield ref, rep


TRAIN = [  # (sd, na, n, kind, valid, separate, dropout)
    (40, 13, 4000, "real40", None, False, True), (28, 13, 4000, "real28", None, True, True), (24, 1, 1500, "syn", None, False, True),
    (36, 32, 1500, "syn", None, False, False), (64, 13, 37, "syn", None, True, True), (28, 32, 1500, "syn", None, False, True),
    (40, 13, 300, "syn", 0, False, True), (40, 13, 300, "syn", 1, False, True), (40, 13, 70001, "real40", None, False, True)]


@pytest.mark.parametrize("sd,na,n,kind,valid,separate,drop", TRAIN)
def test_training_every_branch_against_float64(sd, na, n, kind, valid, separate, drop):
    q = _qnet(sd, na, seed=sd + 3 * na)
    q.separate_apply = separate
    if not drop:
        q.network.eval()
    b = _train_batch(kind, n, sd, na, seed=n + sd, valid=valid)
    # (the float64 bound of 70,001 rows takes about a minute of CPU: one step there, three elsewhere)
    for ref, rep in _train_and_check(q, b, steps=1 if n > 10_000 else 3, label=f"sd{sd} na{na} n{n} {kind}"):
        if kind.startswith("real"):
            assert ref["norm"] > 1.0, "real observations: the clipped regime"
        elif valid is None:
            assert ref["norm"] < 1.0, "small inputs: the unclipped regime"


@pytest.mark.parametrize("N,P,fused", [(4096, 10, True), (4096, 10, False), (4099, 6, True)])
def test_trainer_step_with_act_lists_against_float64(N, P, fused):
    """The trainer's own sequence (scripts/trainGPU.py, native branch): act_policy_step (fused=True; with N % 128 != 0 or
    state_dim 28 it falls back to the two calls) or act_into(select_for_training=True) + policy_step, then train_step_native
    on the lists the act launch wrote (select_from_act: win_shift 7, row_mask / terminated / reward_sum folded into the
    training launch).  Per step: the trainer's mask is (seat_idx == q_seat) & ~terminated taken before the update; the
    learner's actions follow the float64 reference on the pre-step parameters; state_before is the double-buffered
    observation the step did not overwrite; the update matches the reference on that observation, the device's actions,
    rewards, next observation, dones and the mask, with global_step as the dropout key; terminated |= dones; reward_sum
    grows by the mask rows' rewards."""
    from pulselib_amd.environments.Poker import PokerGPU
    dev = torch.device(DEV)
    sd, q_tid = 13 + 3 * (P - 1), 9000
    env = PokerGPU(device=dev, agents=[], n_players=P, max_players=P, n_games=N, starting_bbs=100, max_bbs=1000, w1=.5, w2=.3,
                   K=100, alpha=50, seed=77, table_id0=q_tid)
    env.double_buffer_obs = True
    q = _qnet(sd, 13, seed=21)
    q.table_id0 = q_tid
    q.epsilon = q.epsilon_end = 0.3
    q_seat = 3                                                         # first to act after the first reset (button 0, blinds 1, 2)
    types = [3, 1, 2, 4, 5, 3, 1, 2, 4, 5][:P]
    types[q_seat] = 0                                                  # PULSE_AGENT_EXTERNAL: the learner's seat
    g = torch.Generator(device="cpu"); g.manual_seed(N + P)
    decks = (torch.rand((N, 52), generator=g).argsort(dim=1) + 1).to(torch.int32)
    states, info = env.reset(options={"active_players": P, "q_agent_seat": q_seat, "prefixed_decks": decks})
    actions = torch.zeros(N, dtype=torch.long, device=dev)
    term = torch.zeros(N, dtype=torch.bool, device=dev)
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    acc = torch.zeros((), dtype=torch.float64, device=dev)
    q._native_state(N)
    trained = 0
    for gstep in range(14):
        ctx = f"N={N} P={P} fused={fused} step {gstep}"
        S = states.cpu().numpy().copy()
        seat = info["seat_idx"].cpu().numpy().copy()
        term0 = term.cpu().numpy().copy()
        pre = _pre(q)
        acc0 = float(acc)
        if fused:
            out = env.act_policy_step(q, q_seat, types, actions, gstep, states, info["seat_idx"], term, mask)
        else:
            q.act_into(states, info["seat_idx"], q_seat, actions, step_counter=gstep, terminated=term, row_mask_out=mask,
                       select_for_training=True)
            out = env.policy_step(types, actions, gstep)
        next_states, rewards, dones = out[0], out[1], out[2]
        assert next_states.data_ptr() != states.data_ptr()
        assert np.array_equal(states.cpu().numpy(), S), ctx + ": the step overwrote state_before"
        m = mask.cpu().numpy()
        assert np.array_equal(m, (seat == q_seat) & ~term0), ctx + " trainer mask"
        a = actions.cpu().numpy()
        mine = np.flatnonzero(seat == q_seat)
        ws, bs = R.split(pre[0].astype(np.float64), sd, 13)
        fw = R.forward(ws, bs, S[mine])
        ex, un = R.explore_draws(N, 13, q.epsilon, q.seed, gstep, q.table_id0)
        R.check_actions(a[mine], fw["q"], fw["e_q"], ex[mine], un[mine], ctx=ctx + " actions")
        b = dict(states=S, actions=a, rewards=rewards.cpu().numpy().copy(), next_states=next_states.cpu().numpy().copy(),
                 dones=dones.cpu().numpy().copy(), row_mask=m)
        rep = q.train_step_native(states, actions, rewards, next_states, dones, mask, step_counter=gstep, terminated=term,
                                  reward_sum=acc).cpu().numpy().copy()
        assert q._struct_cache["train"].select_from_act == 1, ctx + ": the training launch did not take the act launch's lists"
        ref = _check_update(q, pre, b, rep, gstep, ctx, f"trainer step N{N} P{P} fused={fused}")
        trained += ref is not None
        assert np.array_equal(term.cpu().numpy(), term0 | b["dones"]), ctx + " terminated |= dones"
        r_m = b["rewards"][m].astype(np.float64)
        R.assert_within(float(acc) - acc0, r_m.sum(), R.gam(max(r_m.size, 1)) * np.abs(r_m).sum()        # the fp32 partial sums
                        + 2.0 ** -52 * (abs(acc0) + np.abs(r_m).sum()), ctx + " reward_sum")                  # their float64 accumulation
        states, info = next_states, out[4]
    assert trained >= 3
    assert q.native_steps() == trained


def test_four_wavefront_training_kernel_against_float64(tmp_path):
    root = Path(__file__).resolve().parent.parent
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_qnet_ref64_gpu as T\n"
            "q = T._qnet(40, 13, seed=4); b = T._train_batch('real40', 3000, 40, 13, 5)\n"
            "n = sum(1 for _ in T._train_and_check(q, b, label='four waves'))\n"
            "assert n == 3, n\n"
            "q = T._qnet(28, 13, seed=5); b = T._train_batch('syn', 1000, 28, 13, 6)\n"
            "assert sum(1 for _ in T._train_and_check(q, b, label='four waves sd28')) == 3\n"
            "print('ok')\n") % str(root)
    env = dict(os.environ, PULSE_TRAIN_WAVES="4")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=str(root), timeout=110, capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-3000:]


# ---- the reference signature's returned loss --------------------------------------------------------------------------
def test_train_step_returns_its_own_loss():
    """PokerQNetwork.train_step keeps the loss of each call (the report buffer is shared by every call); step_count counts
    the calls with a valid row; a batch without rows, or without a valid row, returns 0 without launching anything and
    without counting a step (Player.py:261-262)."""
    q = _qnet(40, 13, seed=12)
    q.network.eval()
    losses, refs = [], []
    for it in range(3):
        b = _train_batch("syn", 500, 40, 13, seed=40 + it)
        b["states"][:, 12] = 0.0
        p0, tp0 = _flat(q), _flat(q, True)
        dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
        losses.append(q.train_step(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"]))
        refs.append(R.train_grads(p0, tp0, 40, 13, b["states"], b["actions"], b["rewards"], b["next_states"], b["dones"], None, 0.95, 0.0))
    for i, (l, ref) in enumerate(zip(losses, refs)):
        R.assert_within(float(l), ref["loss"], ref["e_loss"], f"loss of call {i}")
    steps, calls = q.step_count, q._calls
    empty = torch.zeros((0, 40), device=DEV)
    z = q.train_step(empty, torch.zeros(0, dtype=torch.long, device=DEV), torch.zeros(0, device=DEV), empty,
                     torch.zeros(0, dtype=torch.bool, device=DEV))
    assert float(z) == 0.0 and q.step_count == steps and q._calls == calls
    assert steps == 3
    dead = _train_batch("syn", 200, 40, 13, seed=9)                  # rows, but every seat folded or sitting out (:261-262)
    dead["states"][:, 12] = np.where(np.arange(200) % 2 == 0, 1.0, 3.0)
    dv = {k: torch.from_numpy(x).to(DEV) for k, x in dead.items()}
    before = _flat(q)
    z = q.train_step(dv["states"], dv["actions"], dv["rewards"], dv["next_states"], dv["dones"])
    assert float(z) == 0.0 and q.step_count == steps and q._calls == calls and np.array_equal(_flat(q), before)
    R.assert_within(float(losses[-1]), refs[-1]["loss"], refs[-1]["e_loss"], "the last loss after an empty call")


def test_zz_report_ratio_statistics():
    for k, (med, mx) in sorted(RATIOS.items()):
        print(f"[ratio summary] {k}: median {med:.3g} max {mx:.3g}")
