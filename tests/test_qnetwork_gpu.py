"""Learner, GPU side: the MFMA action-selection kernel (csrc/qnet.hip, through the C ABI) against
the reference's recorded Q values (tests/golden/qnetwork.npz) and the oracle (oracle/qnet_oracle.c).
Floating point: the kernel, torch and the oracle sum fp32 products in different orders; Q values are compared with
atol = Q_TOL (|Q| is O(1) for these weights), actions exactly -- derived from the kernel's own Q rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_qnetwork_cpu import LINEARS, Q_TOL, weights_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(golden_dir / "qnetwork.npz")


def _qnet(g, case, **kw):
    from pulselib_amd.environments.Poker import PokerQNetwork
    state_dim = g[f"{case}/states"].shape[1]
    q = PokerQNetwork(None, torch.device(DEV), gamma=.95, update_freq=20, state_dim=state_dim, action_dim=13,
                      learning_rate=2e-4, weight_decay=1e-5, **kw)
    q.network.load_state_dict({k.split("/")[-1]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{case}/w0/")})
    q.target_network.load_state_dict(q.network.state_dict())
    return q


@pytest.mark.parametrize("case", ["s40", "s27"])
def test_hip_forward_matches_reference_and_oracle(g, case):
    from oracle import oracle as orc
    q = _qnet(g, case)
    states = torch.from_numpy(g[f"{case}/states"]).to(DEV)
    got = q.q_values(states).cpu().numpy()
    np.testing.assert_allclose(got, g[f"{case}/q"], rtol=0, atol=Q_TOL)                       # the reference's own outputs
    w, b = weights_of(g, case, "w0")
    np.testing.assert_allclose(got, orc.qnet_forward(w, b, g[f"{case}/states"]), rtol=0, atol=Q_TOL)
    with torch.no_grad():                                                                      # torch fp32 on the same GPU
        q.network.eval()
        ref = q.network(states).cpu().numpy()
        q.network.train()
    np.testing.assert_allclose(got, ref, rtol=0, atol=Q_TOL)
    # rows inside a wider buffer (row stride > state_dim), as the env's observation rows would be with more columns
    wide = torch.zeros((states.shape[0], states.shape[1] + 8), device=DEV)
    wide[:, :states.shape[1]] = states
    np.testing.assert_array_equal(q.q_values(wide[:, :states.shape[1]]).cpu().numpy(), got)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 65536])
def test_hip_forward_row_counts_and_large_batch(n):
    from oracle import oracle as orc
    from pulselib_amd.environments.Poker import PokerQNetwork
    torch.manual_seed(n)
    q = PokerQNetwork(None, torch.device(DEV), gamma=.95, update_freq=20, state_dim=40)
    states = (torch.randn((n, 40)) * 4).round()                      # observation-like magnitudes
    got = q.q_values(states.to(DEV)).cpu().numpy()
    w = [q.network[i].weight.detach().cpu().numpy() for i in LINEARS]
    b = [q.network[i].bias.detach().cpu().numpy() for i in LINEARS]
    np.testing.assert_allclose(got, orc.qnet_forward(w, b, states.numpy()), rtol=0, atol=Q_TOL)


@pytest.mark.parametrize("eps,case", [(0.0, "s40"), (0.3, "s40"), (1.0, "s40"), (0.3, "s27")])
def test_hip_act_matches_oracle_and_leaves_other_seats_alone(g, eps, case):
    from oracle import oracle as orc
    from pulselib_amd import _native
    q = _qnet(g, case, seed=4242, table_id0=10_000_000_000)
    n, sd = 5000, q.state_dim
    rng = np.random.default_rng(5)
    states = torch.from_numpy((rng.standard_normal((n, sd)) * 3).astype(np.float32)).to(DEV)
    seat = torch.from_numpy(rng.integers(0, 10, n).astype(np.int32)).to(DEV)
    seat[64:192] = 3            # a full and an empty wavefront window
    seat[192:256] = 4
    actions = torch.full((n,), -5, dtype=torch.long, device=DEV)
    qrows = torch.zeros((n, 13), device=DEV)
    term = torch.from_numpy(rng.random(n) < 0.25).to(DEV)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    net = q._net_struct(q.network)
    _native.check(_native.lib().pulse_qnet_act(C.byref(net), states.data_ptr(), sd, n, seat.data_ptr(), 3, eps, 4242, 77,
                                               10_000_000_000, actions.data_ptr(), qrows.data_ptr(), term.data_ptr(), mask.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "pulse_qnet_act")
    np.testing.assert_array_equal(mask.cpu().numpy().astype(bool), (seat.cpu().numpy() == 3) & ~term.cpu().numpy().astype(bool))
    sel = seat.cpu().numpy() == 3
    got = actions.cpu().numpy()
    assert (got[~sel] == -5).all() and sel.sum() > 400
    full = q.q_values(states).cpu().numpy()
    mine = qrows.cpu().numpy()
    # the masked kernel splits the k range of layers 3 and 4 over wavefronts: same values up to summation order
    np.testing.assert_allclose(mine[sel], full[sel], rtol=0, atol=Q_TOL)
    assert (mine[~sel] == 0).all()
    want = np.full(n, -5, dtype=np.int64)
    orc.qnet_act(mine, seat.cpu().numpy(), 3, eps, 4242, 77, 10_000_000_000, want)    # actions follow the kernel's own Q rows
    np.testing.assert_array_equal(got, want)
    if eps == 1.0:
        counts = np.bincount(got[sel], minlength=13)
        assert counts.min() > 0.5 * sel.sum() / 13


def test_get_actions_and_build_actions_fused_path(g):
    """get_actions on a dense batch (reference contract) and build_actions with the learner seated: scripted seats by
    the policy kernel, the learner's rows by act_into, every table gets exactly one writer."""
    from oracle import oracle as orc
    from pulselib_amd.environments.Poker import PokerGPU, build_actions, load_gpu_agents
    from pulselib_amd.environments.Poker.utils import PokerAgentType
    q = _qnet(g, "s40", seed=9)
    q.epsilon, q.epsilon_end = 0.0, 0.0
    states = torch.from_numpy(g["s40/states"]).to(DEV)
    acts = q.get_actions(states).cpu().numpy()
    top2 = np.sort(g["s40/q"], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 4 * Q_TOL
    np.testing.assert_array_equal(acts[clear], g["s40/greedy"][clear])            # the reference's greedy picks

    dev = torch.device(DEV)
    names = ["tight_aggressive", "heuristic_hands", "loose_passive", "random", "small_ball"]
    agents, types = load_gpu_agents(dev, 5, names, 100, 13)
    agents.insert(3, q)                       # seat 3 opens the betting after a first reset (button 0, blinds 1 and 2)
    types.insert(3, PokerAgentType.QLEARNING)
    env = PokerGPU(device=dev, agents=agents, n_players=6, max_players=10, n_games=4096, seed=1)
    state, info = env.reset(options={"active_players": 6})
    actions = torch.full((4096,), -9, dtype=torch.long, device=dev)
    build_actions(state, actions, info["seat_idx"], agents, types, dev)
    a = actions.cpu().numpy()
    assert ((a >= 0) & (a < 13)).all()
    mine = info["seat_idx"].cpu().numpy() == 3
    assert mine.all()
    for _ in range(12):                       # play on until the tables wait on different seats, the learner's among them
        state, _, _, _, info = env.step(actions)
        actions.fill_(-9)
        build_actions(state, actions, info["seat_idx"], agents, types, dev)
        mine = info["seat_idx"].cpu().numpy() == 3
        if 0 < mine.sum() < 4096:
            break
    a = actions.cpu().numpy()
    assert ((a >= 0) & (a < 13)).all()
    assert 0 < mine.sum() < 4096
    qv = q.q_values(state).cpu().numpy()
    top2 = np.sort(qv, axis=1)[:, -2:]
    clear = mine & ((top2[:, 1] - top2[:, 0]) > 4 * Q_TOL)
    assert clear.sum() > 0.5 * mine.sum() > 0
    np.testing.assert_array_equal(a[clear], qv.argmax(axis=1)[clear])


def test_train_step_masked_equals_filtered_train_step(g):
    """With dropout off (eval) the 0/1-weighted update equals the reference's filtered update; an all-invalid batch
    leaves the weights where they were."""
    qa, qb = _qnet(g, "s40"), _qnet(g, "s40")
    qa.network.eval(); qb.network.eval()
    t = {k: torch.from_numpy(g[f"s40/{k}"]).to(DEV) for k in ("states", "next_states", "actions", "rewards", "dones")}
    row_mask = torch.arange(t["states"].shape[0], device=DEV) % 2 == 0
    for _ in range(3):
        la = qa.train_step_torch(states=t["states"][row_mask], actions=t["actions"][row_mask], rewards=t["rewards"][row_mask],
                                 next_states=t["next_states"][row_mask], dones=t["dones"][row_mask])
        lb = qb.train_step_masked(t["states"], t["actions"], t["rewards"], t["next_states"], t["dones"], row_mask)
        assert abs(float(la) - float(lb)) < 1e-4 * max(1.0, abs(float(la)))
    for (k, va), vb in zip(qa.network.state_dict().items(), qb.network.state_dict().values()):
        np.testing.assert_allclose(va.cpu().numpy(), vb.cpu().numpy(), rtol=0, atol=2e-5, err_msg=k)
    before = {k: v.clone() for k, v in qb.network.state_dict().items()}
    qb.train_step_masked(t["states"], t["actions"], t["rewards"], t["next_states"], t["dones"], torch.zeros_like(row_mask))
    for k, v in qb.network.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_fused_trainer_loop_runs_and_learns_something(g):
    """train_agent_fused end to end on a small batch: step accounting as trainGPU.py:108, the learner's weights move,
    every transition fed to the learner is one where the learner's seat acted on a live table."""
    from pulselib_amd.environments.Poker import PokerGPU, load_gpu_agents
    from pulselib_amd.environments.Poker.utils import PokerAgentType
    from pulselib_amd.scripts.trainGPU import train_agent_fused
    dev = torch.device(DEV)
    names = ["tight_aggressive", "heuristic_hands", "loose_passive", "random", "small_ball"]
    agents, types = load_gpu_agents(dev, 5, names, 100, 13)
    q = _qnet(g, "s40", seed=3)
    agents.insert(0, q)
    types.insert(0, PokerAgentType.QLEARNING)
    N = 2048
    env = PokerGPU(device=dev, agents=agents, n_players=6, max_players=10, n_games=N, seed=11)
    w0 = q.network[0].weight.detach().clone()
    seen = {"rows": 0, "bad": 0, "steps": 0}

    def hook(episode, idx, state_before, actions, rewards, next_state, dones, active):
        seen["steps"] += 1
        seen["rows"] += int(active.sum())
        a = actions[active]
        seen["bad"] += int(((a < 0) | (a > 12)).sum())
        # the learner's own seat is the one to act in every transition it learns from: relative position column 8
        # of the pre-step observation identifies the actor's offset from the button, status column 12 is the actor's
        assert state_before.shape == (N, 40)

    out = train_agent_fused(env, agents, types, episodes=3, n_games=N, device=dev, max_episode_steps=30, reduce_stats=False,
                            stop_rule="sync", step_hook=hook)
    assert out["total_steps"] % N == 0 and out["total_steps"] > 0
    assert out["env_step_calls"] == seen["steps"] and seen["rows"] > 0 and seen["bad"] == 0
    assert q.step_count == seen["steps"]
    assert not torch.equal(q.network[0].weight.detach(), w0)
    assert len(out["episode_rewards"]) == 3 and all(np.isfinite(out["episode_rewards"]))


# ---- native training step (pulse_qnet_train_step) ------------------------------------------------------------
GRAD_RTOL = 2e-5      # fp32 sums of a few hundred products in a different order (atomics), relative to the largest entry
# AdamW moves every parameter by about lr * m / (sqrt(v) + eps): where a gradient entry is within a few orders of eps
# (1e-8) the quotient amplifies rounding-level differences of the gradient sum, so parameters are compared to 5 % of
# one learning-rate step (lr = 2e-4), far below any real discrepancy (a wrong gradient sign moves a parameter by 2 lr).
PARAM_ATOL = 1e-5


def _flat(net):
    return np.concatenate([np.concatenate([net[i].weight.detach().cpu().numpy().ravel(), net[i].bias.detach().cpu().numpy().ravel()])
                           for i in LINEARS]).astype(np.float32)


def _batch(n, seed, state_dim=40):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((n, state_dim)) * 2).astype(np.float32)
    s[:, 12] = rng.integers(0, 4, n)
    ns = (rng.standard_normal((n, state_dim)) * 2).astype(np.float32)
    return dict(states=s, next_states=ns, actions=rng.integers(0, 13, n).astype(np.int64),
                rewards=(rng.standard_normal(n) * 3).astype(np.float32), dones=rng.random(n) < 0.3, row_mask=rng.random(n) < 0.6)


@pytest.mark.parametrize("n,drop,case", [(1000, True, "s40"), (1000, False, "s40"), (37, True, "s40"), (70000, True, "s40"),
                                         (1500, True, "s27")])
def test_native_train_step_matches_oracle(g, n, drop, case):
    """Three native updates against the oracle's scalar restatement (same dropout draws, same AdamW arithmetic):
    row count, loss, gradient norm and the parameters after every step; target sync at update_freq."""
    from oracle import oracle as orc
    q = _qnet(g, case, seed=77, table_id0=5_000_000_000)        # s27: the scalar-load (unaligned state_dim) variants of the kernels
    sd = q.state_dim
    q.update_freq = 2
    if not drop:
        q.network.eval()
    p = _flat(q.network); tp = p.copy()
    m = np.zeros_like(p); v = np.zeros_like(p)
    t_opt = 0
    for it in range(3):
        b = _batch(n, 100 * n + it, sd)
        if it == 2:
            b["row_mask"][:] = False                       # nothing valid: the step must be a no-op
        dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
        rep = q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"],
                                  step_counter=900 + it).cpu().numpy().copy()
        grad, cnt, sq = orc.qnet_train_grads(p, tp, b["states"], b["actions"], b["rewards"], b["next_states"], b["dones"], b["row_mask"],
                                             0.95, 0.1 if drop else 0.0, 77, 900 + it, 5_000_000_000)
        assert rep[0] == cnt
        if cnt:
            t_opt += 1
            norm = orc.qnet_adamw(p, tp, grad, m, v, cnt, t_opt, 2e-4, 1e-5, update_freq=2)
            assert abs(rep[1] - sq / cnt) <= 1e-4 * max(1.0, sq / cnt)
            assert abs(rep[2] - norm) <= 1e-4 * max(1.0, norm)
        np.testing.assert_allclose(_flat(q.network), p, rtol=0, atol=PARAM_ATOL, err_msg=f"parameters after step {it}")
        np.testing.assert_allclose(_flat(q.target_network), tp, rtol=0, atol=PARAM_ATOL, err_msg=f"target after step {it}")
        p[:] = _flat(q.network); tp[:] = _flat(q.target_network)      # follow the device so that rounding does not accumulate
    assert q.native_steps() == t_opt == 2
    assert np.abs(_flat(q.target_network) - _flat(q.network)).max() == 0        # synced at optimizer step 2


def test_native_gradient_matches_oracle_and_torch_autograd(g):
    """The raw gradient (before mean / clip / AdamW) of one batch: native kernel vs oracle vs torch autograd of the
    reference's loss (dropout off so that torch can be compared)."""
    from oracle import oracle as orc
    q = _qnet(g, "s40", seed=5)
    q.network.eval()
    n = 3000
    b = _batch(n, 42)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    t = q._native_state()
    t.lr, t.weight_decay = 0.0, 0.0                      # keep the parameters: only the gradient path is looked at
    p0 = _flat(q.network)
    from pulselib_amd import _native
    nat = q._native
    # run only the compaction + gradient kernels' effect: take the gradient by differencing is not possible with lr=0,
    # so read the flat gradient through a zero-lr step that leaves exp_avg = (1-beta1) * clipped mean gradient
    _native.check(_native.lib().pulse_qnet_train_step(C.byref(t), dev["states"].data_ptr(), 40, dev["actions"].data_ptr(),
                                                      dev["rewards"].data_ptr(), dev["next_states"].data_ptr(), 40,
                                                      dev["dones"].view(torch.uint8).data_ptr(), dev["row_mask"].view(torch.uint8).data_ptr(),
                                                      n, 5, 1, 0, None, None, torch.cuda.current_stream().cuda_stream), "pulse_qnet_train_step")
    rep = nat["report"].cpu().numpy()
    grad, cnt, sq = orc.qnet_train_grads(p0, p0, b["states"], b["actions"], b["rewards"], b["next_states"], b["dones"], b["row_mask"],
                                         0.95, 0.0, 5, 1, 0)
    mean_grad = grad / cnt
    norm = float(np.sqrt((mean_grad.astype(np.float64) ** 2).sum()))
    coef = min(1.0, 1.0 / (norm + 1e-6))
    got = nat["m"].cpu().numpy() / (1 - 0.9)             # exp_avg after the first step = (1 - beta1) * clipped gradient
    np.testing.assert_allclose(got, mean_grad * coef, rtol=0, atol=GRAD_RTOL * np.abs(mean_grad * coef).max())
    assert rep[0] == cnt and abs(rep[2] - norm) < 1e-4 * norm
    np.testing.assert_array_equal(_flat(q.network), p0)
    # torch autograd on the reference's loss
    valid = dev["row_mask"] & ((dev["states"][:, 12] == 0) | (dev["states"][:, 12] == 2))
    qa = q.network(dev["states"][valid]).gather(1, dev["actions"][valid].unsqueeze(1)).squeeze(1)
    with torch.no_grad():
        tgt = dev["rewards"][valid] + 0.95 * q.target_network(dev["next_states"][valid]).max(dim=1).values * (~dev["dones"][valid]).float()
    loss = torch.nn.functional.mse_loss(qa, tgt)
    q.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    tg = np.concatenate([np.concatenate([q.network[i].weight.grad.cpu().numpy().ravel(), q.network[i].bias.grad.cpu().numpy().ravel()])
                         for i in LINEARS])
    np.testing.assert_allclose(mean_grad, tg, rtol=0, atol=GRAD_RTOL * np.abs(tg).max())
    assert abs(float(loss) - rep[1]) < 1e-4 * max(1.0, float(loss))


def test_reference_signature_train_step_runs_the_native_kernels(g):
    """PokerQNetwork.train_step(states, actions, rewards, next_states, dones) (Player.py:255-294) on a GPU module IS the
    native update: same parameters as train_step_native with no row mask, within the native tolerance of the torch
    reference path (dropout off), loss returned as a 0-d device tensor, no-valid-row batch = no-op returning 0."""
    qa, qb, qc = _qnet(g, "s40", seed=9), _qnet(g, "s40", seed=9), _qnet(g, "s40", seed=9)
    for q in (qa, qb, qc):
        q.network.eval()
    b = _batch(2000, 21)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    for it in range(2):
        la = qa.train_step(states=dev["states"], actions=dev["actions"], rewards=dev["rewards"], next_states=dev["next_states"], dones=dev["dones"])
        assert isinstance(la, torch.Tensor) and la.is_cuda and la.dim() == 0
        la = float(la)                                              # (the tensor is a view of the report: read it before the next step)
        rep = qb.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], None,
                                   step_counter=(1 << 41) + it + 1)
        lc = qc.train_step_torch(states=dev["states"], actions=dev["actions"], rewards=dev["rewards"], next_states=dev["next_states"], dones=dev["dones"])
        assert la == float(rep[1])
        assert abs(la - float(lc)) < 1e-4 * max(1.0, abs(float(lc)))
    np.testing.assert_array_equal(_flat(qa.network), _flat(qb.network))
    np.testing.assert_allclose(_flat(qa.network), _flat(qc.network), rtol=0, atol=PARAM_ATOL)
    assert qa.step_count == 2 and qa.native_steps() == 2
    before = _flat(qa.network)
    dead = dev["states"].clone(); dead[:, 12] = 1                 # every seat folded: nothing valid (:261-262)
    assert float(qa.train_step(dead, dev["actions"], dev["rewards"], dev["next_states"], dev["dones"])) == 0.0
    np.testing.assert_array_equal(_flat(qa.network), before)


def test_a_called_off_meeting_updates_nothing_and_fails_the_next_call(g):
    """The reduce + AdamW launch is a meeting of its workgroups (qnet.hip).  With the wait cut to 50 ms and one arrival
    more expected than the grid has (the test hook: the meeting cannot come about) the launch returns, no parameter,
    moment or step count has moved, report[3] = -1, the learner's report check raises and the next native call fails
    with PULSE_EINTERNAL -- once; training then goes on (the meeting is all or nothing: a counter that is short is
    marked with a compare-and-swap, so no workgroup can apply its part while another skips its own)."""
    import time
    from pulselib_amd import _native
    q = _qnet(g, "s40", seed=4)
    b = _batch(3000, 5)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    args = (dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"])
    q.train_step_native(*args)                                      # one ordinary step: moments are non-zero from here
    torch.cuda.synchronize()
    p0, m0, v0, s0 = _flat(q.network), q._native["m"].clone(), q._native["v"].clone(), q.native_steps()
    t = q._native_state(3000)
    q.meet_wait_ticks = 5_000_000                                   # 50 ms of the 100 MHz clock
    t.debug_meet_extra = 1
    t.meet_wait_ticks = q.meet_wait_ticks
    called_off = int(_native.lib().pulse_qnet_called_off_meetings())
    t0 = time.perf_counter()
    rep = q.train_step_native(*args).cpu().numpy().copy()
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 5.0                           # it gave up after its 50 ms, not after the default 5 s
    assert int(_native.lib().pulse_qnet_called_off_meetings()) == called_off + 1      # one add per called-off meeting, not one per workgroup
    assert rep[3] == -1.0 and rep[0] == 0.0
    np.testing.assert_array_equal(_flat(q.network), p0)
    assert torch.equal(q._native["m"], m0) and torch.equal(q._native["v"], v0) and q.native_steps() == s0
    with pytest.raises(RuntimeError, match="applied no update"):
        q.check_native_report()
    t.debug_meet_extra = 0
    with pytest.raises(RuntimeError, match="PULSE_EINTERNAL|could not gather"):
        q.train_step_native(*args)
    rep = q.train_step_native(*args).cpu().numpy()                  # reported once; the next step is an ordinary one
    assert rep[3] == 0.0 and rep[0] > 0 and q.native_steps() == s0 + 1
    q.check_native_report()
    assert np.abs(_flat(q.network) - p0).max() > 0
    torch.cuda.synchronize()
    assert int(_native.lib().pulse_qnet_called_off_meetings()) == called_off + 1      # the two ordinary steps added nothing


def test_separate_apply_equals_the_in_launch_adamw(g):
    """`separate_apply` (AdamW as a launch of its own: what a device that cannot hold the reduce grid at once gets, and
    what the data-parallel path always runs) gives the parameters of the in-launch form."""
    qa, qb = _qnet(g, "s40", seed=6), _qnet(g, "s40", seed=6)
    qb.separate_apply = True
    for it in range(3):
        b = _batch(4000, 300 + it)
        dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
        ra = qa.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"], step_counter=it).cpu().numpy().copy()
        rb = qb.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"], step_counter=it).cpu().numpy().copy()
        assert ra[0] == rb[0] and abs(ra[1] - rb[1]) <= 1e-6 * max(1.0, abs(ra[1]))
        np.testing.assert_allclose(_flat(qa.network), _flat(qb.network), rtol=0, atol=PARAM_ATOL)
    assert qa.native_steps() == qb.native_steps() == 3


def test_native_training_reduces_td_error_on_a_fixed_batch(g):
    q = _qnet(g, "s40", seed=1)
    q.lr = 1e-3
    b = _batch(4096, 7)
    b["dones"][:] = True                       # targets = rewards: a plain regression the network can fit
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    losses = []
    for it in range(200):
        rep = q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"])
        if it % 50 == 0 or it == 199:
            losses.append(float(rep[1]))
    assert losses[-1] < 0.7 * losses[0], losses


@pytest.mark.parametrize("net", ["s40", "s64"])
def test_native_train_step_writes_only_inside_its_buffers(g, net):
    """Guard words either side of the gradient, the moments and the slice scratch stay untouched by a training step (the
    slice layout has padding elements that map to no parameter: they must be dropped, not written at index -1)."""
    if net == "s64":
        from pulselib_amd.environments.Poker import PokerQNetwork
        torch.manual_seed(64)
        q = PokerQNetwork(None, torch.device(DEV), gamma=.97, update_freq=3, state_dim=64, action_dim=13, learning_rate=1e-3,
                          weight_decay=0.01, seed=8)
        rng = np.random.default_rng(5)
        n = 3000
        b = dict(states=rng.standard_normal((n, 64)).astype(np.float32), actions=rng.integers(0, 13, n),
                 rewards=rng.standard_normal(n).astype(np.float32), next_states=rng.standard_normal((n, 64)).astype(np.float32),
                 dones=rng.random(n) < 0.1, row_mask=rng.random(n) < 0.8)
        b["states"][:, 12] = rng.integers(0, 4, n)       # seat status column: some rows are not trainable
    else:
        q = _qnet(g, "s40", seed=4)
        b = _batch(3000, 13)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    q._native_state()
    nat, guard, fill = q._native, 256, 12345.0
    held = {}
    for name in ("grad", "m", "v", "partials"):
        n_el = nat[name].numel()
        big = torch.full((n_el + 2 * guard,), fill, dtype=torch.float32, device=DEV)
        big[guard:guard + n_el] = 0.0
        held[name] = big
        nat[name] = big[guard:guard + n_el]
    q._struct_cache.pop("train", None)                   # the cached struct holds the old pointers
    for _ in range(3):
        q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"])
    torch.cuda.synchronize()
    for name, big in held.items():
        n_el = nat[name].numel()
        assert bool((big[:guard] == fill).all()) and bool((big[guard + n_el:] == fill).all()), name
    assert float(nat["grad"].abs().sum()) > 0.0


def test_native_train_step_folds_trainer_bookkeeping(g):
    """terminated |= dones and reward_sum += rewards[row_mask] ride along with the training launches (trainGPU.py:86,96)."""
    q = _qnet(g, "s40", seed=2)
    n = 5000
    b = _batch(n, 11)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    term = torch.from_numpy(np.random.default_rng(3).random(n) < 0.2).to(DEV)
    want_term = (term | dev["dones"]).cpu().numpy()
    acc = torch.full((), 10.0, dtype=torch.float64, device=DEV)
    q.train_step_native(dev["states"], dev["actions"], dev["rewards"], dev["next_states"], dev["dones"], dev["row_mask"],
                        terminated=term, reward_sum=acc)
    np.testing.assert_array_equal(term.cpu().numpy(), want_term)
    want = 10.0 + float(b["rewards"][b["row_mask"]].astype(np.float64).sum())
    assert abs(float(acc) - want) < 1e-3 * max(1.0, abs(want))


def test_trainer_entry_point_writes_run_summary_and_weights(tmp_path):
    """python -m pulselib_amd.scripts.trainGPU: fused loop + run_N.yaml with the reference writer's keys + the final
    weights (scripts/Poker/trainGPU.py:118), which load back into the reference's Sequential layout."""
    import yaml
    from pulselib_amd.environments.Poker.qnetwork import build_network
    from pulselib_amd.scripts.trainGPU import main
    out = main(["--tables", "2048", "--episodes", "2", "--results", str(tmp_path)])
    run = tmp_path / "PokerGPU" / "runs" / "run_1.yaml"
    d = yaml.safe_load(run.read_text())
    assert d["env"] == "Pulse-Poker-GPU-v1" and d["total_steps"] == out["total_steps"] > 0 and d["sps"] > 0
    assert d["episode_stats"]["count"] == 2 and d["config"]["N_GAMES"] == 2048
    sd = torch.load(tmp_path / "PokerGPU" / "poker_qnet_final.pth", weights_only=True)
    build_network(40, 13).load_state_dict(sd)


def test_fused_trainer_with_hand_metrics_side_channel(g):
    from pulselib_amd.environments.Poker import PokerGPU, load_gpu_agents
    from pulselib_amd.environments.Poker.utils import PokerAgentType
    from pulselib_amd.scripts.trainGPU import train_agent_fused
    from pulselib_amd.utils.performance import HandMetrics
    dev = torch.device(DEV)
    agents, types = load_gpu_agents(dev, 5, ["tight_aggressive", "heuristic_hands", "loose_passive", "random", "small_ball"], 100, 13)
    agents.insert(0, _qnet(g, "s40", seed=3))
    types.insert(0, PokerAgentType.QLEARNING)
    N = 2048
    env = PokerGPU(device=dev, agents=agents, n_players=6, max_players=10, n_games=N, seed=11)
    out = train_agent_fused(env, agents, types, episodes=3, n_games=N, device=dev, max_episode_steps=30, reduce_stats=False,
                            hand_metrics=HandMetrics(dev, N))
    hm = out["hand_metrics"]
    assert len(hm["episodes"]) == 3 and hm["final"]["total_hands"] == sum(e["hands_completed"] for e in hm["episodes"]) > 0
    # chips are conserved per table, so what the learner's seat won over the finished hands is what the episodes report
    assert abs(hm["final"]["total_bb_won"]) <= 100 * hm["final"]["total_hands"]
    assert set(hm["final"]["slices"]) == {"opponent_mix", "seat", "player_count", "street_depth"}


@pytest.mark.parametrize("state_dim,n_actions", [(16, 4), (24, 32), (13, 1), (64, 13)])
def test_native_kernels_other_shapes(state_dim, n_actions):
    """The ABI promises state_dim 13..64 and n_actions 1..32 for training (1..4096 / 1..32 for inference): forward,
    masked act and one training step against the oracle at the corners."""
    from oracle import oracle as orc
    from pulselib_amd.environments.Poker import PokerQNetwork
    torch.manual_seed(state_dim * 100 + n_actions)
    q = PokerQNetwork(None, torch.device(DEV), gamma=.9, update_freq=3, state_dim=state_dim, action_dim=n_actions, learning_rate=1e-3,
                      weight_decay=1e-4, seed=8)
    n = 700
    rng = np.random.default_rng(state_dim)
    s = (rng.standard_normal((n, state_dim)) * 2).astype(np.float32); s[:, 12] = rng.integers(0, 4, n)
    ns = (rng.standard_normal((n, state_dim)) * 2).astype(np.float32)
    p0 = _flat(q.network)
    w, b = orc.qnet_split(p0, state_dim, n_actions)
    qv = q.q_values(torch.from_numpy(s).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(qv, orc.qnet_forward(w, b, s), rtol=0, atol=Q_TOL)
    seat = torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)).to(DEV)
    acts = torch.full((n,), -3, dtype=torch.long, device=DEV)
    q.epsilon = q.epsilon_end = 0.0
    q.act_into(torch.from_numpy(s).to(DEV), seat, 1, acts, step_counter=4)
    a = acts.cpu().numpy(); mine = seat.cpu().numpy() == 1
    assert (a[~mine] == -3).all() and ((a[mine] >= 0) & (a[mine] < n_actions)).all()
    top2 = np.sort(qv, axis=1)[:, -2:] if n_actions > 1 else None
    clear = mine if n_actions == 1 else mine & ((top2[:, 1] - top2[:, 0]) > 4 * Q_TOL)
    np.testing.assert_array_equal(a[clear], qv.argmax(axis=1)[clear])
    act = rng.integers(0, n_actions, n).astype(np.int64); rew = rng.standard_normal(n).astype(np.float32); done = rng.random(n) < 0.4
    dev = lambda x: torch.from_numpy(x).to(DEV)
    rep = q.train_step_native(dev(s), dev(act), dev(rew), dev(ns), dev(done), None, step_counter=12).cpu().numpy()
    grad, cnt, sq = orc.qnet_train_grads(p0, p0, s, act, rew, ns, done, None, 0.9, 0.1, 8, 12, 0)
    tp, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    orc.qnet_adamw(p0, tp, grad, m, v, cnt, 1, 1e-3, 1e-4, update_freq=3)
    assert rep[0] == cnt > 0
    np.testing.assert_allclose(_flat(q.network), p0, rtol=0, atol=5e-5)        # 5 % of one learning-rate step (lr = 1e-3)


def test_native_kernels_empty_and_full_selections(g):
    q = _qnet(g, "s40", seed=1)
    q.epsilon = q.epsilon_end = 0.0
    n = 1000
    s = torch.randn((n, 40), device=DEV)
    acts = torch.full((n,), -1, dtype=torch.long, device=DEV)
    q.act_into(s, torch.full((n,), 5, dtype=torch.int32, device=DEV), 2, acts)           # nobody's turn
    assert (acts == -1).all()
    q.act_into(s, torch.full((n,), 2, dtype=torch.int32, device=DEV), 2, acts)           # everybody's turn
    np.testing.assert_array_equal(acts.cpu().numpy(), q.get_actions(s).cpu().numpy())
    before = _flat(q.network)
    rep = q.train_step_native(s[:0], acts[:0], torch.zeros(0, device=DEV), s[:0], torch.zeros(0, dtype=torch.bool, device=DEV))
    assert np.array_equal(_flat(q.network), before)                                      # zero rows: nothing launched, nothing moves


@pytest.mark.parametrize("n", [700, 5000, 70001])
def test_row_lists_from_the_act_launch_equal_the_selection_launch(g, n):
    """act_into(select_for_training=True) writes the training launch's row lists (128-row windows) itself; the lists of the
    selection launch (256-row windows) hold the same rows in the same order, so the two ways train the same tiles and
    leave bit-identical parameters; `terminated |= dones` equal, the episode reward equal up to its summation order."""
    rng = np.random.default_rng(n)
    b = _batch(n, 17)
    b["states"][:, 12] = rng.integers(0, 4, n)                   # seat status: a good part of the rows is not trainable
    seat = torch.from_numpy(rng.integers(0, 6, n).astype(np.int32)).to(DEV)
    term0 = torch.from_numpy(rng.random(n) < 0.15).to(DEV)
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}
    out = []
    for fold in (False, True):
        q = _qnet(g, "s40", seed=9)
        acts = torch.zeros(n, dtype=torch.long, device=DEV)
        mask = torch.zeros(n, dtype=torch.bool, device=DEV)
        term = term0.clone()
        acc = torch.zeros((), dtype=torch.float64, device=DEV)
        for step in range(3):
            q.act_into(dev["states"], seat, 2, acts, step_counter=step, terminated=term, row_mask_out=mask, select_for_training=fold)
            assert (getattr(q, "_act_selected", None) is not None) == fold
            rep = q.train_step_native(dev["states"], acts, dev["rewards"], dev["next_states"], dev["dones"], mask, step_counter=step,
                                      terminated=term, reward_sum=acc)
        out.append((_flat(q.network), rep.cpu().numpy(), term.cpu().numpy(), float(acc), acts.cpu().numpy(), mask.cpu().numpy()))
    (p0, r0, t0, a0, ac0, m0), (p1, r1, t1, a1, ac1, m1) = out
    np.testing.assert_array_equal(ac0, ac1); np.testing.assert_array_equal(m0, m1); np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(p0, p1)
    np.testing.assert_array_equal(r0[:1], r1[:1])
    assert r0[0] > 0 and abs(a0 - a1) <= 1e-4 * max(1.0, abs(a0))
    # a training call on other inputs than the act call's does not pick the lists up
    q.act_into(dev["states"], seat, 2, acts, step_counter=9, terminated=term, row_mask_out=mask, select_for_training=True)
    other = dev["states"].clone()
    q.train_step_native(other, acts, dev["rewards"], dev["next_states"], dev["dones"], mask, step_counter=9)
    assert q._struct_cache["train"].select_from_act == 0


def test_four_and_eight_wavefront_training_kernels_agree(g, tmp_path):
    """PULSE_TRAIN_WAVES=4 keeps the four-wavefront training kernel (comparison runs): the same tiles and dropout draws, layer 4's
    k quarters summed in another order -- parameters after three steps agree to a few ulp of a learning-rate step."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, %r)\n"
        "from tests.test_qnetwork_gpu import _qnet, _batch, _flat, DEV\n"
        "g = np.load(%r)\n"
        "q = _qnet(g, 's40', seed=21); b = _batch(9000, 31)\n"
        "dev = {k: torch.from_numpy(x).to(DEV) for k, x in b.items()}\n"
        "for s in range(3): rep = q.train_step_native(dev['states'], dev['actions'], dev['rewards'], dev['next_states'], dev['dones'], dev['row_mask'], step_counter=s)\n"
        "np.save(sys.argv[1], np.concatenate([_flat(q.network), rep.cpu().numpy()]))\n") % (str(root), str(root / "tests" / "golden" / "qnetwork.npz"))
    out = {}
    for waves in ("4", "8"):
        path = tmp_path / f"p{waves}.npy"
        env = dict(__import__("os").environ, PULSE_TRAIN_WAVES=waves)
        subprocess.run([sys.executable, "-c", code, str(path)], check=True, env=env, cwd=str(root), timeout=300)
        out[waves] = np.load(path)
    assert out["4"][-4] == out["8"][-4] > 0                                  # rows trained on
    np.testing.assert_allclose(out["4"][:-4], out["8"][:-4], rtol=0, atol=2e-7)     # lr = 2e-4: a step moves a weight by <= 2e-4


@pytest.mark.parametrize("N", [4096, 65536])
def test_act_policy_step_equals_act_then_policy_step(g, N, monkeypatch):
    """ONE launch for the first half of the trainer's step (pulse_poker_act_policy_step: the workgroup that picks the
    learner's actions of 128 tables steps those tables itself) against the two launches it replaces (act_into with the row
    lists + policy_step): after every step of three episodes the actions, the trainer's mask, the training launch's row
    lists, the observation / reward / done buffers and the whole table state are identical word for word, and so is the
    stop rule's count taken by the launch (scripts/Poker/trainGPU.py:79-86; Player.py:242-253; PokerGPU.py:527-633).  (The fused
    launch runs the network on 32-row tiles; the stand-alone act launch is held to that form here -- its default, sixteen rows per
    wavefront, sums in another order and may break a near tie of two Q values the other way.)"""
    monkeypatch.setenv("PULSE_ACT_TILES", "1")
    from pulselib_amd.environments.Poker import PokerGPU
    from pulselib_amd.stoprule import LaggedDoneCount
    from tests.helpers import INT_KEYS
    dev = torch.device(DEV)
    kw = dict(n_players=10, max_players=10, n_games=N, starting_bbs=100, max_bbs=1000, w1=.5, w2=.3, K=100, alpha=50, seed=99, table_id0=1000)
    envs = [PokerGPU(device=dev, agents=[], **kw) for _ in range(2)]
    qs = [_qnet(g, "s40", seed=12, table_id0=1000) for _ in range(2)]
    for e, q in zip(envs, qs):
        e.double_buffer_obs = True
        q.epsilon, q.epsilon_end = 0.2, 0.2
    rules = [LaggedDoneCount(dev, N, 0.8, lag=0) for _ in range(2)]
    acts = [torch.zeros(N, dtype=torch.long, device=dev) for _ in range(2)]
    term = [torch.zeros(N, dtype=torch.bool, device=dev) for _ in range(2)]
    mask = [torch.zeros(N, dtype=torch.bool, device=dev) for _ in range(2)]
    gstep, acted = 0, 0
    for ep, (A, q_seat) in enumerate(((10, 3), (6, 0), (3, 2))):
        types = [3, 1, 2, 4, 5, 3, 1, 2, 4, 5]
        types[q_seat] = 0                                              # PULSE_AGENT_EXTERNAL: the learner's seat
        states, infos = [], []
        for e, r, t in zip(envs, rules, term):
            st, info = e.reset(options={"active_players": A, "rotation": ep, "q_agent_seat": q_seat})
            states.append(st); infos.append(info); r.drain(); t.zero_()
        for i in range(12):
            check = i % 5 == 0
            a, b = envs
            out_a = a.act_policy_step(qs[0], q_seat, types, acts[0], gstep, states[0], infos[0]["seat_idx"], term[0], mask[0],
                                      stop_rule=rules[0] if check else None)
            qs[1].act_into(states[1], infos[1]["seat_idx"], q_seat, acts[1], step_counter=gstep, terminated=term[1], row_mask_out=mask[1],
                           select_for_training=True)
            out_b = b.policy_step(types, acts[1], gstep)
            ctx = f"N={N} episode {ep} step {i}"
            assert torch.equal(acts[0], acts[1]), ctx + " actions"
            assert torch.equal(mask[0], mask[1]), ctx + " row mask"
            acted += int(mask[0].sum())
            W = N // 128
            sa, sb = qs[0]._native["select"], qs[1]._native["select"]
            nw256 = (N + 255) // 256
            ca, cb = sa[nw256 * 256: nw256 * 256 + W], sb[nw256 * 256: nw256 * 256 + W]
            assert torch.equal(ca, cb), ctx + " row-list lengths"
            rows_a, rows_b = sa[:N].view(W, 128), sb[:N].view(W, 128)
            keep = torch.arange(128, device=dev)[None, :] < ca[:, None]
            assert torch.equal(rows_a[keep], rows_b[keep]), ctx + " row lists"
            for x, y, name in zip(out_a[:3], out_b[:3], ("obs", "rewards", "dones")):
                assert torch.equal(x, y), f"{ctx} {name}"
            for name in INT_KEYS + ("equities", "prev_stacks", "prev_invested", "equity_dirty"):
                assert torch.equal(getattr(a, name), getattr(b, name)), f"{ctx} {name}"
            assert a._pp == b._pp
            if check:
                rules[1].submit(out_b[2])
                assert rules[0].counts() == rules[1].counts() and rules[0].counts()[2], ctx + " stop-rule count"
            for k in range(2):
                term[k] |= (out_a, out_b)[k][2]
                states[k] = (out_a, out_b)[k][0]
                infos[k] = (out_a, out_b)[k][4]
            gstep += 1
    assert qs[0].epsilon == qs[1].epsilon and qs[0]._calls == qs[1]._calls and acted > N
    # the training launch finds the lists the fused launch wrote (no selection launch of its own): identical updates
    rew = torch.randn(N, device=dev)
    nxt = states[0]
    prev = envs[0]._obs_bufs[1 - envs[0]._pp]
    for k in range(2):
        e, q = envs[k], qs[k]
        st_prev = e._obs_bufs[1 - e._pp]
        if k == 0:
            e.act_policy_step(q, 2, types, acts[k], gstep, states[k], infos[k]["seat_idx"], term[k], mask[k])
        else:
            q.act_into(states[k], infos[k]["seat_idx"], 2, acts[k], step_counter=gstep, terminated=term[k], row_mask_out=mask[k], select_for_training=True)
            e.policy_step(types, acts[k], gstep)
        assert q._act_selected is not None
        q.train_step_native(states[k], acts[k], rew, e.obs, e.is_done, mask[k], step_counter=gstep)
    np.testing.assert_array_equal(_flat(qs[0].network), _flat(qs[1].network))
    for r in rules:
        r.close()


def test_two_launch_action_selection_of_large_batches_equals_the_window_form(g, monkeypatch):
    """The 32-row-tile forms of the masked action selection (what shapes outside the sixteen-rows-per-wavefront kernel's run, and
    PULSE_ACT_TILES=1): from 262,144 rows on (and with the larger scratch) pulse_qnet_act_select first lists the learner's rows per window and
    then runs them in FULL 32-row tiles (qnet_act_rows_kernel) instead of one two-thirds-full tile per window of 128
    candidates: actions, the trainer's mask and the training launch's row lists must be those of the window form (forced
    here by handing the same learner the small scratch), row for row (Player.py:242-253; utils.py:113-119)."""
    monkeypatch.setenv("PULSE_ACT_TILES", "1")
    n = 262144 + 128 * 5 + 77                                   # ragged: a last window that is not full
    dev = torch.device(DEV)
    rng = np.random.default_rng(8)
    states = torch.from_numpy((rng.standard_normal((n, 40)) * 3).round().astype(np.float32)).to(dev)
    states[:, 12] = torch.from_numpy(rng.integers(0, 4, n).astype(np.float32)).to(dev)
    seat = torch.from_numpy(rng.integers(0, 6, n).astype(np.int32)).to(dev)
    seat[1000:1400] = 2                                          # windows full of the learner's rows: four tiles' worth in one window
    seat[5000:5300] = 5                                          # ... and windows without any
    term = torch.from_numpy(rng.random(n) < 0.3).to(dev)
    out = []
    for big in (True, False):
        q = _qnet(g, "s40", seed=31, table_id0=123456)
        q.epsilon, q.epsilon_end = 0.15, 0.15
        q._native_state(n)
        nw = (n + 255) // 256
        if not big:
            q._native["select"] = torch.empty(259 * nw + 512, dtype=torch.int32, device=dev)
            q._struct_cache.pop("train", None)
        else:
            assert q._native["select"].numel() >= 517 * nw + 512
        scratch = q._native["select"]
        scratch.fill_(-7)
        acts = torch.full((n,), -1, dtype=torch.long, device=dev)
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        # (act_into would re-create the scratch at its default size: call the entry point the way it does)
        from pulselib_amd import _native
        net = q._net_struct(q.network)
        _native.check(_native.lib().pulse_qnet_act_select(C.byref(net), states.data_ptr(), states.stride(0), n, seat.data_ptr(), 2, float(q.epsilon),
                                                          q.seed, 4242, q.table_id0, acts.data_ptr(), term.view(torch.uint8).data_ptr(),
                                                          mask.view(torch.uint8).data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                          torch.cuda.current_stream().cuda_stream), "pulse_qnet_act_select")
        torch.cuda.synchronize()
        W = (n + 127) // 128
        counts = scratch[nw * 256: nw * 256 + W].clone()
        rows = scratch[:W * 128].view(W, 128).clone()
        out.append((acts.clone(), mask.clone(), counts, rows))
        if big:                                                   # the act lists exist and hold exactly the learner's rows
            a_counts = scratch[nw * 259 + 512 + nw * 256: nw * 259 + 512 + nw * 256 + W]
            assert int(a_counts.sum()) == int((seat == 2).sum())
    (a1, m1, c1, r1), (a2, m2, c2, r2) = out
    assert torch.equal(a1, a2) and torch.equal(m1, m2) and torch.equal(c1, c2)
    keep = torch.arange(128, device=dev)[None, :] < c1[:, None]
    assert torch.equal(r1[keep], r2[keep])
    mine = seat == 2
    assert bool((a1[~mine] == -1).all()) and bool(((a1[mine] >= 0) & (a1[mine] < 13)).all()) and int(mine.sum()) > n // 8


@pytest.mark.parametrize("n,case", [(70001, "s40"), (300, "s40"), (5000, "s64"), (300001, "s40")])
def test_sixteen_rows_per_wavefront_action_selection_equals_the_tile_form(g, n, case, monkeypatch):
    """pulse_qnet_act_select's default kernel (csrc/qnet_rows16.h: sixteen rows per wavefront, v_mfma_f32_16x16x4 with the
    activations in registers and the network in LDS) against the cooperative 32-row tiles (PULSE_ACT_TILES=1) on the same inputs: the trainer's
    mask and the training launch's row lists are identical, the Q rows agree to the order of the sums, and the actions are
    equal wherever the two best Q values of a row are further apart than that (Player.py:242-253; utils.py:113-119).  Ragged
    sizes, windows full of the learner's rows and windows without any; 300,000 rows take the windows of 1,024 candidates."""
    from pulselib_amd import _native
    dev = torch.device(DEV)
    rng = np.random.default_rng(n)
    sd = 40 if case == "s40" else 64
    states = torch.from_numpy((rng.standard_normal((n, sd)) * 3).round().astype(np.float32)).to(dev)
    states[:, 12] = torch.from_numpy(rng.integers(0, 4, n).astype(np.float32)).to(dev)
    seat = torch.from_numpy(rng.integers(0, 6, n).astype(np.int32)).to(dev)
    if n > 2000:
        seat[1000:1700] = 2
        seat[1700:2300] = 5
    else:
        seat[:] = 2
    term = torch.from_numpy(rng.random(n) < 0.3).to(dev)
    out = []
    for tiles in (False, True):
        monkeypatch.setenv("PULSE_ACT_TILES", "1" if tiles else "0")
        if case == "s64":
            from pulselib_amd.environments.Poker import PokerQNetwork
            torch.manual_seed(64)
            q = PokerQNetwork(None, dev, gamma=.97, update_freq=3, state_dim=64, action_dim=13, learning_rate=1e-3, weight_decay=0.01,
                              seed=31, table_id0=123456)
        else:
            q = _qnet(g, case, seed=31, table_id0=123456)
        q.epsilon, q.epsilon_end = 0.15, 0.15
        q._native_state(n)
        nw = (n + 255) // 256
        scratch = q._native["select"]
        scratch.fill_(-7)
        acts = torch.full((n,), -1, dtype=torch.long, device=dev)
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        net = q._net_struct(q.network)
        _native.check(_native.lib().pulse_qnet_act_select(C.byref(net), states.data_ptr(), states.stride(0), n, seat.data_ptr(), 2, float(q.epsilon),
                                                          q.seed, 4242, q.table_id0, acts.data_ptr(), term.view(torch.uint8).data_ptr(),
                                                          mask.view(torch.uint8).data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                          torch.cuda.current_stream().cuda_stream), "pulse_qnet_act_select")
        qrows = torch.zeros((n, 13), device=dev)
        acts_q = torch.full((n,), -1, dtype=torch.long, device=dev)
        _native.check(_native.lib().pulse_qnet_act(C.byref(net), states.data_ptr(), states.stride(0), n, seat.data_ptr(), 2, float(q.epsilon),
                                                   q.seed, 4242, q.table_id0, acts_q.data_ptr(), qrows.data_ptr(), term.view(torch.uint8).data_ptr(), None,
                                                   torch.cuda.current_stream().cuda_stream), "pulse_qnet_act")
        torch.cuda.synchronize()
        assert torch.equal(acts, acts_q)                                   # the Q output rides along without changing anything
        W = (n + 127) // 128
        out.append((acts.clone(), mask.clone(), scratch[nw * 256: nw * 256 + W].clone(), scratch[:W * 128].view(W, 128).clone(), qrows))
    (a1, m1, c1, r1, q1), (a2, m2, c2, r2, q2) = out
    assert torch.equal(m1, m2) and torch.equal(c1, c2)
    keep = torch.arange(128, device=dev)[None, :] < c1[:, None]
    assert torch.equal(r1[keep], r2[keep])
    mine = seat == 2
    assert int(mine.sum()) > n // 8 and bool((a1[~mine] == -1).all()) and bool((q1[~mine] == 0).all())
    np.testing.assert_allclose(q1.cpu().numpy(), q2.cpu().numpy(), rtol=0, atol=Q_TOL)
    top2 = torch.topk(q2, 2, dim=1).values
    clear = mine & ((top2[:, 0] - top2[:, 1]) > 4 * Q_TOL)
    assert int(clear.sum()) > 0.9 * int(mine.sum())
    assert torch.equal(a1[clear], a2[clear])
    assert bool(((a1[mine] >= 0) & (a1[mine] < 13)).all())
    # the actions follow the kernel's own Q rows exactly (first maximal index, the same epsilon draws)
    from oracle import oracle as orc
    want = np.full(n, -1, dtype=np.int64)
    orc.qnet_act(q1.cpu().numpy(), seat.cpu().numpy(), 2, 0.15, 31, 4242, 123456, want)
    np.testing.assert_array_equal(a1.cpu().numpy(), want)
