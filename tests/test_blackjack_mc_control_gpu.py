"""On-policy first-visit Monte-Carlo control for Blackjack on the GPU (csrc/blackjack_mc.hip: pulse_blackjack_mc_control_rollout,
pulse_blackjack_mc_improve; agents/on_policy_first_visit_mc_gpu.py): the roll-out's action histogram is the host's count of pair
first visits of the oracle's replay and sums to the value learner's histogram, the improvement kernel is its host statement bit
for bit, the device loop is the host-driven loop, nothing is written outside the buffers, and the loop learns to play."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.test_blackjack_mc_control_cpu import action_histogram, handmade_histogram
from tests.test_blackjack_mc_gpu import _decks, _replay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _coins(seed, rnd):
    """The improvement kernel's tie coins of one round, from the oracle's Philox: bit 0 of word 0 of (seed ^ key, state, round)."""
    from pulselib_amd import _native
    return np.array([int(orc.philox4x32(seed ^ _native.BJ_MCC_TIE_KEY, s, rnd)[0]) & 1 for s in range(_native.BJ_MC_STATES)], dtype=bool)


def _check_against_cpu_class(agent, hist, episodes):
    """returns: counts exactly, sums bit-equal at gamma 0.5 and within n^2 * 2^-52 at gamma 0.9; q (the agent's gamma, 0.9): the
    same key set -- both actions of every state visited -- and within (n + 1) * 2^-52 (the sums' bound over n, + the division's
    rounding): the bounds of tests/test_blackjack_mc_gpu.py."""
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import returns_from_action_histogram
    for gamma in (0.5, 0.9):
        cpu = OnPolicyFirstVisitMC(gamma, 0.1)
        for ep in episodes:
            cpu.learn(ep)
        got = returns_from_action_histogram(hist, gamma)
        assert set(got) == set(cpu.returns)
        for pair, (total, count) in cpu.returns.items():
            assert got[pair][1] == count, (gamma, pair, got[pair], total, count)
            if gamma == 0.5:
                assert got[pair][0] == total, (pair, got[pair][0], total)
            else:
                assert abs(got[pair][0] - total) <= count * count * 2.0 ** -52, (pair, got[pair][0], total)
    assert agent.gamma == 0.9 and agent.returns == got
    q = agent.q
    assert set(q) == set(cpu.q)
    for pair, value in cpu.q.items():
        count = cpu.returns[pair][1] if pair in cpu.returns else 0.0
        assert abs(q[pair] - value) <= (count + 1) * 2.0 ** -52 and (count or q[pair] == 0.0), (pair, q[pair], value)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 513, 1000])
def test_injected_decks_match_the_oracle(B):
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    decks = _decks(B, 200 + B)
    agent = OnPolicyFirstVisitMCGPU(torch.device(DEV), 0.9, 0.1, seed=3)
    agent.learn_batch(B, decks=decks, trace=True, max_blocks=1 if B == 1000 else 0)      # (1000 games in one workgroup: lanes loop)
    episodes, final = _replay(decks, agent.last_trace.cpu().numpy())
    hist = agent.histogram()
    np.testing.assert_array_equal(hist, action_histogram(episodes))
    _check_against_cpu_class(agent, hist, episodes)
    assert agent.stats() == {"games": B, "wins": int((final > 0).sum()), "actions": sum(len(e) for e in episodes), "capped": 0}
    assert agent.episode == 1 and agent.round == 0
    if B >= 63:                                                            # the uniform default: both actions are taken
        assert {a for e in episodes for _, a, _ in e} == {0, 1}
    assert set(agent.policy) == {s for e in episodes for s, _, _ in e} and all(p == [0.5, 0.5] for p in agent.policy.values())


def test_actions_sum_to_the_value_learners_histogram():
    """Same seed, same table, the device shuffle: cards 0..51 repeat no state within a game, so pair first visits are state
    first visits and the control histogram summed over the actions is pulse_blackjack_mc_rollout's, cell for cell."""
    from pulselib_amd.agents import FirstVisitMonteCarloGPU, OnPolicyFirstVisitMCGPU
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import MAX_ACTIONS, N_STATES
    dev, B = torch.device(DEV), 1000
    value = FirstVisitMonteCarloGPU(dev, 0.9, seed=11)
    control = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1, seed=11)
    value.learn_batch(B, value.uniform_policy(), n_episodes=3)
    control.learn_batch(B, n_episodes=3, policy=control.uniform_policy())
    h = control.histogram()
    summed = h[:, :MAX_ACTIONS * 2].reshape(N_STATES, MAX_ACTIONS, 2).copy()
    summed[:, 0, :] += h[:, MAX_ACTIONS * 2:]
    np.testing.assert_array_equal(summed, value.histogram())
    assert h[:, MAX_ACTIONS * 2:].sum() > 0 and h[:, :MAX_ACTIONS * 2].sum() > 0
    assert control.stats() == value.stats() and control.stats()["games"] == 3 * B and control.episode == 3


def test_degenerate_deck_of_aces():
    """52 aces of one suit, always hit: the rules end such a game by themselves (tests/test_blackjack_mc_gpu.py)."""
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import MAX_ACTIONS, N_STATES
    B, dev = 64, torch.device(DEV)
    decks = np.zeros((B, 52), dtype=np.int32)
    agent = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1)
    agent.learn_batch(B, decks=decks, trace=True, policy=torch.ones(N_STATES, dtype=torch.float32, device=dev))
    st = agent.stats()
    assert st["games"] == B and st["capped"] == 0
    episodes, final = _replay(decks, agent.last_trace.cpu().numpy())
    assert all(len(e) <= MAX_ACTIONS for e in episodes) and (final == -1).all()
    np.testing.assert_array_equal(agent.histogram(), action_histogram(episodes))
    assert st["actions"] == sum(len(e) for e in episodes) and st["wins"] == 0


@pytest.mark.parametrize("hit_below", [32, 15])
def test_a_pair_that_repeats_within_a_game_counts_once(hit_below):
    """A card of rank 0 (-1: any int32 is a card, as the env takes them) leaves the player's sum where it was: 5, 5, 5, then 15.
    Always hitting busts at 25; standing on 15 wins against a dealer who busts.  (5, hit) is counted at its first visit only."""
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    B, dev = 65, torch.device(DEV)
    decks = np.full((B, 52), 9, dtype=np.int32)
    decks[:, :6] = [1, 5, 2, 6, -1, -1]
    agent = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1)
    agent.learn_batch(B, decks=decks, trace=True, policy=agent.threshold_policy(hit_below))
    episodes, final = _replay(decks, agent.last_trace.cpu().numpy())
    stand = hit_below == 15
    assert all([s for s, _, _ in e] == [(5, 0, 6)] * 3 + [(15, 0, 6)] and [a for _, a, _ in e] == [0, 0, 0, int(stand)] for e in episodes)
    expect = np.zeros((mc.N_STATES, mc.CELLS), dtype=np.int64)
    expect.reshape(-1)[mc.cell_hit(mc.state_index(5, 0, 6), 3, not stand)] = B
    expect.reshape(-1)[mc.cell_stand(mc.state_index(15, 0, 6), 0) if stand else mc.cell_hit(mc.state_index(15, 0, 6), 0, 1)] = B
    np.testing.assert_array_equal(action_histogram(episodes), expect)
    np.testing.assert_array_equal(agent.histogram(), expect)
    assert agent.stats() == {"games": B, "wins": B if stand else 0, "actions": 4 * B, "capped": 0} and (final == (1 if stand else -1)).all()


def _improve(acc, hit_prob, gamma, epsilon, seed, rnd, with_q=True):
    from pulselib_amd import _native
    q = torch.full((_native.BJ_MC_STATES, 2), 7.0, dtype=torch.float64, device=acc.device)
    o = _native.BlackjackMCImprove()
    o.acc, o.gamma, o.epsilon, o.seed, o.round, o.hit_prob = acc.data_ptr(), gamma, epsilon, seed, rnd, hit_prob.data_ptr()
    if with_q:
        o.q = q.data_ptr()
    _native.check(_native.lib().pulse_blackjack_mc_improve(C.byref(o), _native.current_stream(acc.device)), "pulse_blackjack_mc_improve")
    return q.cpu().numpy()


def test_improve_kernel_is_its_host_statement():
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    dev = torch.device(DEV)
    h, at = handmade_histogram()
    rng = np.random.default_rng(8)
    busy = h.copy()                                                        # plus states with long sums that round at gamma 0.9
    for s in rng.choice(mc.N_STATES, 200, replace=False).tolist():
        if not h[s].any():
            busy[s] = rng.integers(0, 1000, mc.CELLS) * (rng.random(mc.CELLS) < 0.6)
    before = np.linspace(0.2, 0.8, mc.N_STATES).astype(np.float32)
    for hist, gamma, epsilon, seed, rnd in ((h, 0.5, 0.1, 5, 0), (h, 0.5, 0.0, 5, 1), (h, 0.5, 1.0, 6, 0), (busy, 0.9, 0.1, 2 ** 63 + 9, 2 ** 40)):
        acc = torch.from_numpy(hist.reshape(-1)).to(dev)
        hit_prob = torch.from_numpy(before).to(dev)
        q = _improve(acc, hit_prob, gamma, epsilon, seed, rnd)
        want_q, want_p = mc.improve_on_host(hist, gamma, epsilon, before, _coins(seed, rnd))
        assert q.tobytes() == want_q.tobytes(), (gamma, epsilon, np.nonzero(q != want_q))
        got_p = hit_prob.cpu().numpy()
        assert got_p.tobytes() == want_p.tobytes(), (gamma, epsilon, np.nonzero(got_p != want_p))
        assert got_p[at["unvisited"]] == before[at["unvisited"]] and np.array_equal(acc.cpu().numpy(), hist.reshape(-1))
        if epsilon == 0.1 and hist is h:                                   # the ties followed their coins, whatever those were
            coins = _coins(seed, rnd)
            for name in ("tie_a", "tie_b", "tie_unseen"):
                assert got_p[at[name]] == np.float32(0.05 if coins[at[name]] else 0.95)


def test_improve_kernel_tie_coins():
    """All 1,024 states tied (one stand won, one lost: q_stand = 0 = the unseen hit's)."""
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    dev = torch.device(DEV)
    h = np.zeros((mc.N_STATES, mc.CELLS), dtype=np.int64)
    h[:, mc.MAX_ACTIONS * 2:] = 1
    acc = torch.from_numpy(h.reshape(-1)).to(dev)
    tables = {}
    for seed, rnd in ((5, 0), (5, 0), (5, 1), (6, 0)):
        hit_prob = torch.full((mc.N_STATES,), 0.5, dtype=torch.float32, device=dev)
        _improve(acc, hit_prob, 0.9, 0.1, seed, rnd, with_q=False)
        p = hit_prob.cpu().numpy()
        assert set(np.unique(p).tolist()) == {float(np.float32(0.05)), float(np.float32(0.95))}
        stands = p == np.float32(0.05)
        np.testing.assert_array_equal(stands, _coins(seed, rnd))
        assert abs(float(stands.mean()) - 0.5) <= 6.0 * np.sqrt(0.25 / mc.N_STATES), stands.mean()      # binomial, 6 sigma: false failure ~2e-9
        if (seed, rnd) in tables:
            np.testing.assert_array_equal(tables[seed, rnd], p)            # the same (seed, round): the same coins
        tables[seed, rnd] = p
    assert not np.array_equal(tables[5, 0], tables[5, 1]) and not np.array_equal(tables[5, 0], tables[6, 0])


def test_device_loop_is_the_host_driven_loop():
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    dev, B, seed = torch.device(DEV), 1000, 17
    device, host, whole = (OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1, seed=seed) for _ in range(3))
    whole.train(5, B)
    for batch in range(5):
        device.train(1, B)
        host.learn_batch(B)
        q, table = mc.improve_on_host(host.histogram(), 0.9, 0.1, host.hit_prob.cpu().numpy(), _coins(seed, batch))
        host.hit_prob.copy_(torch.from_numpy(table))
        np.testing.assert_array_equal(device.histogram(), host.histogram(), err_msg=f"batch {batch}")
        assert device.hit_prob.cpu().numpy().tobytes() == table.tobytes(), batch
        assert device.q_table.cpu().numpy().tobytes() == q.tobytes(), batch
    assert device.round == whole.round == 5 and device.episode == whole.episode == 5
    np.testing.assert_array_equal(whole.histogram(), device.histogram())
    assert torch.equal(whole.hit_prob, device.hit_prob) and torch.equal(whole.q_table, device.q_table) and whole.stats() == device.stats()
    table = device.hit_prob.cpu().numpy()
    assert set(np.unique(table).tolist()) == {float(np.float32(0.05)), 0.5, float(np.float32(0.95))}   # 0.5: never visited
    assert device.greedy_policy().keys() == device.policy.keys() and len(device.policy) > 150


def test_reproducibility_and_clear():
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    dev = torch.device(DEV)
    runs = []
    for seed in (9, 9, 10):
        a = OnPolicyFirstVisitMCGPU(dev, 0.9, 0.1, seed=seed)
        a.train(3, 5000, n_episodes=2)
        runs.append((a.histogram(), a.hit_prob.cpu().numpy(), a.q_table.cpu().numpy(), a.stats()))
    assert runs[0][3]["games"] == 30000 and runs[0][3] == runs[1][3]
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(runs[0][0], runs[2][0])
    a.clear()
    assert int(a.acc.abs().sum()) == 0 and int(a.counters.abs().sum()) == 0 and a.round == 0 and (a.hit_prob == 0.5).all()
    assert a.returns == {} and a.q == {} and a.policy == {}


def test_launches_write_only_inside_their_buffers():
    from pulselib_amd import _native
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import ACC_LEN, MAX_ACTIONS, N_STATES
    dev, B, guard, poison = torch.device(DEV), 257, 64, 0x5A5A5A5A5A5A5A5A
    lib = _native.lib()
    acc = torch.full((ACC_LEN + 2 * guard,), poison, dtype=torch.int64, device=dev)
    stats = torch.full((4 + 2 * guard,), poison, dtype=torch.int64, device=dev)
    trace = torch.full((B * MAX_ACTIONS + 2 * guard,), 0x5A, dtype=torch.int8, device=dev)
    q = torch.full((2 * N_STATES + 2 * guard,), poison, dtype=torch.int64, device=dev)          # (float64 cells, compared as bits)
    pol = torch.full((N_STATES + 2 * guard,), 0.5, dtype=torch.float32, device=dev)
    pol[:guard], pol[guard + N_STATES:] = -3.0, -3.0
    acc[guard:guard + ACC_LEN] = 0
    stats[guard:guard + 4] = 0
    spare_trace, spare_q = trace.clone(), q.clone()                        # buffers of the same sizes that are passed nowhere
    for with_extras in (True, False):
        o = _native.BlackjackMCControl()
        o.n_games, o.n_episodes, o.seed, o.episode = B, 1, 4, 0
        o.hit_prob, o.acc, o.stats = pol.data_ptr() + 4 * guard, acc.data_ptr() + 8 * guard, stats.data_ptr() + 8 * guard
        if with_extras:
            o.trace = trace.data_ptr() + guard
        _native.check(lib.pulse_blackjack_mc_control_rollout(C.byref(o), _native.current_stream(dev)), "pulse_blackjack_mc_control_rollout")
        i = _native.BlackjackMCImprove()
        i.acc, i.gamma, i.epsilon, i.seed, i.round, i.hit_prob = o.acc, 0.9, 0.1, 4, 0, o.hit_prob
        if with_extras:
            i.q = q.data_ptr() + 8 * guard
        _native.check(lib.pulse_blackjack_mc_improve(C.byref(i), _native.current_stream(dev)), "pulse_blackjack_mc_improve")
        torch.cuda.synchronize()
        for name, buf, n in (("acc", acc, ACC_LEN), ("stats", stats, 4), ("q", q, 2 * N_STATES)):
            assert (buf[:guard] == poison).all() and (buf[guard + n:] == poison).all(), f"{name}: a guard word was written"
        assert (trace[:guard] == 0x5A).all() and (trace[guard + B * MAX_ACTIONS:] == 0x5A).all(), "trace: a guard byte was written"
        assert (pol[:guard] == -3.0).all() and (pol[guard + N_STATES:] == -3.0).all(), "hit_prob: a guard word was written"
        assert (spare_trace == 0x5A).all() and (spare_q == poison).all()
        rows = trace[guard:guard + B * MAX_ACTIONS].view(B, MAX_ACTIONS).cpu().numpy()
        assert ((rows >= -1) & (rows <= 1)).all() and (rows[:, 0] >= 0).all()
        assert stats[guard:guard + 4].tolist() == [B * (1 if with_extras else 2), stats[guard + 1].item(), int(acc[guard:guard + ACC_LEN].sum()), 0]
        assert (q[guard:guard + 2 * N_STATES] != poison).all()
        inner = pol[guard:guard + N_STATES].cpu().numpy()
        assert set(np.unique(inner).tolist()) <= {float(np.float32(0.05)), 0.5, float(np.float32(0.95))} and (inner != 0.5).any()


def test_it_learns_to_play():
    """train(64, 65536) at gamma 0.9, epsilon 0.1: the greedy policy stands on hard 20 and 21 and hits on hard 9, 10 and 11 against
    every upcard.

    The same batch loop on the CPU (OracleBlackjack under numpy's shuffles and draws + improve_on_host, 64 x 65,536 games) left
    every one of these 50 states decided: the smallest |Q(hit) - Q(stand)| was 0.328 (hard 9 against a 4: +0.187 against -0.140),
    the closest in standard errors hard 9 against a 6, 0.361 at 9.3 standard errors (0.0389; 11,542 hits, 678 stands), then hard
    9 against a 4 at 10.8; hard 20 stood at 120 standard errors or more and hard 21 holds no noise at all (a hit always busts, a
    stand never loses: -1 against +1).  None is within 6 standard errors of zero, so all 50 are asserted."""
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import HIT, STAND
    agent = OnPolicyFirstVisitMCGPU(torch.device(DEV), 0.9, 0.1, seed=1)
    agent.train(64, 65536)
    greedy, st = agent.greedy_policy(), agent.stats()
    assert st["games"] == 64 * 65536 and st["capped"] == 0
    wrong = [(s, up) for s, want in ((20, STAND), (21, STAND), (9, HIT), (10, HIT), (11, HIT)) for up in range(2, 12)
             if greedy.get((s, 0, up)) != want]
    assert not wrong, wrong
