"""The fused Blackjack roll-out + first-visit Monte-Carlo learner (csrc/blackjack_mc.hip, agents/first_visit_mc_gpu.py) on the
GPU: its games are the oracle's and the env's own, its histogram reduces to what the CPU class learns from the same episodes,
it only adds, it is reproducible bit for bit, and it writes nothing outside the buffers it is given."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _decks(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(52) for _ in range(n)]).astype(np.int32)


def _replay(decks, trace):
    """The traced actions through the oracle env: every game must end exactly where its trace ends.  Returns the episodes in the
    CPU class's format and every game's terminal reward."""
    n = decks.shape[0]
    env = orc.OracleBlackjack(n)
    obs = env.reset(decks)
    episodes = [[] for _ in range(n)]
    alive = np.ones(n, dtype=bool)
    final = np.zeros(n, dtype=np.int64)
    for t in range(trace.shape[1]):
        a = trace[:, t].astype(np.int64)
        np.testing.assert_array_equal(alive, a >= 0, err_msg=f"action {t}: the oracle's live games are not the traced ones")
        if not alive.any():
            break
        assert set(np.unique(a[alive]).tolist()) <= {0, 1}
        states = obs.copy()
        obs, rew, term = env.step(np.where(alive, a, 1))
        for g in np.nonzero(alive)[0].tolist():
            episodes[g].append((tuple(states[g].tolist()), int(a[g]), int(rew[g])))
        final[alive] = rew[alive]
        alive &= ~term
    assert not alive.any(), "a traced game is not over for the oracle"
    assert set(np.unique(final).tolist()) <= {-1, 1}
    return episodes, final


def _hist_of(episodes):
    from pulselib_amd.agents import first_visit_mc_gpu as mc
    h = np.zeros((mc.N_STATES, mc.MAX_ACTIONS, 2), dtype=np.int64)
    for ep in episodes:
        seen = set()
        for t, (s, _, _) in enumerate(ep):
            if s not in seen:
                seen.add(s)
                h[mc.state_index(*s), len(ep) - 1 - t, int(ep[-1][2] < 0)] += 1
    return h


def _check_against_cpu_class(hist, episodes):
    """counts exactly; sums bit-equal at gamma 0.5 (every partial sum is a multiple of 2^-15 below 2^53), within n_s^2 * 2^-52 at
    gamma 0.9 (the bound on a float64 running sum of n_s terms <= 1, for both sides)."""
    from pulselib_amd.agents import FirstVisitMonteCarlo
    from pulselib_amd.agents.first_visit_mc_gpu import returns_from_histogram
    for gamma in (0.5, 0.9):
        cpu = FirstVisitMonteCarlo(gamma)
        for ep in episodes:
            cpu.learn(ep)
        got = returns_from_histogram(hist, gamma)
        assert set(got) == set(cpu.returns)
        for s, (total, count) in cpu.returns.items():
            assert got[s][1] == count, (gamma, s, got[s], total, count)
            if gamma == 0.5:
                assert got[s][0] == total, (s, got[s][0], total)
            else:
                assert abs(got[s][0] - total) <= count * count * 2.0 ** -52, (s, got[s][0], total)
            assert abs(got[s][0] / got[s][1] - cpu.values[s]) <= (count + 1) * 2.0 ** -52      # the sums' bound over count, + the division's rounding


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1000])
def test_injected_decks_match_the_oracle(B):
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    decks = _decks(B, 100 + B)
    agent = FirstVisitMonteCarloGPU(torch.device(DEV), 0.9, seed=3)
    agent.learn_batch(B, agent.threshold_policy(17), decks=decks, trace=True)
    episodes, final = _replay(decks, agent.last_trace.cpu().numpy())
    hist = agent.histogram()
    np.testing.assert_array_equal(hist, _hist_of(episodes))
    _check_against_cpu_class(hist, episodes)
    assert agent.stats() == {"games": B, "wins": int((final > 0).sum()), "actions": sum(len(e) for e in episodes), "capped": 0}
    assert agent.episode == 1
    v = agent.values
    assert all(isinstance(x, int) for s in v for x in s) and set(v) == set(agent.returns)


def test_device_shuffle_plays_the_envs_own_games():
    """BlackJack(seed=7) stepped as scripts/blackjack_fvmc.run steps it, three episodes, against three fused launches."""
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    from pulselib_amd.environments.blackjack import BlackJack
    B, dev = 1000, torch.device(DEV)
    env = BlackJack(dev, B, seed=7)
    episodes = []
    for _ in range(3):
        obs, _ = env.reset()
        eps = [[] for _ in range(B)]
        alive = torch.ones(B, dtype=torch.bool)
        for _step in range(12):
            states = obs.cpu()
            actions = (obs[:, 0] >= 17).long()
            obs, rewards, terminated, _, _ = env.step(actions)
            a, r, term = actions.cpu(), rewards.cpu(), terminated.cpu()
            for g in torch.nonzero(alive).flatten().tolist():
                eps[g].append((tuple(states[g].tolist()), int(a[g]), int(r[g])))
            alive &= ~term
            if not alive.any():
                break
        assert not alive.any()
        episodes += eps
    agent = FirstVisitMonteCarloGPU(dev, 0.9, seed=7)
    for _ in range(3):
        agent.learn_batch(B, agent.threshold_policy(17))
    hist = agent.histogram()
    np.testing.assert_array_equal(hist, _hist_of(episodes))
    _check_against_cpu_class(hist, episodes)
    st = agent.stats()
    assert st["games"] == 3 * B and st["actions"] == sum(len(e) for e in episodes) and st["capped"] == 0
    assert st["wins"] == sum(e[-1][2] > 0 for e in episodes)


def test_stochastic_policy_replays_through_the_oracle():
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    B = 4096
    decks = _decks(B, 5)
    agent = FirstVisitMonteCarloGPU(torch.device(DEV), 0.9, seed=21)
    agent.learn_batch(B, agent.uniform_policy(), decks=decks, trace=True)
    trace = agent.last_trace.cpu().numpy()
    episodes, final = _replay(decks, trace)
    np.testing.assert_array_equal(agent.histogram(), _hist_of(episodes))
    assert agent.stats() == {"games": B, "wins": int((final > 0).sum()), "actions": sum(len(e) for e in episodes), "capped": 0}
    share = float((trace[:, 0] == 0).mean())
    assert abs(share - 0.5) <= 6.0 * np.sqrt(0.25 / B), share      # binomial, 6 sigma: false failure ~2e-9
    # another episode draws other actions from the same decks (the stream is keyed by the episode)
    agent.learn_batch(B, agent.uniform_policy(), decks=decks, trace=True)
    assert not np.array_equal(agent.last_trace.cpu().numpy(), trace)


def test_accumulation_batching_and_reproducibility():
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    dev, B = torch.device(DEV), 1000
    one = FirstVisitMonteCarloGPU(dev, 0.9, seed=5)
    pol = one.threshold_policy(17)
    one.learn_batch(B, pol, n_episodes=3)
    assert one.episode == 3
    three = FirstVisitMonteCarloGPU(dev, 0.9, seed=5)
    snaps = []
    for i in range(3):
        three.learn_batch(B, pol, max_blocks=1 if i == 1 else 0)     # (one persistent workgroup looping over all games: same counts)
        snaps.append((three.histogram().copy(), three.counters.cpu().numpy().copy()))
    np.testing.assert_array_equal(one.histogram(), three.histogram())
    np.testing.assert_array_equal(one.counters.cpu().numpy(), three.counters.cpu().numpy())
    assert three.stats()["games"] == 3 * B
    # the second launch added to the first: it is the first episode's histogram plus the second episode's own
    second = FirstVisitMonteCarloGPU(dev, 0.9, seed=5)
    second.episode = 1
    second.learn_batch(B, pol)
    np.testing.assert_array_equal(snaps[1][0], snaps[0][0] + second.histogram())
    np.testing.assert_array_equal(snaps[1][1], snaps[0][1] + second.counters.cpu().numpy())
    assert (snaps[1][0] >= snaps[0][0]).all() and snaps[1][0].sum() > snaps[0][0].sum() > 0
    # same seed, same accumulator, bit for bit (a stochastic policy too)
    runs = []
    for _ in range(2):
        a = FirstVisitMonteCarloGPU(dev, 0.9, seed=9)
        a.learn_batch(5000, a.uniform_policy(), n_episodes=2)
        runs.append((a.histogram(), a.counters.cpu().numpy()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    other = FirstVisitMonteCarloGPU(dev, 0.9, seed=10)
    other.learn_batch(5000, other.uniform_policy(), n_episodes=2)
    assert not np.array_equal(other.histogram(), runs[0][0])
    one.clear()
    assert int(one.acc.abs().sum()) == 0 and int(one.counters.abs().sum()) == 0 and one.returns == {} and one.values == {}


def test_launch_writes_only_inside_its_buffers():
    from pulselib_amd import _native
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    from pulselib_amd.agents.first_visit_mc_gpu import ACC_LEN, MAX_ACTIONS
    dev, B, guard, poison = torch.device(DEV), 257, 64, 0x5A5A5A5A5A5A5A5A
    lib = _native.lib()
    pol = torch.from_numpy(FirstVisitMonteCarloGPU.uniform_policy().table).to(dev)
    acc = torch.full((ACC_LEN + 2 * guard,), poison, dtype=torch.int64, device=dev)
    stats = torch.full((4 + 2 * guard,), poison, dtype=torch.int64, device=dev)
    trace = torch.full((B * MAX_ACTIONS + 2 * guard,), 0x5A, dtype=torch.int8, device=dev)
    acc[guard:guard + ACC_LEN] = 0
    stats[guard:guard + 4] = 0
    spare = trace.clone()                                          # a trace-sized buffer that is passed nowhere
    for with_trace in (True, False):
        o = _native.BlackjackMC()
        o.n_games, o.n_episodes, o.seed, o.episode = B, 1, 4, 0
        o.hit_prob, o.acc, o.stats = pol.data_ptr(), acc.data_ptr() + 8 * guard, stats.data_ptr() + 8 * guard
        if with_trace:
            o.trace = trace.data_ptr() + guard
        _native.check(lib.pulse_blackjack_mc_rollout(C.byref(o), _native.current_stream(dev)), "pulse_blackjack_mc_rollout")
        torch.cuda.synchronize()
        for name, buf, n in (("acc", acc, ACC_LEN), ("stats", stats, 4)):
            assert (buf[:guard] == poison).all() and (buf[guard + n:] == poison).all(), f"{name}: a guard word was written"
        assert (trace[:guard] == 0x5A).all() and (trace[guard + B * MAX_ACTIONS:] == 0x5A).all(), "trace: a guard byte was written"
        assert (spare == 0x5A).all()
        rows = trace[guard:guard + B * MAX_ACTIONS].view(B, MAX_ACTIONS).cpu().numpy()
        assert ((rows >= -1) & (rows <= 1)).all() and (rows[:, 0] >= 0).all()
        assert stats[guard:guard + 4].tolist() == [B * (1 if with_trace else 2), stats[guard + 1].item(), int(acc[guard:guard + ACC_LEN].sum()), 0]


def test_cap_bounds_a_game_on_a_degenerate_deck():
    """52 aces of one suit, always hit: the rules end such a game by themselves (ten hits, then bust); the launch ends, counts 64
    games and the oracle's replay gives its histogram."""
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    from pulselib_amd.agents.first_visit_mc_gpu import MAX_ACTIONS, N_STATES
    B, dev = 64, torch.device(DEV)
    decks = np.zeros((B, 52), dtype=np.int32)
    agent = FirstVisitMonteCarloGPU(dev, 0.9)
    agent.learn_batch(B, torch.ones(N_STATES, dtype=torch.float32, device=dev), decks=decks, trace=True)
    trace = agent.last_trace.cpu().numpy()
    st = agent.stats()
    assert st["games"] == B and st["capped"] == 0
    episodes, final = _replay(decks, trace)
    assert all(len(e) <= MAX_ACTIONS for e in episodes) and (final == -1).all()
    np.testing.assert_array_equal(agent.histogram(), _hist_of(episodes))
    assert st["actions"] == sum(len(e) for e in episodes) and st["wins"] == 0


def test_sanity_at_a_million_games():
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    B = 1 << 20
    agent = FirstVisitMonteCarloGPU(torch.device(DEV), 0.9, seed=7)
    agent.learn_batch(B, agent.threshold_policy(17))
    returns, values, st = agent.returns, agent.values, agent.stats()
    assert st["games"] == B and st["capped"] == 0 and 0.35 * B < st["wins"] < 0.65 * B      # the env counts a push as a win: about half
    assert sum(c for _, c in returns.values()) == st["actions"]     # no state repeats within a game: every action is a first visit
    assert len(values) > 250 and all(-1.0 <= v <= 1.0 for v in values.values())
    assert all(4 <= s <= 21 and ace in (0, 1) and 2 <= up <= 11 for (s, ace, up) in values)
    strong = [v for (s, ace, up), v in values.items() if s in (20, 21)]
    weak = [v for (s, ace, up), v in values.items() if s in (14, 15, 16) and not ace]
    assert sum(strong) / len(strong) > 0.5 > sum(weak) / len(weak)
