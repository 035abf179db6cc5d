"""The host half of the on-device first-visit Monte-Carlo learner for Blackjack (pulselib_amd/agents/first_visit_mc_gpu.py,
csrc/blackjack_mc.hip): the histogram -> (sum of returns, count) reduction against the CPU class, the entry point's argument
checks, and the public state index.  Nothing here launches a kernel."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _episodes(n, seed):
    """Blackjack-shaped episodes in the CPU class's format: 1-6 distinct states, rewards 0 then +-1."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = int(rng.integers(1, 7))
        states = set()
        while len(states) < T:                               # few sums / upcards: states recur ACROSS episodes (n_s up to ~40)
            states.add((int(rng.integers(12, 18)), int(rng.integers(0, 2)), int(rng.integers(2, 6))))
        states = sorted(states)
        rng.shuffle(states)
        r = 1 if rng.random() < 0.45 else -1
        out.append([(tuple(s), int(rng.integers(0, 2)), r if t == T - 1 else 0) for t, s in enumerate(states)])
    return out


def _histogram(episodes):
    from pulselib_amd.agents import first_visit_mc_gpu as mc
    h = np.zeros((mc.N_STATES, mc.MAX_ACTIONS, 2), dtype=np.int64)
    for ep in episodes:
        r = ep[-1][2]
        for t, (s, _, _) in enumerate(ep):
            h[mc.state_index(*s), len(ep) - 1 - t, int(r < 0)] += 1
    return h


@pytest.mark.parametrize("gamma", [1.0, 0.5, 0.9])
def test_histogram_reduction_matches_the_cpu_class(gamma):
    """counts are equal exactly; sums are BIT-equal for gamma 1.0 / 0.5 (every partial sum is a multiple of 2^-15 below 2^53, so
    both summation orders are exact) and within n_s^2 * 2^-52 per state for gamma 0.9: the bound on a float64 running sum of n_s
    terms of magnitude <= 1 (n_s * n_s * 2^-53), once for each side."""
    from pulselib_amd.agents import FirstVisitMonteCarlo
    from pulselib_amd.agents.first_visit_mc_gpu import returns_from_histogram
    episodes = _episodes(400, 11)
    cpu = FirstVisitMonteCarlo(gamma)
    for ep in episodes:
        cpu.learn(ep)
    got = returns_from_histogram(_histogram(episodes), gamma)
    assert set(got) == set(cpu.returns) and len(got) > 40
    assert max(c for _, c in cpu.returns.values()) > 20            # the running sums are long enough to round at gamma 0.9
    for s, (total, count) in cpu.returns.items():
        assert got[s][1] == count, s
        assert all(isinstance(x, int) for x in s)
        if gamma in (1.0, 0.5):
            assert got[s][0] == total, (s, got[s][0], total)
        else:
            assert abs(got[s][0] - total) <= count * count * 2.0 ** -52, (s, got[s][0], total)


def test_histogram_reduction_is_a_pure_numpy_function_of_any_int_layout():
    from pulselib_amd.agents import first_visit_mc_gpu as mc
    h = np.zeros(mc.ACC_LEN, dtype=np.int64)                       # the device accumulator's flat form
    s = mc.state_index(20, 0, 10)
    h[(s * 16 + 0) * 2 + 0] = 3                                    # three wins standing on 20
    h[(s * 16 + 2) * 2 + 1] = 1                                    # one loss two steps later
    assert mc.returns_from_histogram(h, 0.5) == {(20, 0, 10): [3.0 - 0.25, 4.0]}
    assert mc.returns_from_histogram(np.zeros(mc.ACC_LEN, dtype=np.int64), 0.9) == {}


def test_rollout_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    fn = lib.pulse_blackjack_mc_rollout

    def opts(**kw):
        o = _native.BlackjackMC()                                  # (zero-initialised)
        o.n_games, o.n_episodes = 64, 1
        o.hit_prob, o.acc, o.stats = 0x10000, 0x20000, 0x30000    # never dereferenced: every case below fails its check first
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert fn(None, None) == -1 and b"options are null" in lib.pulse_last_error()
    for kw, msg in [(dict(acc=None), b"acc is null"), (dict(hit_prob=None), b"hit_prob is null"), (dict(stats=None), b"stats is null"),
                    (dict(n_games=0), b"n_games must be positive"), (dict(n_games=-5), b"n_games must be positive"),
                    (dict(n_episodes=0), b"n_episodes must be positive"), (dict(n_episodes=-1), b"n_episodes must be positive"),
                    (dict(n_games=1 << 20, n_episodes=1 << 12), b"below 2^32"),
                    (dict(acc=0x20004), b"8-byte aligned"), (dict(stats=0x30004), b"8-byte aligned"),
                    (dict(hit_prob=0x10002), b"4-byte aligned"), (dict(decks_src=0x40001), b"4-byte aligned"),
                    (dict(trace=0x50008), b"16-byte aligned"), (dict(max_blocks=-1), b"max_blocks"),
                    (dict(reserved0=1), b"reserved0 must be 0")]:
        o = opts(**kw)
        assert fn(C.byref(o), None) == -1, kw
        err = lib.pulse_last_error()
        assert err.startswith(b"pulse_blackjack_mc_rollout: ") and msg in err, (kw, err)
    with pytest.raises(ValueError, match="acc is null"):
        _native.check(fn(C.byref(opts(acc=None)), None), "pulse_blackjack_mc_rollout")


def test_gpu_class_refuses_cpu_devices():
    import torch
    from pulselib_amd.agents import FirstVisitMonteCarloGPU
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        FirstVisitMonteCarloGPU(torch.device("cpu"), 0.9)


def test_state_index_of_the_header_round_trips():
    """The macro of include/pulse_env.h, evaluated as written, is the Python state_index; every reachable state gets its own index
    inside the layout and comes back from it."""
    from pulselib_amd import _native
    from pulselib_amd.agents import first_visit_mc_gpu as mc
    text = (ROOT / "include" / "pulse_env.h").read_text()
    body = re.search(r"#define PULSE_BJ_MC_STATE_INDEX\(sum, has_ace, upcard\)\s+(\(.*?\))\s*/\*", text).group(1)
    consts = {n: int(v) for n, v in re.findall(r"#define (PULSE_BJ_MC_(?:MAX_ACTIONS|STATES))\s+(\d+)", text)}
    assert consts == {"PULSE_BJ_MC_MAX_ACTIONS": _native.BJ_MC_MAX_ACTIONS, "PULSE_BJ_MC_STATES": _native.BJ_MC_STATES}
    assert _native.BJ_MC_ACC_LEN == consts["PULSE_BJ_MC_STATES"] * consts["PULSE_BJ_MC_MAX_ACTIONS"] * 2
    seen = set()
    for s in range(4, 22):
        for ace in (0, 1):
            for up in range(2, 12):
                i = eval(body, {"__builtins__": {}}, {"sum": s, "has_ace": ace, "upcard": up})
                assert i == mc.state_index(s, ace, up) and 0 <= i < mc.N_STATES
                assert mc.state_from_index(i) == (s, ace, up)
                seen.add(i)
    assert len(seen) == 18 * 2 * 10
    with pytest.raises(ValueError):
        mc.state_index(32, 0, 2)


def test_policy_tables():
    from pulselib_amd.agents import FirstVisitMonteCarloGPU as G
    from pulselib_amd.agents import first_visit_mc_gpu as mc
    t = G.threshold_policy(17).table
    assert t.dtype == np.float32 and t.shape == (mc.N_STATES,)
    assert t[mc.state_index(16, 1, 11)] == 1.0 and t[mc.state_index(17, 0, 2)] == 0.0
    assert (G.uniform_policy().table == 0.5).all()
