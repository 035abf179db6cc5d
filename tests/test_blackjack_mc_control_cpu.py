"""The host half of on-policy first-visit Monte-Carlo control for Blackjack (pulselib_amd/agents/on_policy_first_visit_mc.py,
on_policy_first_visit_mc_gpu.py, csrc/blackjack_mc.hip): the CPU class against the fixture recorded from the reference, the
action histogram's reduction and the host statement of the policy improvement, and the two entry points' argument checks.
Nothing here launches a kernel."""
import ctypes as C
import math
import random
import re
from pathlib import Path

import numpy as np
import pytest

from tests.native_args import assert_refusals, opts

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "opfvmc.npz")


def _episodes():
    steps, out, at = GOLDEN["steps"], [], 0
    for n in GOLDEN["episode_lengths"].tolist():
        out.append([((int(r[0]), int(r[1]), int(r[2])), int(r[3]), int(r[4])) for r in steps[at:at + n]])
        at += n
    return out


def action_histogram(episodes):
    """The host's count of pair first visits in the launch's layout (shared with tests/test_blackjack_mc_control_gpu.py)."""
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    h = np.zeros(mc.ACC_LEN, dtype=np.int64)
    for ep in episodes:
        seen, negative = set(), int(ep[-1][2] < 0)
        for t, (s, a, _) in enumerate(ep):
            if (s, a) not in seen:
                seen.add((s, a))
                i = mc.state_index(*s)
                h[mc.cell_stand(i, negative) if a == mc.STAND else mc.cell_hit(i, len(ep) - 1 - t, negative)] += 1
    return h.reshape(mc.N_STATES, mc.CELLS)


def test_fixture_holds_the_cases_it_is_for():
    eps = _episodes()
    assert any(len(e) == 1 for e in eps)
    assert any(len({(s, a) for s, a, _ in e}) < len(e) for e in eps), "no pair repeats within an episode"
    assert all(a == 0 and r == 0 for e in eps for _, a, r in e[:-1]) and all(e[-1][2] in (-1, 1) for e in eps)
    q = dict(zip(map(tuple, GOLDEN["r0/q_keys"].tolist()), GOLDEN["r0/q_values"].tolist()))
    assert q[(16, 0, 10, 0)] == q[(16, 0, 10, 1)] == -1.0 and q[(14, 1, 9, 0)] == q[(14, 1, 9, 1)] == 0.0


@pytest.mark.parametrize("run", range(4))
def test_cpu_class_reproduces_the_reference(run):
    """Key sets in the tables' own order, counts, sums, q and probabilities to the last bit, and the draws of action()."""
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    gamma, epsilon = float(GOLDEN[f"r{run}/gamma"]), float(GOLDEN[f"r{run}/epsilon"])
    random.seed(int(GOLDEN["seed"]))
    agent = OnPolicyFirstVisitMC(gamma, epsilon)
    for ep in _episodes():
        agent.learn(ep)
    draws = [agent.action(tuple(s)) for s in GOLDEN[f"r{run}/draw_states"].tolist()]
    assert draws == GOLDEN[f"r{run}/draws"].tolist()
    for name, table in (("q", agent.q), ("returns", agent.returns), ("policy", agent.policy)):
        keys = list(map(tuple, GOLDEN[f"r{run}/{name}_keys"].tolist()))
        assert list(table) == keys, name
        got = np.array([table[k] for k in keys], dtype=np.float64)
        assert got.tobytes() == GOLDEN[f"r{run}/{name}_values"].tobytes(), name
    assert len(agent.q) > len(agent.returns) > 40                          # unseen pairs of visited states read (and enter) as 0.0


@pytest.mark.parametrize("gamma", [0.5, 0.9])
def test_action_histogram_reduction_matches_the_cpu_class(gamma):
    """counts exactly; sums bit-equal at gamma 0.5 (every partial sum is a multiple of 2^-15 below 2^53), within n^2 * 2^-52 at
    gamma 0.9 (the bound on a float64 running sum of n terms <= 1, once for each side): tests/test_blackjack_mc_cpu.py's bounds."""
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    from pulselib_amd.agents.on_policy_first_visit_mc_gpu import returns_from_action_histogram
    eps = _episodes()
    cpu = OnPolicyFirstVisitMC(gamma, 0.1)
    for ep in eps:
        cpu.learn(ep)
    got = returns_from_action_histogram(action_histogram(eps), gamma)
    assert set(got) == set(cpu.returns) and len(got) > 40
    assert max(c for _, c in cpu.returns.values()) >= 5
    for pair, (total, count) in cpu.returns.items():
        assert got[pair][1] == count, pair
        assert all(isinstance(x, int) for x in pair)
        if gamma == 0.5:
            assert got[pair][0] == total, (pair, got[pair][0], total)
        else:
            assert abs(got[pair][0] - total) <= count * count * 2.0 ** -52, (pair, got[pair][0], total)


def handmade_histogram():
    """(histogram, {name: state index}) for the improvement's cases (shared with the GPU test).  gamma 0.5 keeps every q exact."""
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    h = np.zeros(mc.ACC_LEN, dtype=np.int64)
    at = {"unvisited": mc.state_index(12, 0, 2), "hit_only": mc.state_index(13, 0, 3), "stand_only": mc.state_index(14, 0, 4),
          "hit_wins": mc.state_index(11, 0, 5), "stand_wins": mc.state_index(20, 0, 6), "tie_a": mc.state_index(16, 0, 10),
          "tie_b": mc.state_index(16, 1, 10), "tie_unseen": mc.state_index(15, 0, 7), "last": mc.N_STATES - 1}
    h[mc.cell_hit(at["hit_only"], 1, 0)] = 3                               # q_hit = +0.5 against the unseen stand's 0.0: hit
    h[mc.cell_stand(at["stand_only"], 1)] = 4                              # q_stand = -1 against the unseen hit's 0.0: hit
    h[mc.cell_hit(at["hit_wins"], 1, 0)], h[mc.cell_hit(at["hit_wins"], 0, 1)], h[mc.cell_stand(at["hit_wins"], 1)] = 6, 1, 2
    h[mc.cell_stand(at["stand_wins"], 0)], h[mc.cell_stand(at["stand_wins"], 1)], h[mc.cell_hit(at["stand_wins"], 0, 1)] = 9, 1, 5
    for name in ("tie_a", "tie_b"):                                        # q_hit = (2 * 0.5 - 1 * 1) / 3 = 0 = q_stand = (1 - 1) / 2
        h[mc.cell_hit(at[name], 1, 0)], h[mc.cell_hit(at[name], 0, 1)] = 2, 1
        h[mc.cell_stand(at[name], 0)], h[mc.cell_stand(at[name], 1)] = 1, 1
    h[mc.cell_hit(at["tie_unseen"], 2, 0)], h[mc.cell_hit(at["tie_unseen"], 2, 1)] = 7, 7     # q_hit = 0.0 = the unseen stand
    h[mc.cell_hit(at["last"], 15, 1)], h[mc.cell_stand(at["last"], 0)] = 1, 1                 # the layout's last cells: stand wins
    return h.reshape(mc.N_STATES, mc.CELLS), at


@pytest.mark.parametrize("epsilon", [0.1, 0.0, 1.0])
def test_improve_on_host(epsilon):
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    h, at = handmade_histogram()
    before = np.linspace(0.2, 0.8, mc.N_STATES).astype(np.float32)
    coins = np.zeros(mc.N_STATES, dtype=bool)
    coins[at["tie_a"]] = True                                              # tie_a goes to stand, tie_b and tie_unseen to hit
    q, after = mc.improve_on_host(h, 0.5, epsilon, before, coins)
    assert q.shape == (mc.N_STATES, 2) and q.dtype == np.float64 and after.dtype == np.float32
    hit_p, stand_p = np.float32(1 - epsilon + epsilon / 2), np.float32(epsilon / 2)
    expect = {"hit_only": ((0.5, 0.0), hit_p), "stand_only": ((0.0, -1.0), hit_p), "hit_wins": ((2.0 / 7.0, -1.0), hit_p),
              "stand_wins": ((-1.0, 0.8), stand_p), "tie_a": ((0.0, 0.0), stand_p), "tie_b": ((0.0, 0.0), hit_p),
              "tie_unseen": ((0.0, 0.0), hit_p), "last": ((-(0.5 ** 15), 1.0), stand_p)}
    for name, (qs, p) in expect.items():
        assert tuple(q[at[name]]) == qs and after[at[name]] == p, (name, q[at[name]], after[at[name]])
    untouched = np.ones(mc.N_STATES, dtype=bool)
    untouched[[at[n] for n in expect]] = False
    assert untouched[at["unvisited"]] and np.array_equal(after[untouched], before[untouched]) and not q[untouched].any()
    coins[:] = True                                                        # the other coin: only the ties that went to hit move
    q2, after2 = mc.improve_on_host(h, 0.5, epsilon, before, coins)
    moved = np.nonzero(after2 != after)[0].tolist()
    assert np.array_equal(q2, q) and (sorted(moved) == sorted(at[n] for n in ("tie_b", "tie_unseen")) if epsilon < 1.0 else moved == [])
    if epsilon == 1.0:
        assert hit_p == stand_p == np.float32(0.5)


def test_control_rollout_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    base = dict(n_games=64, n_episodes=1, hit_prob=0x10000, acc=0x20000, stats=0x30000)   # never dereferenced: every case fails its check first
    cases = [(dict(acc=None), b"acc is null"), (dict(hit_prob=None), b"hit_prob is null"), (dict(stats=None), b"stats is null"),
             (dict(n_games=0), b"n_games must be positive"), (dict(n_games=-5), b"n_games must be positive"),
             (dict(n_episodes=0), b"n_episodes must be positive"), (dict(n_episodes=-1), b"n_episodes must be positive"),
             (dict(n_games=1 << 20, n_episodes=1 << 12), b"below 2^32"),
             (dict(acc=0x20004), b"8-byte aligned"), (dict(stats=0x30004), b"8-byte aligned"),
             (dict(hit_prob=0x10002), b"4-byte aligned"), (dict(decks_src=0x40001), b"4-byte aligned"),
             (dict(trace=0x50008), b"16-byte aligned"), (dict(max_blocks=-1), b"max_blocks"),
             (dict(reserved0=1), b"reserved0 must be 0")]
    control = assert_refusals(lib, "pulse_blackjack_mc_control_rollout", lambda **kw: opts(_native.BlackjackMCControl, **{**base, **kw}), cases)
    value = assert_refusals(lib, "pulse_blackjack_mc_rollout", lambda **kw: opts(_native.BlackjackMC, **{**base, **kw}), cases)
    # the value entry point: the same message under its own name
    assert value == [err.replace(b"pulse_blackjack_mc_control_rollout", b"pulse_blackjack_mc_rollout") for err in control]


def test_improve_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    base = dict(acc=0x20000, hit_prob=0x10000, q=0x30000, gamma=0.9, epsilon=0.1)
    cases = [(dict(acc=None), b"acc is null"), (dict(hit_prob=None), b"hit_prob is null"),
             (dict(acc=0x20004), b"8-byte aligned"), (dict(q=0x30004), b"8-byte aligned"), (dict(hit_prob=0x10002), b"4-byte aligned"),
             (dict(epsilon=-0.01), b"epsilon must be in [0, 1]"), (dict(epsilon=1.5), b"epsilon must be in [0, 1]"),
             (dict(epsilon=math.nan), b"epsilon must be in [0, 1]"),
             (dict(gamma=math.inf), b"gamma must be finite"), (dict(gamma=math.nan), b"gamma must be finite"),
             (dict(reserved0=1), b"reserved0 / reserved1 must be 0"), (dict(reserved1=-1), b"reserved0 / reserved1 must be 0")]
    assert_refusals(lib, "pulse_blackjack_mc_improve", lambda **kw: opts(_native.BlackjackMCImprove, **{**base, **kw}), cases)


def test_header_macros_agree_with_the_binding():
    from pulselib_amd import _native
    from pulselib_amd.agents import on_policy_first_visit_mc_gpu as mc
    text = (ROOT / "include" / "pulse_env.h").read_text()
    consts = {n: int(v, 0) for n, v in re.findall(r"#define (PULSE_BJ_MCC_(?:CELLS|TIE_KEY))\s+(\w+?)(?:ull)?\s", text)}
    assert consts == {"PULSE_BJ_MCC_CELLS": _native.BJ_MCC_CELLS, "PULSE_BJ_MCC_TIE_KEY": _native.BJ_MCC_TIE_KEY} and _native.BJ_MCC_CELLS == 34
    assert _native.BJ_MCC_TIE_KEY not in (0, 0xB1AC7AC4D3A1E5)             # apart from the shuffle's key and the policy's
    env = {"PULSE_BJ_MCC_CELLS": 34, "PULSE_BJ_MC_MAX_ACTIONS": 16, "PULSE_BJ_MC_STATES": 1024}
    hit = re.search(r"#define PULSE_BJ_MCC_CELL_HIT\(state, k, negative\)\s+(\(.*\))\s*$", text, re.M).group(1)
    stand = re.search(r"#define PULSE_BJ_MCC_CELL_STAND\(state, negative\)\s+(\(.*\))\s*$", text, re.M).group(1)
    acc_len = re.search(r"#define PULSE_BJ_MCC_ACC_LEN\s+(\(.*\))\s*$", text, re.M).group(1)
    assert eval(acc_len, {"__builtins__": {}}, env) == _native.BJ_MCC_ACC_LEN == mc.ACC_LEN == 1024 * 34
    cells = set()
    for s in (0, 377, 1023):
        for neg in (0, 1):
            cells.add(eval(stand, {"__builtins__": {}}, {**env, "state": s, "negative": neg}))
            assert max(cells) == mc.cell_stand(s, neg)
            for k in range(16):
                c = eval(hit, {"__builtins__": {}}, {**env, "state": s, "k": k, "negative": neg})
                assert c == mc.cell_hit(s, k, neg) and c // 34 == s
                cells.add(c)
    assert len(cells) == 3 * 34 and max(cells) == mc.ACC_LEN - 1
    # the value learner's layout is what it was
    old = {n: int(v) for n, v in re.findall(r"#define (PULSE_BJ_MC_(?:MAX_ACTIONS|STATES))\s+(\d+)", text)}
    assert old == {"PULSE_BJ_MC_MAX_ACTIONS": 16, "PULSE_BJ_MC_STATES": 1024} and _native.BJ_MC_ACC_LEN == 32768
    assert "#define PULSE_BJ_MC_CELL(state, k, negative) ((((state) * PULSE_BJ_MC_MAX_ACTIONS + (k)) * 2) + (negative))" in text
    assert C.sizeof(_native.BlackjackMCControl) == C.sizeof(_native.BlackjackMC) == 72 and C.sizeof(_native.BlackjackMCImprove) == 64


def test_gpu_class_refuses_cpu_devices():
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCGPU
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        OnPolicyFirstVisitMCGPU(torch.device("cpu"), 0.9, 0.1)
