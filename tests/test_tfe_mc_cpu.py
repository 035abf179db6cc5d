"""The host half of on-policy first-visit Monte-Carlo control for 2048 (pulselib_amd/agents/tfe_on_policy_mc_gpu.py,
csrc/tfe_mc.hip): the run-mask first-visit rule against the reference's dict rule on oracle-played games, the host statement of the
learner against the CPU class, the tie coins, the frac_bits rule and the two entry points' argument checks.  Nothing here launches
a kernel."""
import ctypes as C
import math
import random
import re
from pathlib import Path

import numpy as np
import pytest

from tests.native_args import assert_refusals, opts

ROOT = Path(__file__).resolve().parent.parent


def _uniform_games(n, n_games, seed):
    """oracle-played games under the uniform policy (an empty table), per game (keys, actions, rewards, flags)"""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    o = rollout_on_host(n_games, n, 256, 0.1, {}, seed, seed ^ mc.AGENT_KEY, seed ^ mc.TIE_KEY, 100, 0)
    assert o["truncated"] == 0
    a, r, f = mc.unpack_steps(o["steps"])
    return o, [(o["keys"][:L, g], a[:L, g], r[:L, g], f[:L, g]) for g, L in enumerate(o["lengths"].tolist())]


@pytest.mark.parametrize("n,n_games", [(2, 800), (3, 250)])
def test_run_mask_is_the_dict_rule_on_oracle_games(n, n_games):
    """Equal states of a game are consecutive, so four bits per game decide a first visit.  At n = 2 the board
    fills within a few moves and repeats are common; the sample must hold at least 100 repeated pairs to mean anything."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    _, games = _uniform_games(n, n_games, 11 + n)
    repeats = 0
    for keys, actions, _, flags in games:
        want = mc.first_visit_flags_on_host(keys, actions)
        assert np.array_equal(mc.run_mask_flags_on_host(keys, actions), want)
        assert np.array_equal(flags, want)                                 # the roll-out's own bit 7
        repeats += int((~want).sum())
        assert all(k != 0 for k in keys.tolist())
    assert repeats >= 100, repeats


def test_python_philox_is_the_oracles():
    from oracle import oracle as orc
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import philox4x32
    for args in [(0, 0, 0), (5, 1 << 40, 3), (0xDEADBEEFCAFEF00D, 0x123456789ABCDEF, (1 << 63) + 17), (1, 2, 1 << 32)]:
        assert philox4x32(*args) == orc.philox4x32(*args).tolist(), args


@pytest.mark.parametrize("n,gamma", [(2, 0.9), (3, 0.9), (3, 0.5), (3, 1.0)])
def test_learn_on_host_against_the_cpu_class(n, gamma):
    """Games fed one at a time (B = 1).  Each contribution is rounded to 2^-frac_bits, so it is off by at most 2^-(frac_bits + 1),
    and so is a mean; the CPU class's own float64 running sum is off by ~1e-13.  Every q within 2^-frac_bits, and the pairs with a
    count are exactly the pairs the CPU class recorded."""
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    _, games = _uniform_games(n, 60, 5)
    fb = mc.frac_bits_for(gamma, 256)
    random.seed(3)
    cpu, table = OnPolicyFirstVisitMC(gamma, 0.1, n_actions=4), {}
    for keys, actions, rewards, flags in games:
        cpu.learn([((int(k),), int(a), int(r)) for k, a, r in zip(keys.tolist(), actions.tolist(), rewards.tolist())])
        steps = (actions | (rewards << 2) | (flags.astype(np.uint8) << 7)).astype(np.uint8)
        mc.learn_on_host(keys, steps, [len(keys)], gamma, fb, table)
    seen = {(k, a) for k, (cnt, _) in table.items() for a in range(4) if cnt[a] > 0}
    assert seen == set(cpu.returns) and len(seen) > 100
    assert max(cnt[a] for cnt, _ in table.values() for a in range(4)) >= 2     # some mean is of more than one return
    for (k, a), (total, count) in cpu.returns.items():
        assert table[k][0][a] == count
        assert abs(mc.q_of_entry(table[k], fb)[a] - cpu.q[(k, a)]) <= 2.0 ** -fb, (k, a)
    for k, e in table.items():                                             # a pair never seen reads 0.0, as the defaultdict
        for a in range(4):
            assert (k, a) in seen or (mc.q_of_entry(e, fb)[a] == 0.0 and cpu.q.get((k, a), 0.0) == 0.0)


def test_stated_coins_give_the_stated_greedy_action():
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import greedy_on_host
    asked = []

    def coins(*words):
        def philox(seed, key, r):
            asked.append((seed, key, r))
            return [w << 31 for w in words] + [0xFFFFFFFF]
        return philox

    unseen = ([0] * 4, [0] * 4)                                            # q = 0, 0, 0, 0
    for words, want in [((0, 0, 0), 0), ((1, 0, 0), 1), ((1, 1, 0), 2), ((1, 0, 1), 3), ((0, 0, 1), 3), ((0, 1, 0), 2)]:
        assert greedy_on_host(unseen, 0x21, 7, 3, coins(*words)) == want, words
    assert asked and set(asked) == {(7, 0x21, 3)}
    three = ([2, 0, 0, 0], [-10, 0, 0, 0])                                 # q = -5, 0, 0, 0: action 1 wins outright, 2 and 3 tie with it at 0
    for words, want in [((1, 0, 0), 1), ((0, 0, 0), 1), ((0, 1, 0), 2), ((0, 1, 1), 3), ((1, 0, 1), 3)]:
        assert greedy_on_host(three, 9, 0, 0, coins(*words)) == want, words
    del asked[:]
    clear = ([1, 2, 4, 1], [3, 8, 20, 4])                                  # q = 3, 4, 5, 4: no tie, no coin drawn
    assert greedy_on_host(clear, 9, 0, 0, coins(1, 1, 1)) == 2 and not asked
    late = ([1, 1, 1, 1], [1, 1, 2, 0])                                    # q = 1, 1, 2, 0: the tie's coin does not matter to the larger q after it
    assert greedy_on_host(late, 9, 0, 0, coins(1, 0, 0)) == 2 and greedy_on_host(late, 9, 0, 0, coins(0, 0, 0)) == 2
    big = ([3, 3, 1, 1], [(1 << 61) + 3, (1 << 61) + 3, 0, 0])             # equal int64 sums far above 2^53: still a tie
    assert greedy_on_host(big, 9, 0, 0, coins(1, 0, 0)) == 1 and greedy_on_host(big, 9, 0, 0, coins(0, 1, 1)) == 0


FRAC_CASES = [(0.9, 1024, 22), (0.9, 8, 22), (1.0, 65535, 9), (0.0, 1024, 25), (0.5, 100, 24), (1.0, 1, 25), (0.99, 1024, 19)]


@pytest.mark.parametrize("gamma,max_steps,want", FRAC_CASES)
def test_frac_bits_rule(gamma, max_steps, want):
    """the largest f <= 30 with G_max * 2^f * 2^32 < 2^62, G_max = 17 * min(max_steps, 1 / (1 - gamma)); the library accepts it and
    refuses the next one"""
    from pulselib_amd import _native
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import frac_bits_for
    g_max = 17.0 * min(max_steps, 1.0 / (1.0 - gamma) if gamma < 1.0 else math.inf)
    assert frac_bits_for(gamma, max_steps) == want
    assert g_max * 2.0 ** want * 2.0 ** 32 < 2.0 ** 62 <= g_max * 2.0 ** (want + 1) * 2.0 ** 32
    lib = _native.lib()
    for fn, struct in ((lib.pulse_tfe_mc_rollout, _native.TfeMCRollout), (lib.pulse_tfe_mc_learn, _native.TfeMCLearn)):
        o = opts(struct, **{**BASE, "gamma": gamma, "max_steps": max_steps, "frac_bits": want + 1})
        assert fn(C.byref(o), None) == -1 and b"frac_bits" in lib.pulse_last_error()
        o = opts(struct, **{**BASE, "gamma": gamma, "max_steps": max_steps, "frac_bits": want, "keys": None})
        assert fn(C.byref(o), None) == -1 and b"keys is null" in lib.pulse_last_error()      # past the frac_bits check


# never dereferenced: every case fails its check first
BASE = dict(entries=0x100000, capacity=1 << 10, n_games=64, n=3, max_steps=128, frac_bits=22, gamma=0.9, epsilon=0.1,
            keys=0x200000, steps=0x300000, lengths=0x400000, total_score=0x500000, episode_reward=0x600000, stats=0x700000)
COMMON = [(dict(entries=None), b"entries is null"), (dict(entries=0x100040), b"128-byte aligned"), (dict(entries=0x100008), b"128-byte aligned"),
          (dict(capacity=0), b"power of two"), (dict(capacity=1000), b"power of two"), (dict(capacity=(1 << 20) + 1), b"power of two"),
          (dict(n=1), b"board side must be 2..4"), (dict(n=5), b"board side must be 2..4"), (dict(n=-3), b"board side must be 2..4"),
          (dict(n_games=0), b"n_games must be positive"), (dict(n_games=-7), b"n_games must be positive"),
          (dict(max_steps=0), b"max_steps must be in 1..65535"), (dict(max_steps=65536), b"max_steps must be in 1..65535"),
          (dict(max_steps=-1), b"max_steps must be in 1..65535"),
          (dict(gamma=-0.01), b"gamma must be in [0, 1]"), (dict(gamma=1.01), b"gamma must be in [0, 1]"), (dict(gamma=math.nan), b"gamma must be in [0, 1]"),
          (dict(epsilon=-0.01), b"epsilon must be in [0, 1]"), (dict(epsilon=1.5), b"epsilon must be in [0, 1]"),
          (dict(epsilon=math.nan), b"epsilon must be in [0, 1]"),
          (dict(frac_bits=-1), b"frac_bits"), (dict(frac_bits=23), b"frac_bits"), (dict(frac_bits=31), b"frac_bits"),
          (dict(keys=None), b"keys is null"), (dict(steps=None), b"steps is null"), (dict(lengths=None), b"lengths is null"),
          (dict(stats=None), b"stats is null"), (dict(keys=0x200004), b"8-byte aligned"), (dict(stats=0x700004), b"8-byte aligned"),
          (dict(lengths=0x400002), b"4-byte aligned"), (dict(reserved0=1), b"reserved0 must be 0")]
ROLLOUT_ONLY = [(dict(total_score=None), b"total_score is null"), (dict(episode_reward=None), b"episode_reward is null"),
                (dict(total_score=0x500004), b"total_score must be 8-byte aligned"), (dict(episode_reward=0x600002), b"episode_reward must be 4-byte aligned")]


def test_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    for name, struct, cases in (("pulse_tfe_mc_rollout", _native.TfeMCRollout, COMMON + ROLLOUT_ONLY), ("pulse_tfe_mc_learn", _native.TfeMCLearn, COMMON)):
        assert_refusals(lib, name, lambda **kw: opts(struct, **{**BASE, **kw}), cases)


def test_header_agrees_with_the_binding():
    from pulselib_amd import _native
    text = (ROOT / "include" / "pulse_env.h").read_text()
    consts = {n: int(v) for n, v in re.findall(r"#define (PULSE_TFE_MC_\w+)\s+(\d+)", text)}
    assert consts == {"PULSE_TFE_MC_ENTRY_BYTES": _native.TFE_MC_ENTRY_BYTES, "PULSE_TFE_MC_MAX_PROBE": _native.TFE_MC_MAX_PROBE,
                      "PULSE_TFE_MC_R_MAX": _native.TFE_MC_R_MAX} and _native.TFE_MC_ENTRY_BYTES == 128
    assert C.sizeof(_native.TfeMCRollout) == 144 and C.sizeof(_native.TfeMCLearn) == 88
    for f in ("entries", "capacity", "n_games", "n", "max_steps", "frac_bits", "gamma", "epsilon"):     # the shared head
        assert getattr(_native.TfeMCRollout, f).offset == getattr(_native.TfeMCLearn, f).offset
    for struct in ("PulseTfeMCRollout", "PulseTfeMCLearn"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        names = [n for decl in re.sub(r"/\*.*?\*/", "", body).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        want = [f for f, _ in getattr(_native, struct.replace("Pulse", "", 1))._fields_]
        assert names == want, (struct, names, want)


def test_gpu_class_refuses_cpu_devices_and_bad_settings():
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        OnPolicyFirstVisitMCTFEGPU(torch.device("cpu"), 64)
