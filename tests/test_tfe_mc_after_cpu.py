"""The host half of 2048 Monte-Carlo control on afterstates (agents/tfe_on_policy_mc_gpu.py, csrc/tfe_mc.hip:
pulse_tfe_mc_rollout_after, _after_canon, pulse_tfe_mc_learn_after, pulse_tfe_mc_evaluate_after, pulse_tfe_mc_table_fold_after): the
host's move against the oracle's step, the `first` bit against the set rule on host-played games, the host statement of the
learner against a dict-of-lists learner, the fold of a value table, the five entry points' argument checks, and the checkpoint's
kind.  Nothing here launches a kernel."""
import ctypes as C
import functools
import math
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

from tests.native_args import assert_refusals, opts
from tests.test_tfe_mc_cpu import BASE, COMMON, ROLLOUT_ONLY
from tests.test_tfe_mc_sym_cpu import BASE as EVAL_BASE, EVAL, TABLE
from tests.test_tfe_mc_table_cpu import BASE as MERGE_BASE, CASES as MERGE_CASES

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n,n_games", [(2, 400), (3, 80), (4, 24)])
def test_move_on_host_against_the_oracles_step(n, n_games):
    """Oracle-played games under uniform actions: the oracle's step is the move and then a spawn into one empty cell, so its board
    differs from the host's moved board in at most one cell (none where the moved board is full), the cell that differs was empty,
    and the step's reward is the reward of the host's merge score.  At least 2,000 moves per board side."""
    from oracle import oracle as orc
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    boards, score = np.zeros((n_games, n, n), dtype=np.int32), np.zeros(n_games, dtype=np.int64)
    rewards, dones = np.zeros(n_games, dtype=np.int32), np.zeros(n_games, dtype=np.uint8)
    seed = 40 + n
    orc.tfe_reset(boards, score, n, seed, 0)
    rng = np.random.default_rng(n)
    live, moves, unchanged, merged = np.ones(n_games, dtype=bool), 0, 0, 0
    for t in range(400):
        if not live.any():
            break
        before, before_score = boards.copy(), score.copy()
        actions = rng.integers(0, 4, n_games).astype(np.int64)
        orc.tfe_step(boards, score, actions, rewards, dones, n, seed, t + 1, 0)
        for g in np.nonzero(live)[0].tolist():
            want, merge = mc.move_on_host(before[g], int(actions[g]))
            differ = want != boards[g]
            assert differ.sum() <= 1 and (want[differ] == 0).all() and differ.sum() == int((want == 0).any()), (n, t, g)
            assert mc.reward_of_score(merge) == int(rewards[g]) and merge == int(score[g] - before_score[g]), (n, t, g)
            assert want.dtype == np.int64 and want.sum() == before[g].sum()                # a move keeps the tile sum
            moves, unchanged, merged = moves + 1, unchanged + int((want == before[g]).all()), merged + (merge > 0)
        live &= dones == 0
    assert moves >= 2000 and unchanged >= 20 and merged >= 500, (moves, unchanged, merged)


@functools.lru_cache(maxsize=None)
def _host_games(n, n_games, canonical=False, rounds=2):
    """Host-played games: round 0 on an empty table, round 1 on the table learnt from it.  Per round (roll-out, table after it)."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_after_on_host
    seed, fb, table, out = 11 + n, mc.frac_bits_for(0.9, 256), {}, []
    for r in range(rounds):
        o = rollout_after_on_host(n_games, n, 256, 0.1, 0.9, fb, table, seed, seed ^ mc.AGENT_KEY, seed ^ mc.TIE_KEY, 100 + r * n_games, r, canonical)
        assert o["truncated"] == 0
        mc.learn_after_on_host(o["keys"], o["steps"], o["lengths"], 0.9, fb, table)
        out.append((o, {k: (list(c), list(s)) for k, (c, s) in table.items()}))
    return out


def _per_game(o):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import unpack_steps
    a, r, f = unpack_steps(o["steps"])
    return [(o["keys"][:L, g], a[:L, g], r[:L, g], f[:L, g]) for g, L in enumerate(o["lengths"].tolist())]


@pytest.mark.parametrize("canonical", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("n,n_games", [(2, 800), (3, 250)])
def test_first_is_the_set_rule_on_host_games(n, n_games, canonical):
    """Equal afterstates of a game are consecutive, so "differs from the key recorded one move earlier" is
    "was not recorded earlier in the game".  Round 0 and round 1; the sample must hold at least 100 repeats to mean anything."""
    repeats = 0
    for o, _ in _host_games(n, n_games, canonical):
        for keys, _, _, flags in _per_game(o):
            seen, want = set(), []
            for k in keys.tolist():
                want.append(k not in seen)
                seen.add(k)
            assert flags.tolist() == want and flags[0] and all(k != 0 for k in keys.tolist())
            repeats += len(want) - sum(want)
    assert repeats >= 100, repeats


@pytest.mark.parametrize("gamma", [0.9, 0.5, 1.0])
def test_learn_after_on_host_against_a_dict_of_lists(gamma):
    """Games fed one at a time (B = 1) to learn_after_on_host and to a plain first-visit learner on afterstates: per game, backwards,
    an afterstate that was not recorded earlier in the game collects the return that FOLLOWS its move, then the move's reward enters.
    Counts are exact; each contribution is rounded to 2^-frac_bits, so every mean is within 2^-frac_bits (off by half of it at the most)."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    fb = mc.frac_bits_for(gamma, 256)
    games = [g for n in (2, 3) for o, _ in _host_games(n, 60) for g in _per_game(o)]
    returns, table = defaultdict(list), {}
    for keys, actions, rewards, flags in games:
        ks, G = keys.tolist(), 0.0
        for t in range(len(ks) - 1, -1, -1):
            if ks[t] not in ks[:t]:
                returns[ks[t]].append(G)
            G = gamma * G + float(rewards[t])
        steps = (actions | (rewards << 2) | (flags.astype(np.uint8) << 7)).astype(np.uint8)
        mc.learn_after_on_host(keys, steps, [len(keys)], gamma, fb, table)
    assert set(table) == set(returns) and len(table) > 100
    assert max(len(v) for v in returns.values()) >= 2 and any(v != 0.0 for vs in returns.values() for v in vs)
    for k, (cnt, total) in table.items():
        assert cnt == [len(returns[k]), 0, 0, 0] and total[1:] == [0, 0, 0]
        assert abs(mc.v_of_entry((cnt, total), fb) - sum(returns[k]) / len(returns[k])) <= 2.0 ** -fb, k
    assert mc.v_of_entry(([0] * 4, [0] * 4), fb) == 0.0                        # an afterstate never seen reads 0.0


def test_the_policy_rule_on_stated_values():
    """greedy_after_on_host on one board with stated entries and coins: q = r + gamma * v, in order, a tie by the coin of the plain key."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    board = np.array([[2, 2, 0], [0, 4, 0], [0, 0, 0]])
    keys, rewards = mc.afterstates_on_host(board)
    assert rewards == [2, 0, 2, 0] and len(set(keys)) == 4 and keys[0] == mc.pack_board([[4, 0, 0], [4, 0, 0], [0, 0, 0]])
    asked = []

    def coins(*words):
        def philox(seed, key, r):
            asked.append((seed, key, r))
            return [w << 31 for w in words] + [0]
        return philox
    assert mc.greedy_after_on_host(board, {}, 0.9, 4, 7, 3) == (None, keys, rewards)
    one = {keys[1]: ([1, 0, 0, 0], [16, 0, 0, 0])}                          # v = 1: q = 2, 0.9, 2, 0 -- actions 0 and 2 tie
    assert mc.greedy_after_on_host(board, one, 0.9, 4, 7, 3, philox=coins(1, 0, 1))[0] == 0
    assert mc.greedy_after_on_host(board, one, 0.9, 4, 7, 3, philox=coins(0, 1, 0))[0] == 2
    assert set(asked) == {(7, mc.pack_board(board), 3)}                     # the key of the state before the move
    del asked[:]
    big = {keys[3]: ([2, 0, 0, 0], [5 * 16 * 2, 0, 0, 0])}                  # v = 5: q = 2, 0, 2, 4.5 -- no coin decides
    assert mc.greedy_after_on_host(board, big, 0.9, 4, 7, 3, philox=coins(0, 0, 0))[0] == 3
    # symmetric: the mirror image of the board meets the same canonical afterstates under the mirrored actions
    ks, rs = mc.afterstates_on_host(board, symmetric=True)
    km, rm = mc.afterstates_on_host(board[:, ::-1], symmetric=True)
    assert [ks[0], ks[1], ks[2], ks[3]] == [km[2], km[1], km[0], km[3]] and rs == [rm[2], rm[1], rm[0], rm[3]]
    assert all(k == mc.canon_key_on_host(p, 3)[0] for k, p in zip(ks, keys))


@pytest.mark.parametrize("n", [2, 3])
def test_fold_values_on_host(n):
    """folding and then reading equals reading each key's canonical key and summing; the slots stay where they are; idempotent; and
    the fold of the table learnt from plain games on an empty table is the table learnt from the same games' canonical keys"""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    (o, plain), _ = _host_games(n, 60)
    folded = mc.fold_values_on_host(plain, n)
    want = defaultdict(lambda: [0, 0])
    for key, (cnt, total) in plain.items():
        entry = want[mc.canon_key_on_host(key, n)[0]]
        entry[0], entry[1] = entry[0] + cnt[0], entry[1] + total[0]
    assert {k: [c[0], s[0]] for k, (c, s) in folded.items()} == want and len(folded) < len(plain)
    assert all(c[1:] == [0, 0, 0] and s[1:] == [0, 0, 0] for c, s in folded.values())
    assert mc.fold_values_on_host(folded, n) == folded and all(mc.canon_key_on_host(k, n)[0] == k for k in folded)
    odd = {next(k for k in plain if mc.canon_key_on_host(k, n)[1] == 1): ([1, 2, 3, 4], [5, 6, 7, 8])}      # j* = 1: the Q fold would permute
    assert list(mc.fold_values_on_host(odd, n).values()) == [([1, 2, 3, 4], [5, 6, 7, 8])]
    assert list(mc.fold_table_on_host(odd, n).values()) != [([1, 2, 3, 4], [5, 6, 7, 8])]


def test_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    for name, struct, cases in (("pulse_tfe_mc_rollout_after", _native.TfeMCRollout, COMMON + ROLLOUT_ONLY),
                                ("pulse_tfe_mc_rollout_after_canon", _native.TfeMCRollout, COMMON + ROLLOUT_ONLY),
                                ("pulse_tfe_mc_learn_after", _native.TfeMCLearn, COMMON)):
        assert_refusals(lib, name, lambda **kw: opts(struct, **{**BASE, **kw}), cases)
    assert_refusals(lib, "pulse_tfe_mc_evaluate_after", lambda **kw: opts(_native.TfeMCEval, **{**EVAL_BASE, **kw}), TABLE + EVAL, 0.9)
    for gamma in (-0.01, 1.01, math.nan):
        assert lib.pulse_tfe_mc_evaluate_after(C.byref(opts(_native.TfeMCEval, **EVAL_BASE)), gamma, None) == -1
        assert lib.pulse_last_error() == b"pulse_tfe_mc_evaluate_after: gamma must be in [0, 1]"
    name = "pulse_tfe_mc_table_fold_after"
    assert_refusals(lib, name, lambda **kw: opts(_native.TfeMCMerge, **{**MERGE_BASE, "canonical": 1, **kw}), MERGE_CASES)
    assert lib.pulse_tfe_mc_table_fold_after(C.byref(opts(_native.TfeMCMerge, **{**MERGE_BASE, "canonical": 0})), None) == -1
    assert lib.pulse_last_error() == name.encode() + b": canonical must be 1 (the plain merge of a value table is pulse_tfe_mc_table_merge)"


def test_header_agrees_with_the_binding():
    from pulselib_amd import _native
    text = (ROOT / "include" / "pulse_env.h").read_text()
    assert C.sizeof(_native.TfeMCRollout) == 144 and C.sizeof(_native.TfeMCLearn) == 88            # the mode adds no field
    assert C.sizeof(_native.TfeMCEval) == 128 and C.sizeof(_native.TfeMCMerge) == 56
    two, gamma = (C.c_int, [C.c_void_p, C.c_void_p]), (C.c_int, [C.c_void_p, C.c_double, C.c_void_p])
    for name, struct, sig in (("pulse_tfe_mc_rollout_after", "PulseTfeMCRollout", two), ("pulse_tfe_mc_rollout_after_canon", "PulseTfeMCRollout", two),
                              ("pulse_tfe_mc_learn_after", "PulseTfeMCLearn", two), ("pulse_tfe_mc_evaluate_after", "PulseTfeMCEval", gamma),
                              ("pulse_tfe_mc_table_fold_after", "PulseTfeMCMerge", two)):
        extra = r"double gamma, " if sig is gamma else ""
        assert re.search(r"int %s\(const %s\* o, %svoid\* stream\);" % (name, struct, extra), text), name
        assert _native.SYMBOLS[name] == sig, name


# ------------------------------------------------------------------ the checkpoint's kind, and what the Python layer refuses
SCALARS = dict(n=3, gamma=0.9, epsilon=0.1, frac_bits=22, max_steps=64, seed=5, board_id0=7, round=2, symmetric=0, n_games=300)


def test_checkpoint_keeps_the_kind(tmp_path):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    keys = np.array([0x12, 0x211], dtype=np.uint64)
    cnt, total = np.array([[3, 0, 0, 0], [1, 0, 0, 0]], dtype=np.int64), np.array([[1 << 30, 0, 0, 0], [5, 0, 0, 0]], dtype=np.int64)
    for kind in (1, 0):
        path = tmp_path / f"kind{kind}.npz"
        mc.write_checkpoint(path, keys, cnt, total, afterstate=kind, **SCALARS)
        f = mc.read_checkpoint(path)
        assert f["afterstate"] is bool(kind) and np.array_equal(f["cnt"], cnt) and np.array_equal(f["sum"], total)
        with np.load(path, allow_pickle=False) as z:
            assert sorted(z.files) == sorted(["version", "keys", "cnt", "sum", "afterstate"] + list(SCALARS)) and z["afterstate"].shape == ()
    old = tmp_path / "old.npz"                                              # a checkpoint without the scalar is a Q table, as before
    mc.write_checkpoint(old, keys, cnt, total, **SCALARS)
    assert mc.read_checkpoint(old)["afterstate"] is False
    with np.load(old, allow_pickle=False) as z:
        assert "afterstate" not in z.files
    with pytest.raises(ValueError, match="exactly the scalars"):
        mc.write_checkpoint(tmp_path / "x.npz", keys, cnt, total, afterstate=1, **{k: v for k, v in SCALARS.items() if k != "seed"})


def test_gpu_class_refuses_cpu_devices():
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        OnPolicyFirstVisitMCTFEGPU(torch.device("cpu"), 64, afterstate=True)
