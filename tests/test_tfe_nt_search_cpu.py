"""The 2048 n-tuple network's expectimax play without a GPU: the library's two entry points and their
refusals, the host mirror search_nt_on_host (pulselib_amd/agents/tfe_ntuple_td_gpu.py) on hand-worked boards -- E as exact rationals
from a move written out in plain Python -- and what the compiler made of the kernels."""
import ctypes as C
import functools
import re
from fractions import Fraction

import numpy as np

from tests.native_args import assert_refusals
from tests.tfe_nt_support import BATCH, CASES, CRAFTED, EPSILON, NET_CASES, P, ROOT, SEARCH_CASES, SEARCH_UNIT, TUPLES, WEIGHTS, assert_exports, assert_no_scratch, bits, opts, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of

WORKED, DEAD, ONE_MERGE = key_of(CRAFTED["worked"]), key_of(CRAFTED["dead"]), key_of(CRAFTED["one_merge"])


def _zero():
    return weights("zero")


def test_library_exports_the_two_entry_points():
    from pulselib_amd import _native
    _, text = assert_exports((("pulse_tfe_nt_search", "PulseTfeNtSearch"), ("pulse_tfe_nt_evaluate_search", "PulseTfeNtEval")), [C.c_void_p, C.c_void_p],
                             r"int %s\(const %s\* o, void\* stream\);")
    assert C.sizeof(_native.TfeNtSearch) == 176 and C.sizeof(_native.TfeNtEval) == 208         # the static_asserts of csrc/tfe_ntuple*.hip
    assert [f[0] for f in _native.TfeNtSearch._fields_] == ["net", "n_boards", "reserved0", "gamma", "tie_seed", "round", "boards", "q", "action",
                                                            "candidates", "reserved1"]
    assert _native.TfeNtSearch.boards.offset == 136 and re.search(r"typedef struct PulseTfeNtSearch \{", text)
    assert "static_assert(sizeof(PulseTfeNtSearch) == 176" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_search.hip").read_text()


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
def test_search_refuses_without_gpu():
    from pulselib_amd import _native
    assert len(assert_refusals(_native.lib(), "pulse_tfe_nt_search", functools.partial(opts, _native.TfeNtSearch), SEARCH_CASES)) == len(SEARCH_CASES)


def test_evaluate_search_refuses_what_evaluate_refuses():
    """the same struct, the same checks, under its own name"""
    from pulselib_amd import _native
    cases = CASES["pulse_tfe_nt_evaluate"]
    assert len(cases) == len(NET_CASES + WEIGHTS + BATCH + EPSILON) + 6
    errors = assert_refusals(_native.lib(), "pulse_tfe_nt_evaluate_search", functools.partial(opts, _native.TfeNtEval), cases)
    assert all(e.startswith(b"pulse_tfe_nt_evaluate_search: ") for e in errors)


def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    for name in ("search", "search_launch", "evaluate_search", "evaluate_search_launch"):
        assert callable(getattr(NTupleTDAfterstateTFEGPU, name))
    assert _nt().TILE_ODDS == (float(P[0]), float(P[1])) and P[0] + P[1] == 1


# ------------------------------------------------------------------ the definition once more, in plain Python and exact rationals
def _squash(row):
    """(the row of nibbles squashed to the left, the reward's score), TFE.py:85-101"""
    out, score, merged = [], 0, False
    for v in row:
        if v == 0:
            continue
        if out and out[-1] == v and not merged:
            out[-1], score, merged = v + 1, score + (2 << v), True
        else:
            out.append(v)
            merged = False
    return out + [0] * (4 - len(out)), score


def _move(cells, a):
    """(cells after move a, merge score): 0 left, 1 up, 2 right, 3 down"""
    lines = {0: [[4 * r + c for c in range(4)] for r in range(4)], 2: [[4 * r + 3 - c for c in range(4)] for r in range(4)],
             1: [[4 * r + c for r in range(4)] for c in range(4)], 3: [[4 * (3 - r) + c for r in range(4)] for c in range(4)]}[a]
    out, total = list(cells), 0
    for line in lines:
        row, score = _squash([cells[i] for i in line])
        total += score
        for i, v in zip(line, row):
            out[i] = v
    return out, total


def _reward(score):
    return score.bit_length() - 1 if score > 0 else 0


def _exact(key, value=lambda cells: Fraction(0), gamma=Fraction(1)):
    """per move a: None for a non-candidate, else (E_a, q_a) as Fractions"""
    cells = [(key >> (4 * i)) & 15 for i in range(16)]
    out = []
    for a in range(4):
        after, score = _move(cells, a)
        if after == cells:
            out.append(None)
            continue
        empty = [c for c in range(16) if after[c] == 0]
        total = Fraction(0)
        for c in empty:
            for k in (1, 2):
                chance = list(after)
                chance[c] = k
                best = [(_reward(s) + gamma * value(b)) for b, s in (_move(chance, m) for m in range(4)) if b != chance]
                total += P[k - 1] * (max(best) if best else 0)
        out.append((total / len(empty), _reward(score) + gamma * total / len(empty)))
    return out


def test_gamma_zero_is_the_one_ply_policy():
    nt = _nt()
    rng = np.random.default_rng(21)
    nib = (rng.integers(1, 9, (300, 16)) * (rng.random((300, 16)) < .7)).astype(np.uint64)
    keys = (nib << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    w = rng.standard_normal(nt.tuple_offsets(TUPLES)[1]).astype(np.float32)
    look, ply = nt.search_nt_on_host(keys, w, TUPLES, True, 0.0, 9, 4), nt.greedy_nt_on_host(keys, w, TUPLES, True, 0.0, 9, 4)
    cand = look["after"] != keys[:, None]
    assert cand.any(axis=1).sum() > 250 and not cand.all()
    assert np.array_equal(bits(look["q"]), bits(np.where(cand, look["rewards"].astype(np.float64), 0.0)))
    assert np.array_equal(look["action"], ply["action"]) and np.array_equal(look["candidates"], (cand << np.arange(4)).sum(axis=1))
    # ... and gamma enters: the same boards at gamma 1 choose otherwise somewhere
    assert not np.array_equal(nt.search_nt_on_host(keys, w, TUPLES, True, 1.0, 9, 4)["action"], ply["action"])


def test_a_hand_worked_board_on_zero_weights():
    """Left (a = 0) makes 2 . . . of the first row: reward 2, three empty cells.  A 4-tile in any of them merges with that 4 for reward
    3, a 2-tile merges with nothing and no tile meets its like below: m = 3 for k = 2, 0 for k = 1, E_0 = 3 * (3 P_2) / 3 = 3 P_2 and
    q_0 = 2 + 3 P_2; right is its mirror image.  Every term is a multiple of 2^-24 below 2^5, so S is exact and E rounds once, in the
    division: the float64 E is float(the exact E)."""
    nt = _nt()
    look = nt.search_nt_on_host([WORKED], _zero(), TUPLES, True, 1.0, 1, 0)
    exact = _exact(WORKED)
    assert exact[0] == (3 * P[1], 2 + 3 * P[1]) and exact[2] == exact[0] and exact[3] is None and int(look["candidates"][0]) == 7
    assert look["terms"][0, 0].tolist() == [0.0] * 2 + [0.0, 3 * float(P[1])] * 3 + [0.0] * 24
    for a in range(3):                                                     # (down moves nothing)
        assert look["E"][0, a] == float(exact[a][0]) and look["q"][0, a] == float(exact[a][1]), a
    assert look["rewards"][0].tolist() == [2, 0, 2, 0] and exact[1][0] > 1 and look["q"][0, 3] == 0.0 and look["E"][0, 3] == 0.0
    # other boards, and a value that is not zero: V = 1/4 per tile of the board, exact in both forms
    rng = np.random.default_rng(8)
    w4 = np.zeros(16 ** 4, dtype=np.float32)
    idx = np.arange(16 ** 4)
    w4[:] = sum(((idx >> (4 * i)) & 15) > 0 for i in range(4)) * 0.25      # the tuple (0, 1, 2, 3) alone, no symmetry: tiles in row 0
    for _ in range(20):
        cells = (rng.integers(1, 6, 16) * (rng.random(16) < .6)).tolist()
        key = key_of(cells)
        for weights, tuples, value in ((_zero(), TUPLES, lambda b: Fraction(0)), (w4, ((0, 1, 2, 3),), lambda b: Fraction(sum(v > 0 for v in b[:4]), 4))):
            look, exact = nt.search_nt_on_host([key], weights, tuples, False, .5, 1, 0), _exact(key, value, Fraction(1, 2))
            for a in range(4):
                # (E rounds once, in the division; q rounds twice more, so it is held to the float64 E)
                want = (0.0, 0.0) if exact[a] is None else (float(exact[a][0]), float(look["rewards"][0, a]) + .5 * float(exact[a][0]))
                assert exact[a] is None or abs(want[1] - float(exact[a][1])) <= 2 ** -49
                assert (look["E"][0, a], look["q"][0, a]) == want and bool(look["candidates"][0] >> a & 1) == (exact[a] is not None), (cells, a)


def test_a_dead_board_and_a_full_board_with_one_merge():
    nt = _nt()
    look = nt.search_nt_on_host([DEAD, ONE_MERGE], _zero(), TUPLES, True, 1.0, 1, 0)
    assert look["action"].tolist()[0] == -1 and look["candidates"].tolist() == [0, 0b0101] and not look["q"][0].any() and not look["terms"][0].any()
    # left: 4 2 16 . in the last row, cell 15 under a 4: a 2-tile ends the game (m = 0.0), a 4-tile merges upwards (reward 3).  right:
    # . 4 2 16 brings a 4 under a 4 and a 2 under a 2 as well: the chance boards of cell 12 have merges whatever the tile (by _exact).
    exact = _exact(ONE_MERGE)
    assert exact[0] == (3 * P[1], 4 + 3 * P[1]) and exact[2][0] > 3 and exact[1] is None and exact[3] is None
    assert look["terms"][1, 0, 30:].tolist() == [0.0, 3 * float(P[1])] and not look["terms"][1, 0, :30].any() and look["terms"][1, 2, 24:26].all()
    over = key_of([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 4, 1])          # the chance board of slot 30
    assert int(nt.search_nt_on_host([over], _zero(), TUPLES, True, 1.0, 1, 0)["candidates"][0]) == 0
    for a in (0, 2):
        assert look["E"][1, a] == float(exact[a][0]) and look["q"][1, a] == float(exact[a][1])
    assert look["q"][1, 1] == 0.0 and look["q"][1, 3] == 0.0 and int(look["action"][1]) == 2


def test_q_is_the_same_on_the_eight_images():
    """weights that are multiples of 2^-4 below 2^6: V, the terms (multiples of 2^-28 below 2^12) and S are exact, so the order of the
    cells does not enter and q of T_j(B) is q of B with the moves mapped, to the bit"""
    nt = _nt()
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import ACTION_MAP, transforms_on_host
    rng = np.random.default_rng(12)
    w = (rng.integers(-2 ** 10, 2 ** 10, nt.tuple_offsets(TUPLES)[1]) / 16.0).astype(np.float32)
    nib = (rng.integers(1, 8, (60, 16)) * (rng.random((60, 16)) < .65)).astype(np.uint64)
    pack = lambda cells: (cells << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    q = nt.search_nt_on_host(pack(nib), w, TUPLES, True, 1.0, 1, 0)["q"]
    assert len(set(q.ravel().tolist())) > 150
    for j, src in enumerate(transforms_on_host(4)):
        image = nt.search_nt_on_host(pack(nib[:, src]), w, TUPLES, True, 1.0, 1, 0)["q"]
        assert np.array_equal(bits(image[:, list(ACTION_MAP[j])]), bits(q)), j
    plain = nt.search_nt_on_host(pack(nib[:, transforms_on_host(4)[1]]), w, TUPLES, False, 1.0, 1, 0)["q"]
    assert not np.array_equal(plain[:, list(ACTION_MAP[1])], nt.search_nt_on_host(pack(nib), w, TUPLES, False, 1.0, 1, 0)["q"])


def test_the_sum_is_the_tree():
    """E * n_empty = S is the xor butterfly's sum, slot s with s ^ 1, then s ^ 2, ... s ^ 16 -- not the sum from left to right, which
    rounds otherwise on weights that are not round numbers"""
    nt = _nt()
    rng = np.random.default_rng(33)
    w = (rng.standard_normal(nt.tuple_offsets(TUPLES)[1]) * 3).astype(np.float32)
    nib = (rng.integers(1, 8, (200, 16)) * (rng.random((200, 16)) < .4)).astype(np.uint64)
    keys = (nib << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    look = nt.search_nt_on_host(keys, w, TUPLES, True, 1.0, 1, 0)
    lanes = look["terms"].copy()
    for d in (1, 2, 4, 8, 16):
        lanes = lanes + lanes[..., np.arange(32) ^ d]
    assert all(np.array_equal(bits(lanes[..., s]), bits(lanes[..., 0])) for s in range(32))          # the sum, in every lane
    left_to_right = np.zeros(lanes.shape[:2])
    for s in range(32):
        left_to_right = left_to_right + look["terms"][..., s]
    cand = (look["candidates"][:, None] >> np.arange(4) & 1).astype(bool)
    n_empty = ((look["after"][:, :, None] >> (np.uint64(4) * np.arange(16, dtype=np.uint64))) & np.uint64(15) == 0).sum(axis=2)
    assert np.array_equal(bits(look["E"][cand]), bits((lanes[..., 0] / np.maximum(n_empty, 1))[cand]))
    differ = cand & (bits(lanes[..., 0]) != bits(left_to_right))
    assert differ.sum() > 20 and np.allclose(lanes[..., 0], left_to_right, rtol=1e-13, atol=0)
    assert (bits(look["E"]) != bits(left_to_right / np.maximum(n_empty, 1)))[differ].any()


# ------------------------------------------------------------------ what the compiler made
def test_search_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_search.hip with the Makefile's flags: twelve kernels, this file's four at 32 lanes among
    them, none with scratch or a spilled vector register.  VGPRs as built: search 138 (symmetric) / 112, games 152 / 97."""
    assert_no_scratch("ntuple-search-resource-usage", SEARCH_UNIT, 256)
