"""The 2048 n-tuple network without a GPU: the library's exports and argument checks, the host's statement of
the features, the value, the learner and the apply launch (pulselib_amd/agents/tfe_ntuple_td_gpu.py), that the host mirror learns, the
checkpoint file, and what the compiler made of the kernels."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.native_args import assert_refusals
from tests.tfe_nt_support import CASES, assert_exports, assert_no_scratch, play_kernels, opts, worked_games

NAMES = ("pulse_tfe_nt_rollout", "pulse_tfe_nt_learn", "pulse_tfe_nt_apply", "pulse_tfe_nt_evaluate")
STRUCTS = dict(zip(NAMES, ("TfeNtRollout", "TfeNtLearn", "TfeNtApply", "TfeNtEval")))


def test_library_exports_the_four_entry_points():
    from pulselib_amd import _native
    _, text = assert_exports([(name, "Pulse" + STRUCTS[name]) for name in NAMES], [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    assert [C.sizeof(s) for s in (_native.TfeNtNet, _native.TfeNtRollout, _native.TfeNtLearn, _native.TfeNtApply, _native.TfeNtEval)] == \
        [104, 232, 176, 128, 208]                                          # the static_assert of csrc/tfe_ntuple.hip
    for macro, value in (("MAX_TUPLES", 8), ("MAX_LEN", 6), ("FRAC_BITS", 16)):
        assert re.search(r"#define PULSE_TFE_NT_%s\s+%d\b" % (macro, value), text) and getattr(_native, "TFE_NT_" + macro) == value
    assert re.search(r"#define PULSE_TFE_NT_DELTA_MAX\s+8192\.0", text) and _native.TFE_NT_DELTA_MAX == 8192.0


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_without_gpu(name):
    """every refusal comes back as PULSE_EINVAL with its message under the entry point's name; a refusal returns before the row table
    is asked for or anything is launched (there is no device here to ask)"""
    from pulselib_amd import _native
    lib = _native.lib()
    struct = getattr(_native, STRUCTS[name])
    assert_refusals(lib, name, lambda **kw: opts(struct, **kw), CASES[name])
    if name == "pulse_tfe_nt_learn":                                       # the learner reads no weight
        o = opts(struct, net_weights=None, n_games=0)
        assert getattr(lib, name)(C.byref(o), None) == -1 and b"n_games must be positive" in lib.pulse_last_error()


def test_python_layer_refuses():
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        NTupleTDAfterstateTFEGPU(torch.device("cpu"), 64)
    for bad in ([], [[0]] * 9, [[0, 1, 2, 3, 4, 5, 6]], [[]], [[0, 16]], [[3, 3]]):
        with pytest.raises(ValueError):
            nt.check_tuples(bad)
    assert nt.check_tuples([[0, 1], (2,)]) == ((0, 1), (2,)) and nt.tuple_offsets(nt.DEFAULT_TUPLES) == ([0, 65536, 131072, 131072 + 16 ** 6], 33685504)


# ------------------------------------------------------------------ features and the value
def test_image_cells_are_the_eight_transforms():
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import transforms_on_host
    tf = transforms_on_host(4)
    (cells,) = nt.feature_cells_on_host([tuple(range(16))[:6]], True)
    assert cells.shape == (8, 6) and np.array_equal(cells, tf[:, :6])
    for t, cells in zip(nt.DEFAULT_TUPLES, nt.feature_cells_on_host(nt.DEFAULT_TUPLES, True)):
        assert np.array_equal(cells, np.array([[tf[j][c] for c in t] for j in range(8)]))
        assert len({tuple(row) for row in cells.tolist()}) == 8               # eight different readings of a row or a rectangle
    (plain,) = nt.feature_cells_on_host([(4, 5, 6, 8, 9, 10)], False)
    assert plain.tolist() == [[4, 5, 6, 8, 9, 10]]
    # the index reads the board's image: feature (t, j) of a board is feature (t, 0) of T_j(board)
    rng = np.random.default_rng(3)
    nib = rng.integers(0, 16, (50, 16)).astype(np.uint64)
    pack = lambda cells: (cells << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    all8 = nt.feature_indices_on_host(pack(nib), nt.DEFAULT_TUPLES, True)
    assert all8.shape == (50, 32) and all8.max() < 33685504
    for j in range(8):
        assert np.array_equal(nt.feature_indices_on_host(pack(nib[:, tf[j]]), nt.DEFAULT_TUPLES, False), all8[:, j::8])
    assert int(nt.feature_indices_on_host([0x0000000000004321], [(0, 1, 2, 3)], False)[0, 0]) == 0x4321


def test_value_is_the_same_on_the_eight_images():
    """weights that are multiples of 2^-10 below 2^10 in magnitude: every partial sum is exact, so the order of the images does not
    enter and the eight values agree to the bit"""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import transforms_on_host
    tuples = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (5, 6, 9))
    rng = np.random.default_rng(11)
    w = (rng.integers(-2 ** 20, 2 ** 20, nt.tuple_offsets(tuples)[1]) / 1024.0).astype(np.float32)
    nib = rng.integers(0, 12, (200, 16)).astype(np.uint64)
    pack = lambda cells: (cells << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    v = nt.value_on_host(pack(nib), w, tuples, True)
    assert v.dtype == np.float64 and len(set(v.tolist())) == 200
    for src in transforms_on_host(4):
        assert np.array_equal(nt.value_on_host(pack(nib[:, src]), w, tuples, True), v)
    assert not np.array_equal(nt.value_on_host(pack(nib[:, transforms_on_host(4)[1]]), w, tuples, False), nt.value_on_host(pack(nib), w, tuples, False))


def test_host_philox_and_moves_are_the_oracles():
    from oracle import oracle as orc
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    from tests.tfe_host import move_on_host, pack_boards
    for seed, subseq, offset in ((1, 2, 3), (2 ** 63 + 5, 2 ** 64 - 1, 77), (0x2048AC7105EED, 12345678901234, 0)):
        assert nt.philox_many_on_host(seed, [subseq], offset)[0].tolist() == [int(x) for x in orc.philox4x32(seed, subseq, offset)]
    rng = np.random.default_rng(5)
    boards = ((1 << rng.integers(1, 12, (120, 4, 4))) * (rng.random((120, 4, 4)) < .6)).astype(np.int32)
    after, scores = nt.moves_on_host(pack_boards(boards))
    checked = 0
    for g, board in enumerate(boards):
        for a in range(4):
            moved, score, spawned = move_on_host(board, a)                 # the oracle's step, with its spawn undone where it can be
            assert score == int(scores[g, a])
            if not spawned:
                assert int(pack_boards(moved[None])[0]) == int(after[g, a]), (g, a)
                checked += 1
    assert checked > 400
    assert nt.rewards_of_scores([0, 4, 12, 65536 + 4]).tolist() == [0, 2, 3, 16]


# ------------------------------------------------------------------ the learner and the apply launch on a hand-worked case
def test_learn_and_apply_on_a_hand_worked_case():
    """One tuple of the cells (0, 3), symmetric: the images read the corner pairs (0,3) (3,15) (15,12) (12,0) and, transposed,
    (0,12) (12,15) (15,3) (3,0).  Board X = a 2 in cell 0 (nibble 1), nothing else.  Reading (first, second) nibbles, index = first +
    16 * second: (1,0) -> 1, (0,0) -> 0, (0,0) -> 0, (0,1) -> 16, (1,0) -> 1, (0,0) -> 0, (0,0) -> 0, (0,1) -> 16: images share weights.
    Game 0 (length 3, ends): values 10, 20000, 2; rewards 0, 1, 3; terminal at t = 2.
      t = 0: target 1 + 20000, delta 19991 clamps to 8192, d = 8192 * 65536;  t = 1: target 3 + 2 = 5, delta -19995 clamps to -8192;
      t = 2: terminal, target 0, delta -2, d = -131072.
    Game 1 (length 2, cut): values 1.5, 7; rewards 2, 2: t = 0: target 2 + 7, delta 7.5, d = 491520; t = 1: the last move of a cut game,
      skipped.  All five moves record board X, so per learnt move index 0 gets 4 adds, 1 and 16 two each."""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    tuples, X = ((0, 3),), 0x1
    assert nt.feature_cells_on_host(tuples, True)[0].tolist() == [[0, 3], [3, 15], [15, 12], [12, 0], [0, 12], [12, 15], [15, 3], [3, 0]]
    assert nt.feature_indices_on_host([X], tuples, True)[0].tolist() == [1, 0, 0, 16, 1, 0, 0, 16]
    keys, values, steps, lengths = worked_games()
    assert (keys == X).all() and lengths == [3, 2]
    acc = np.zeros((256, 2), dtype=np.int64)
    st = nt.learn_nt_on_host(keys, values, steps, lengths, tuples, True, 1.0, acc)
    assert st == dict(learnt=4, skipped=1, clamped=2)
    total = 8192 * 65536 - 8192 * 65536 - 131072 + 491520
    want = np.zeros((256, 2), dtype=np.int64)
    want[0], want[1], want[16] = (4 * total, 16), (2 * total, 8), (2 * total, 8)
    assert np.array_equal(acc, want)
    # gamma enters the target: .5 * 7 + 2 - 1.5 = 4 for game 1's first move alone
    acc2 = np.zeros((256, 2), dtype=np.int64)
    assert nt.learn_nt_on_host(keys[:, 1:], values[:, 1:], steps[:, 1:], [2], tuples, True, .5, acc2) == dict(learnt=1, skipped=1, clamped=0)
    assert acc2[0].tolist() == [4 * 4 * 65536, 4] and acc2[1].tolist() == [2 * 4 * 65536, 2]
    # apply: the mean of the four moves' differences is total / 4 * 2^-16 = 1.375, step 1 / 8; a weight with cnt = 0 keeps its bits
    w = np.zeros(256, dtype=np.float32)
    w[0], w[1], w[5] = 1.0, np.float32(0.1), np.float32(-0.0)
    before = w.copy()
    assert nt.apply_nt_on_host(w, acc, 0.125) == 3 and not acc.any()
    assert w[0] == np.float32(1.0 + 0.125 * 1.375) and w[16] == np.float32(0.171875)
    assert w[1].view(np.uint32) == np.float32(np.float64(np.float32(0.1)) + 0.171875).view(np.uint32)
    keep = np.ones(256, dtype=bool)
    keep[[0, 1, 16]] = False
    assert np.array_equal(w.view(np.uint32)[keep], before.view(np.uint32)[keep]) and w.view(np.uint32)[5] == 0x80000000
    # the mean rounds once in the division: sum 1, cnt 3
    acc[7] = (1, 3)
    nt.apply_nt_on_host(w, acc, 1.0)
    assert w[7] == np.float32(1.0 / 3.0 * 2.0 ** -16)


# ------------------------------------------------------------------ games on the host
def _round(weights, tuples, r, n_games=256, epsilon=0.0, max_steps=4096, seed=0, **kw):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_host import nt_games_on_host
    return nt_games_on_host(n_games, max_steps, epsilon, 1.0, weights, tuples, True, seed, seed ^ AGENT_KEY, seed ^ TIE_KEY, r * n_games, r, **kw)


def test_the_host_mirror_learns():
    """256 games per round, the default network, alpha 1, epsilon 0, gamma 1: the mean final score of round 1 (one round's update)
    beats round 0's (zero weights: greedy on the reward) by at least five standard errors of the difference.  Measured: 1,898 +- 60
    against 4,426 +- 140."""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    tuples = nt.DEFAULT_TUPLES
    w = np.zeros(nt.tuple_offsets(tuples)[1], dtype=np.float32)
    acc = np.zeros((len(w), 2), dtype=np.int64)
    scores = []
    for r in range(2):
        out = _round(w, tuples, r)
        scores.append(out["total_score"].astype(np.float64))
        if r == 0:
            st = nt.learn_nt_on_host(out["keys"], out["values"], out["steps"], out["lengths"], tuples, True, 1.0, acc)
            assert out["truncated"] == 0 and st == dict(learnt=int(out["lengths"].sum()), skipped=0, clamped=0)
            assert int(acc[:, 1].sum()) == 32 * st["learnt"] and nt.apply_nt_on_host(w, acc, 1.0 / 32) > 10000 and not acc.any()
    mean, se = [s.mean() for s in scores], [s.std(ddof=1) / np.sqrt(s.size) for s in scores]
    print("mean final score per round", mean, "standard errors", se)
    assert 1500 < mean[0] < 2400
    assert mean[1] - mean[0] >= 5.0 * np.hypot(se[0], se[1]), (mean, se)


def test_the_tile_cap_cuts_a_game_on_the_host():
    """a board that merges two 16,384 tiles holds nibble 15: the game stops there, is not over, and counts as cut; its one move has no
    terminal bit, so the learner skips it"""
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    tuples = ((0, 1, 2, 3),)
    boards = np.zeros((2, 4, 4), dtype=np.int32)
    boards[0, 0, :2] = 16384
    boards[0, 3, 3] = 2
    boards[1, 0, :2] = 8192
    out = _round(np.zeros(65536, dtype=np.float32), tuples, 0, n_games=2, max_steps=8, boards0=boards)
    assert out["lengths"].tolist() == [1, 8] and out["capped"] == 1 and out["truncated"] == 2 and out["ended"] == 0
    assert int(out["steps"][0, 0]) >> 7 == 0 and (int(out["steps"][0, 0]) >> 2) & 31 == 15 and int(out["total_score"][0]) == 32768
    assert int(out["final_boards"][0].max()) == 32768 and (int(out["keys"][0, 0]) & 0xFFFF) in (0x000F, 0xF000)
    acc = np.zeros((65536, 2), dtype=np.int64)
    st = nt.learn_nt_on_host(out["keys"], out["values"], out["steps"], out["lengths"], tuples, True, 1.0, acc)
    assert st["skipped"] == 2 and st["learnt"] == 7


def test_checkpoint_round_trip(tmp_path):
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    tuples = ((0, 1, 2, 3), (4, 5, 6, 8, 9, 10), (15,))
    n = nt.tuple_offsets(tuples)[1]
    rng = np.random.default_rng(2)
    w = np.zeros(n, dtype=np.float32)
    at = rng.choice(n, 5000, replace=False)
    w[at] = rng.standard_normal(5000).astype(np.float32)
    w[at[0]], w[at[1]], w[n - 1] = np.float32(-0.0), np.float32(1e-42), np.float32(3.5)      # a negative zero, a subnormal, the last weight
    scalars = dict(symmetric=1, gamma=1.0, epsilon=0.25, alpha=0.5, max_steps=256, seed=2 ** 63 + 9, board_id0=2 ** 62 + 1, round=7, n_games=257)
    path = tmp_path / "net.npz"
    nt.write_checkpoint(path, w, tuples, **scalars)
    f = nt.read_checkpoint(path)
    assert np.array_equal(nt.weights_of_checkpoint(f).view(np.uint32), w.view(np.uint32)) and f["tuples"] == tuples and f["n_weights"] == n
    assert {k: f[k] for k in scalars} == {**scalars, "symmetric": True} and len(f["index"]) == 5001
    assert path.stat().st_size < 200000                                    # the non-zero weights only
    with np.load(path, allow_pickle=False) as raw:
        assert sorted(raw.files) == sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS)
    with pytest.raises(ValueError, match="exactly the scalars"):
        nt.write_checkpoint(path, w, tuples, **{**scalars, "extra": 1})
    np.savez(open(tmp_path / "bad.npz", "wb"), version=np.array(1))
    with pytest.raises(ValueError, match="not an n-tuple network checkpoint"):
        nt.read_checkpoint(tmp_path / "bad.npz")


# ------------------------------------------------------------------ what the compiler made
def test_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple.hip with the Makefile's flags: nine kernels, none with scratch or a spilled vector
    register.  VGPRs as built: games 118 (symmetric) / 63, scatter 59 / 18 (both learners'), apply 22."""
    assert_no_scratch("ntuple-resource-usage", {**play_kernels(1, True), **play_kernels(1, False), "tfe_nt_scatter_kernel": 4, "tfe_nt_apply_kernel": 1}, 128)
