"""The 2048 n-tuple network's temporal-coherence step sizes without a GPU: the library's two entry points and
their refusals, the host's statement of the learner with its third accumulator and of the apply launch
(pulselib_amd/agents/tfe_ntuple_td_gpu.py: learn_tc_nt_on_host, apply_tc_nt_on_host) on two hand-worked rounds, the first apply against
apply_nt_on_host, the checkpoint's version 4, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

from tests.native_args import assert_refusals, remarks
from tests.tfe_nt_support import BATCH, CASES, NET_CASES, RHO, ROOT, STEP_SIZE, V, X, Y, assert_exports, assert_no_scratch, bits, opts, tc_worked, tc_worked_state
from tests.tfe_nt_support import nt as _nt

LEARN, APPLY = "pulse_tfe_nt_learn_tc", "pulse_tfe_nt_apply_tc"


# ------------------------------------------------------------------ the export
def test_library_exports_the_two_entry_points():
    from pulselib_amd import _native
    names = ((LEARN, "PulseTfeNtLearnTc"), (APPLY, "PulseTfeNtApplyTc"))
    lib, text = assert_exports(names, [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    for name, struct in names:
        assert re.search(r"typedef struct %s \{" % struct, text)
    s = _native.TfeNtLearnTc
    assert C.sizeof(s) == 200
    assert [f[0] for f in s._fields_] == ["net", "n_games", "max_steps", "gamma", "lam", "keys", "values", "steps", "lengths", "deltas", "acc", "acc_abs",
                                          "stats", "reserved0"]
    assert (s.n_games.offset, s.max_steps.offset, s.gamma.offset, s.lam.offset, s.keys.offset, s.values.offset, s.steps.offset, s.lengths.offset,
            s.deltas.offset, s.acc.offset, s.acc_abs.offset, s.stats.offset, s.reserved0.offset) == (104, 108, 112, 120, 128, 136, 144, 152, 160, 168, 176,
                                                                                                     184, 192)
    lam = _native.TfeNtLearnLambda                                         # PulseTfeNtLearnLambda's fields, in its order, plus acc_abs
    assert [f[0] for f in s._fields_ if f[0] != "acc_abs"] == [f[0] for f in lam._fields_]
    s = _native.TfeNtApplyTc
    assert C.sizeof(s) == 160 and [f[0] for f in s._fields_] == ["net", "step", "acc", "acc_abs", "e", "a", "tc_stats", "reserved0"]
    assert (s.step.offset, s.acc.offset, s.acc_abs.offset, s.e.offset, s.a.offset, s.tc_stats.offset, s.reserved0.offset) == (104, 112, 120, 128, 136, 144, 152)
    unit = (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_tc.hip").read_text()
    assert "static_assert(sizeof(PulseTfeNtLearnTc) == 200 && sizeof(PulseTfeNtApplyTc) == 160" in unit
    assert [C.sizeof(x) for x in (_native.TfeNtNet, _native.TfeNtRollout, _native.TfeNtLearn, _native.TfeNtLearnLambda, _native.TfeNtApply, _native.TfeNtEval)] == \
        [104, 232, 176, 192, 128, 208]                                     # the old structs are as they were
    assert lib.pulse_version() == 1


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
def test_argument_checks_without_gpu():
    """every refusal of pulse_tfe_nt_learn_lambda under the new name and the four of its own (acc_abs null, misaligned; lambda > 0
    without deltas, twice), and every refusal of pulse_tfe_nt_apply and the eight of its own, before anything is launched (there is no
    device here to launch on)"""
    from pulselib_amd import _native
    lib = _native.lib()
    _learn_opts, _apply_opts = functools.partial(opts, _native.TfeNtLearnTc), functools.partial(opts, _native.TfeNtApplyTc)
    assert len(assert_refusals(lib, LEARN, _learn_opts, CASES[LEARN])) == len(NET_CASES) + len(BATCH) + 3 + 5 + 4 + 1 + 1 + 2 + 4
    assert len(assert_refusals(lib, APPLY, _apply_opts, CASES[APPLY])) == len(NET_CASES) + 2 + 4 + 2 + 8 + 1
    o = _learn_opts(net_weights=None, n_games=0)                            # the learner reads no weight
    assert getattr(lib, LEARN)(C.byref(o), None) == -1 and b"n_games must be positive" in lib.pulse_last_error()
    # lambda == 0 with deltas null is the TD(0) form: it passes that check, and the next one refuses
    o = _learn_opts(lam=0.0, deltas=None, lengths=2)
    assert getattr(lib, LEARN)(C.byref(o), None) == -1 and b"lengths must be 4-byte aligned" in lib.pulse_last_error()
    for lam in (0.0, 1.0):                                                 # the ends of the interval are inside
        assert getattr(lib, LEARN)(C.byref(_learn_opts(lam=lam, keys=None)), None) == -1 and b"keys is null" in lib.pulse_last_error()


def test_python_layer():
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    nt = _nt()
    from tests.tfe_nt_support import assert_init_parameters
    p = assert_init_parameters(NTupleTDAfterstateTFEGPU)
    assert p["tc"].default is False and p["lam"].default == 0.0
    for name in ("learn_tc_launch", "apply_tc_launch", "coherence", "tc_summary", "clear", "learn_lambda_launch"):
        assert callable(getattr(NTupleTDAfterstateTFEGPU, name)), name
    for name in ("learn_tc_nt_on_host", "apply_tc_nt_on_host", "tc_summary_on_host", "coherence_of_checkpoint"):
        assert callable(getattr(nt, name)), name
    assert list(inspect.signature(nt.apply_tc_nt_on_host).parameters) == ["weights", "acc", "acc_abs", "E", "A", "step"]
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        NTupleTDAfterstateTFEGPU(torch.device("cpu"), 64, tc=True)
    assert nt.tc_summary_on_host([4, 3 << 32, 0, 0]) == dict(moved=4, mean_rho=0.75) and nt.tc_summary_on_host([0, 0, 0, 0]) == dict(moved=0, mean_rho=1.0)


# ------------------------------------------------------------------ the hand-worked case: two rounds
def test_two_hand_worked_rounds():
    nt = _nt()
    tuples = ((0, 3),)
    assert nt.feature_indices_on_host([X, Y, V], tuples, True).tolist() == [[1, 0, 0, 16, 1, 0, 0, 16], [34] * 8, [1, 48, 3, 16, 1, 48, 3, 16]]
    assert 0.0 < RHO < 1.0 and RHO == 11.0 / 32787.0
    w, E, A = np.zeros(256, dtype=np.float32), np.zeros(256), np.zeros(256)
    acc, ab = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    for r, (games, want) in enumerate(zip(tc_worked(), tc_worked_state())):
        want_acc, want_ab, want_st, want_w, want_E, want_A, want_tc = want
        assert nt.learn_tc_nt_on_host(*games, tuples, True, 1.0, 0.0, acc, ab) == want_st, r
        assert np.array_equal(acc, want_acc) and np.array_equal(ab, want_ab), r
        assert nt.apply_tc_nt_on_host(w, acc, ab, E, A, STEP_SIZE) == want_tc, r
        assert not acc.any() and not ab.any(), r
        assert np.array_equal(w.view(np.uint32), want_w.view(np.uint32)), r
        assert np.array_equal(bits(E), bits(want_E)) and np.array_equal(bits(A), bits(want_A)), r
    assert w[1] < np.float32(0.171875) and w[1] > np.float32(0.171875 - 0.25)      # the turned sign moved it by less than the full step
    # the lambda form of round 1: the same four clamped integers (D_0 = 9,993 and D_1 = -19,996 clamp as the one-step ones do)
    acc2, ab2 = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    st = nt.learn_tc_nt_on_host(*tc_worked()[0], tuples, True, 1.0, 0.5, acc2, ab2)
    assert st["deltas"][:, 0].tolist() == [9993.0, -19996.0, -2.0] and {k: st[k] for k in ("learnt", "skipped", "clamped")} == dict(learnt=5, skipped=1, clamped=2)
    assert np.array_equal(acc2, tc_worked_state()[0][0]) and np.array_equal(ab2, tc_worked_state()[0][1])
    # acc is the other learners' whatever acc_abs: the third accumulator only adds
    acc3 = np.zeros((256, 2), dtype=np.int64)
    nt.learn_nt_on_host(*tc_worked()[0], tuples, True, 1.0, acc3)
    assert np.array_equal(acc3, acc2)


def test_first_apply_is_the_fixed_step():
    """on zero E and A rho is 1.0 exactly: the weights of apply_nt_on_host, as float32 bit patterns, on accumulators with means that
    round (sum / cnt with cnt 3, 7, ...), a negative zero and a subnormal weight among them"""
    nt = _nt()
    rng = np.random.default_rng(8)
    W = 4096
    acc = np.zeros((W, 2), dtype=np.int64)
    at = rng.choice(W, 1500, replace=False)
    acc[at, 1] = rng.integers(1, 50, 1500)
    acc[at, 0] = rng.integers(-2 ** 40, 2 ** 40, 1500)
    ab = np.zeros(W, dtype=np.int64)
    ab[at] = np.abs(acc[at, 0]) + rng.integers(0, 2 ** 40, 1500)
    w = (rng.standard_normal(W) * 100).astype(np.float32)
    w[at[0]], w[at[1]] = np.float32(-0.0), np.float32(1e-42)
    for step in (1.0 / 32, 1.0, 0.3):
        w0, w1, acc0, acc1, ab1, E, A = w.copy(), w.copy(), acc.copy(), acc.copy(), ab.copy(), np.zeros(W), np.zeros(W)
        moved = nt.apply_nt_on_host(w0, acc0, step)
        assert nt.apply_tc_nt_on_host(w1, acc1, ab1, E, A, step) == (moved, moved << 32) and moved == 1500
        assert np.array_equal(w0.view(np.uint32), w1.view(np.uint32)) and not acc1.any() and not ab1.any()
        assert np.array_equal(E[at], acc[at, 0] / acc[at, 1] * 2.0 ** -16) and np.array_equal(A[at], ab[at] / acc[at, 1] * 2.0 ** -16)
        rest = np.ones(W, dtype=bool)
        rest[at] = False
        assert not E[rest].any() and not A[rest].any() and (np.abs(E) <= A).all()


# ------------------------------------------------------------------ the checkpoint
def test_checkpoint_version_4(tmp_path):
    nt = _nt()
    tuples = ((0, 1, 2, 3), (15,))
    n = nt.tuple_offsets(tuples)[1]
    w, E, A = np.zeros(n, dtype=np.float32), np.zeros(n), np.zeros(n)
    w[[3, 700, 65551]] = (1.5, -2.0, 0.25)
    E[[3, 9, 65551]], A[[3, 700, 65551]] = (-0.5, -0.0, 2.0), (0.75, 1e-300, 2.0)      # E alone (a negative zero), A alone, both
    scalars = dict(symmetric=1, gamma=1.0, epsilon=0.25, alpha=0.5, max_steps=256, seed=9, board_id0=1, round=7, n_games=257)
    today = sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS)
    for lam in (0.0, 0.5):                                                 # lam is always there, 0 included
        path = tmp_path / f"tc{lam}.npz"
        nt.write_checkpoint(path, w, tuples, lam=lam, tc=(E, A), **scalars)
        with np.load(path, allow_pickle=False) as raw:
            assert sorted(raw.files) == sorted(today + ["lam", "tc_index", "tc_e", "tc_a"]) and int(raw["version"]) == 4 == nt.CHECKPOINT_VERSION_TC
            assert raw["tc_index"].dtype == np.int64 and raw["tc_index"].tolist() == [3, 9, 700, 65551]
            assert raw["tc_e"].dtype == raw["tc_a"].dtype == np.float64 and float(raw["lam"]) == lam
        f = nt.read_checkpoint(path)
        assert f["tc"] is True and f["lam"] == lam and {k: f[k] for k in scalars} == {**scalars, "symmetric": True}
        assert np.array_equal(nt.weights_of_checkpoint(f).view(np.uint32), w.view(np.uint32))
        E2, A2 = nt.coherence_of_checkpoint(f)
        assert np.array_equal(bits(E2), bits(E)) and np.array_equal(bits(A2), bits(A))
    # without tc: today's files, byte for byte (versions 1 and 2), and read back with tc False
    for lam, version in ((0.0, 1), (0.5, 2)):
        nt.write_checkpoint(tmp_path / "a.npz", w, tuples, lam=lam, **scalars)
        nt.write_checkpoint(tmp_path / "b.npz", w, tuples, lam=lam, tc=None, **scalars)
        cells = np.full((2, 6), -1, dtype=np.int64)
        cells[0, :4], cells[1, :1] = (0, 1, 2, 3), (15,)
        dtypes = dict(gamma=np.float64, epsilon=np.float64, alpha=np.float64, seed=np.uint64, board_id0=np.uint64)
        arrays = {k: np.array(scalars[k], dtype=dtypes.get(k, np.int64)) for k in nt.CHECKPOINT_SCALARS}
        if lam:
            arrays["lam"] = np.array(lam, dtype=np.float64)
        with open(tmp_path / "c.npz", "wb") as fh:                         # what write_checkpoint wrote before there was a `tc`
            np.savez(fh, version=np.array(version, dtype=np.int64), index=np.array([3, 700, 65551], dtype=np.int64), value=w[[3, 700, 65551]],
                     tuple_len=np.array([4, 1], dtype=np.int64), tuple_cells=cells, **arrays)
        assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes() == (tmp_path / "c.npz").read_bytes()
        f = nt.read_checkpoint(tmp_path / "a.npz")
        assert f["tc"] is False and f["lam"] == lam and "tc_index" not in f
    # refusals
    with np.load(tmp_path / "tc0.5.npz", allow_pickle=False) as raw:
        arrays = {k: raw[k] for k in raw.files}

    def refused(match, **change):
        new = {k: v for k, v in {**arrays, **change}.items() if v is not None}
        with open(tmp_path / "bad.npz", "wb") as fh:
            np.savez(fh, **new)
        with pytest.raises(ValueError, match=match):
            nt.read_checkpoint(tmp_path / "bad.npz")

    refused("format version 3", version=np.array(3, dtype=np.int64))
    refused("format version 5", version=np.array(5, dtype=np.int64))
    refused(r"not an n-tuple network checkpoint \(no \['tc_e'\]\)", tc_e=None)
    refused(r"no \['lam'\]", lam=None)
    refused("tc_index must be strictly ascending", tc_index=np.array([3, 9, 9, 65551], dtype=np.int64))
    refused("tc_index must be strictly ascending", tc_index=np.array([9, 3, 700, 65551], dtype=np.int64))
    refused("tc_index must be strictly ascending", tc_index=np.array([3, 9, 700, n], dtype=np.int64))
    refused("tc_index must be strictly ascending", tc_index=np.array([-1, 9, 700, 65551], dtype=np.int64))
    refused("tc_index must be int64", tc_a=arrays["tc_a"][:3])
    refused("tc_index must be int64", tc_e=arrays["tc_e"].astype(np.float32))
    with pytest.raises(ValueError, match="one float64 per weight"):
        nt.write_checkpoint(tmp_path / "bad.npz", w, tuples, tc=(E[:5], A), **scalars)


# ------------------------------------------------------------------ what the compiler made
def test_tc_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_tc.hip with the Makefile's flags: five kernels -- the scatter text's four forms with
    the third accumulator and the apply -- none with scratch or a spilled vector register.  VGPRs as built: scatter 59 / 20, apply 41."""
    names = assert_no_scratch("ntuple-tc-resource-usage", {"tfe_nt_scatter_kernel": 4, "tfe_nt_tc_apply_kernel": 1}, 128)
    assert all("Lb1ENS_5NtDevEEE" in n for n in names if "tfe_nt_scatter_kernel" in n)  # every one of the four has Abs = true
    sgpr_spills = re.findall(r"SGPRs Spill: (\d+)", remarks("ntuple-tc-resource-usage"))
    assert sgpr_spills == ["0"] * 5
