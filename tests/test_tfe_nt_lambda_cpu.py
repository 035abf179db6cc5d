"""The 2048 n-tuple network's TD(lambda) learner without a GPU: the library's entry point and its refusals,
the host's statement of the lambda-differences and of the learner (pulselib_amd/agents/tfe_ntuple_td_gpu.py: lambda_deltas_on_host,
learn_lambda_nt_on_host) on hand-worked games, at lambda = 0 against learn_nt_on_host and at lambda = 1 against the Monte-Carlo
return, the checkpoint's two versions, and what the compiler made of the kernels."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from tests.native_args import assert_refusals
from tests.tfe_nt_support import BATCH, CASES, NET_CASES, ROOT, assert_exports, assert_no_scratch, bits, opts, worked_games
from tests.tfe_nt_support import nt as _nt

NAME = "pulse_tfe_nt_learn_lambda"


# ------------------------------------------------------------------ C1: the export
def test_library_exports_the_entry_point():
    from pulselib_amd import _native
    _, text = assert_exports([(NAME, "PulseTfeNtLearnLambda")], [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    assert re.search(r"typedef struct PulseTfeNtLearnLambda \{", text) and re.search(r"double gamma, lambda;", text)
    s = _native.TfeNtLearnLambda
    assert C.sizeof(s) == 192
    assert [f[0] for f in s._fields_] == ["net", "n_games", "max_steps", "gamma", "lam", "keys", "values", "steps", "lengths", "deltas", "acc", "stats",
                                          "reserved0"]
    assert (s.n_games.offset, s.gamma.offset, s.lam.offset, s.keys.offset, s.deltas.offset, s.reserved0.offset) == (104, 112, 120, 128, 160, 184)
    assert "static_assert(sizeof(PulseTfeNtLearnLambda) == 192" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_lambda.hip").read_text()
    assert C.sizeof(_native.TfeNtLearn) == 176                            # the TD(0) learner's struct is as it was


# ------------------------------------------------------------------ C2: PULSE_EINVAL before anything is launched
def test_argument_checks_without_gpu():
    """every refusal of pulse_tfe_nt_learn and the three of its own (lambda, deltas null, deltas misaligned), under its own name,
    before anything is launched (there is no device here to launch on)"""
    from pulselib_amd import _native
    lib, make = _native.lib(), lambda **kw: opts(_native.TfeNtLearnLambda, **kw)
    errors = assert_refusals(lib, NAME, make, CASES[NAME])
    assert len(errors) == len(NET_CASES) + len(BATCH) + 3 + 5 + 4 + 1 + 3
    o = make(net_weights=None, n_games=0)                                  # the learner reads no weight
    assert getattr(lib, NAME)(C.byref(o), None) == -1 and b"n_games must be positive" in lib.pulse_last_error()
    for lam in (0.0, 1.0):                                                 # the ends of the interval are inside: the next check refuses
        assert getattr(lib, NAME)(C.byref(make(lam=lam, keys=None)), None) == -1 and b"keys is null" in lib.pulse_last_error()


def test_python_layer_refuses():
    import inspect
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    nt = _nt()
    assert inspect.signature(NTupleTDAfterstateTFEGPU.__init__).parameters["lam"].default == 0.0
    for bad in (-0.1, 1.1, math.nan):
        with pytest.raises(ValueError, match="lam must be in"):
            nt.check_lam(bad)
        with pytest.raises(ValueError, match="lam must be in"):            # (refused before the device is asked for)
            NTupleTDAfterstateTFEGPU(torch.device("cpu"), 64, lam=bad)
    assert nt.check_lam(0) == 0.0 and nt.check_lam(1) == 1.0
    for name in ("learn_lambda_launch", "trajectory_deltas"):
        assert callable(getattr(NTupleTDAfterstateTFEGPU, name))


# ------------------------------------------------------------------ C3: the hand-worked case
def test_a_hand_worked_case():
    """gamma 1, lambda .5.  Game 0: D_2 = 0 - 2 = -2; D_1 = (3 + 2 - 20000) + .5 * (-2) = -19,996, which its add clamps to -8,192;
    D_0 = (1 + 20000 - 10) + .5 * (-19,996) = 9,993 -- from the UNCLAMPED D_1 (the clamped one would give 15,895) -- which clamps to
    8,192.  Game 1: its last move is skipped, D_1 = +0.0; D_0 = (2 + 7 - 1.5) + .5 * 0 = 7.5.  Every move records board X: index 0 gets
    4 adds per learnt move, 1 and 16 two each."""
    nt = _nt()
    keys, values, steps, lengths = worked_games()
    deltas = nt.lambda_deltas_on_host(values, steps, lengths, 1.0, 0.5)
    assert deltas.dtype == np.float64 and deltas.tolist() == [[9993.0, 7.5], [-19996.0, 0.0], [-2.0, 0.0]]
    assert bits(deltas)[1, 1] == 0 and bits(deltas)[2, 1] == 0            # +0.0: the skipped move, and the row beyond game 1's length
    acc = np.zeros((256, 2), dtype=np.int64)
    st = nt.learn_lambda_nt_on_host(keys, values, steps, lengths, ((0, 3),), True, 1.0, 0.5, acc)
    assert np.array_equal(bits(st.pop("deltas")), bits(deltas)) and st == dict(learnt=4, skipped=1, clamped=2)
    total = 8192 * 65536 - 8192 * 65536 - 2 * 65536 + 491520               # the four d
    want = np.zeros((256, 2), dtype=np.int64)
    want[0], want[1], want[16] = (4 * total, 16), (2 * total, 8), (2 * total, 8)
    assert np.array_equal(acc, want)
    # game 1 alone at gamma .9: gl = .9 * .5 is a rounded product, D_0 = (2 + .9 * 7 - 1.5) + gl * 0
    one = nt.lambda_deltas_on_host(values[:, 1:], steps[:, 1:], [2], 0.9, 0.5)
    assert bits(one)[:, 0].tolist() == bits([(2.0 + 0.9 * 7.0) - 1.5 + (0.9 * 0.5) * 0.0, 0.0, 0.0]).tolist()
    acc2 = np.zeros((256, 2), dtype=np.int64)
    st = nt.learn_lambda_nt_on_host(keys[:, 1:], values[:, 1:], steps[:, 1:], [2], ((0, 3),), True, 0.9, 0.5, acc2)
    d = int(np.rint(np.ldexp((2.0 + 0.9 * 7.0) - 1.5, 16)))
    assert (st["learnt"], st["skipped"], st["clamped"]) == (1, 1, 0) and acc2[0].tolist() == [4 * d, 4] and acc2[16].tolist() == [2 * d, 2]
    # ... and where the product's rounding shows: three moves of an ended game, D_1 = delta_1 + gl * D_2 with gl = fl(.9 * .5)
    v = np.array([[3.0], [5.0], [7.0]])
    s = np.array([[0], [1 << 2], [2 << 2 | 0x80]], dtype=np.uint8)
    got = nt.lambda_deltas_on_host(v, s, [3], 0.9, 0.5)[:, 0]
    gl = np.float64(0.9) * np.float64(0.5)
    d2 = 0.0 - 7.0
    d1 = ((2.0 + 0.9 * 7.0) - 5.0) + gl * d2
    d0 = ((1.0 + 0.9 * 5.0) - 3.0) + gl * d1
    assert bits(got).tolist() == bits([d0, d1, d2]).tolist()


def test_lengths_beyond_the_buffers_are_clamped():
    """a game whose length says more than the rows there are has the rows there are, and its last row is its last move"""
    nt = _nt()
    keys, values, steps, _ = worked_games()
    deltas = nt.lambda_deltas_on_host(values, steps, [9, 2], 1.0, 0.5)
    assert deltas.tolist() == [[9993.0, 7.5], [-19996.0, 0.0], [-2.0, 0.0]]


# ------------------------------------------------------------------ C4 and C5: the two ends of lambda
def _recorded_round():
    """64 games of 64 moves at epsilon .25 under random weights on a small network: games that end and games that are cut"""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_host import nt_games_on_host
    nt = _nt()
    tuples = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5))
    w = (np.random.default_rng(6).standard_normal(nt.tuple_offsets(tuples)[1]) * 4).astype(np.float32)
    out = nt_games_on_host(64, 64, 0.25, 1.0, w, tuples, True, 5, 5 ^ AGENT_KEY, 5 ^ TIE_KEY, 100, 0)
    return tuples, len(w), out


def test_lambda_zero_is_the_one_step_learner():
    nt = _nt()
    tuples, W, out = _recorded_round()
    assert out["ended"] >= 1 and out["truncated"] >= 8 and out["values"].any()
    args = (out["keys"], out["values"], out["steps"], out["lengths"], tuples, True)
    for gamma in (1.0, 0.9):
        acc0, acc1 = np.zeros((W, 2), dtype=np.int64), np.zeros((W, 2), dtype=np.int64)
        st0 = nt.learn_nt_on_host(*args, gamma, acc0)
        st1 = nt.learn_lambda_nt_on_host(*args, gamma, 0.0, acc1)
        deltas = st1.pop("deltas")
        assert st0 == st1 and st0["learnt"] > 1000 and np.array_equal(acc0, acc1) and acc0[:, 1].sum() == 24 * st0["learnt"]
        # the one-step differences, formed here as learn_nt_on_host forms them
        T, L = out["values"].shape[0], out["lengths"].astype(np.int64)
        t = np.arange(T)[:, None]
        nxt_r, nxt_v = np.zeros_like(out["values"]), np.zeros_like(out["values"])
        nxt_r[:-1], nxt_v[:-1] = ((out["steps"][1:] >> 2) & 31).astype(np.float64), out["values"][1:]
        one_step = np.where(t == L[None, :] - 1, 0.0, nxt_r + gamma * nxt_v) - out["values"]
        learn = (t < L[None, :]) & ~((t == L[None, :] - 1) & (out["steps"] >> 7 == 0))
        assert np.array_equal(bits(deltas)[learn], bits(one_step)[learn]) and not bits(deltas)[~learn].any()
    # ... and lambda enters: the same games at lambda .5 (gamma .9 still) leave other sums in the same cells
    acc2 = np.zeros((W, 2), dtype=np.int64)
    nt.learn_lambda_nt_on_host(*args, 0.9, 0.5, acc2)
    assert np.array_equal(acc2[:, 1], acc0[:, 1]) and not np.array_equal(acc2[:, 0], acc0[:, 0])


def test_lambda_one_is_the_return_minus_the_value():
    """gamma 1, lambda 1, an ended game, integer values: D_t = (the sum of the later rewards) - V_t exactly; a cut game's D_t = (the
    later rewards up to its last move) + V_{L-1} - V_t: the skipped move passes +0.0 down"""
    nt = _nt()
    rng = np.random.default_rng(4)
    T = 40
    values = rng.integers(-500, 500, (T, 3)).astype(np.float64)
    rewards = rng.integers(0, 17, (T, 3))
    lengths = np.array([T, 17, 9])
    steps = (rng.integers(0, 4, (T, 3)) | rewards << 2).astype(np.uint8)
    steps[T - 1, 0] |= 0x80
    steps[16, 1] |= 0x80                                                   # games 0 and 1 end, game 2 is cut
    deltas = nt.lambda_deltas_on_host(values, steps, lengths, 1.0, 1.0)
    for g, L in enumerate(lengths.tolist()):
        later = np.array([rewards[t + 1:L, g].sum() for t in range(L)], dtype=np.float64)
        want = later - values[:L, g] + (values[L - 1, g] if g == 2 else 0.0)
        if g == 2:
            want[L - 1] = 0.0
        assert deltas[:L, g].tolist() == want.tolist(), g
        assert not deltas[L:, g].any()


# ------------------------------------------------------------------ C6: the checkpoint
def test_checkpoint_versions(tmp_path):
    nt = _nt()
    tuples = ((0, 1, 2, 3), (15,))
    w = np.zeros(nt.tuple_offsets(tuples)[1], dtype=np.float32)
    w[[3, 700, 65551]] = (1.5, -2.0, 0.25)
    scalars = dict(symmetric=1, gamma=1.0, epsilon=0.25, alpha=0.5, max_steps=256, seed=9, board_id0=1, round=7, n_games=257)
    today = sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS)
    for lam, version, names in ((0.0, 1, today), (0.5, 2, sorted(today + ["lam"]))):
        path = tmp_path / f"net{version}.npz"
        nt.write_checkpoint(path, w, tuples, lam=lam, **scalars)
        with np.load(path, allow_pickle=False) as raw:
            assert sorted(raw.files) == names and int(raw["version"]) == version
            assert version == 1 or (raw["lam"].dtype == np.float64 and raw["lam"].shape == () and float(raw["lam"]) == lam)
        f = nt.read_checkpoint(path)
        assert f["lam"] == lam and {k: f[k] for k in scalars} == {**scalars, "symmetric": True}
        assert np.array_equal(nt.weights_of_checkpoint(f).view(np.uint32), w.view(np.uint32))
    nt.write_checkpoint(tmp_path / "default.npz", w, tuples, **scalars)     # no lam given: today's file
    assert (tmp_path / "default.npz").read_bytes() == (tmp_path / "net1.npz").read_bytes()
    with pytest.raises(ValueError, match="exactly the scalars"):            # lam is a keyword of its own, not one of the scalars
        nt.write_checkpoint(tmp_path / "bad.npz", w, tuples, **{**scalars, "lambda": 0.5})
    with np.load(tmp_path / "net2.npz", allow_pickle=False) as raw:
        arrays = {k: raw[k] for k in raw.files}
    np.savez(open(tmp_path / "v3.npz", "wb"), **{**arrays, "version": np.array(3, dtype=np.int64)})
    with pytest.raises(ValueError, match="format version 3"):
        nt.read_checkpoint(tmp_path / "v3.npz")
    del arrays["lam"]
    np.savez(open(tmp_path / "v2_without.npz", "wb"), **arrays)
    with pytest.raises(ValueError, match="not an n-tuple network checkpoint"):
        nt.read_checkpoint(tmp_path / "v2_without.npz")


# ------------------------------------------------------------------ C7: what the compiler made
def test_lambda_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_lambda.hip with the Makefile's flags: one kernel, the walk (the scatter is
    csrc/tfe_ntuple.hip's), without scratch or a spilled vector register.  VGPRs as built: 68."""
    assert_no_scratch("ntuple-lambda-resource-usage", {"tfe_nt_lambda_walk_kernel": 1}, 128)
