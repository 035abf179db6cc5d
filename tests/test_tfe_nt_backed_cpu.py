"""The 2048 n-tuple network's search-backed TD targets without a GPU: the library's two entry points with
their refusals, the new struct's layout, the host's statement of the backed-up value (search_nt_on_host's `backed`) against the scalar
definition and on one board worked by hand, the learner's mirror (backed_deltas_on_host, learn_backed_nt_on_host) on a hand-worked
game of four moves and a cut game, the Python layer's attribute, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import re
from fractions import Fraction

import numpy as np
import pytest

from tests.native_args import PTR, assert_refusals, remarks
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import BOARD_ID0, CASES, CRAFTED, MORE, P, ROOT, TUPLES, assert_exports, assert_no_scratch, play_kernels, bits, opts, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of, scalar_search_on_host

ROLLOUT, LEARN = "pulse_tfe_nt_rollout_backed", "pulse_tfe_nt_learn_backed"


# ------------------------------------------------------------------ the exports and the pins
def test_library_exports_the_two_entry_points():
    from pulselib_amd import _native
    assert_exports(((ROLLOUT, "PulseTfeNtRollout"),), [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
                   r"int %s\(const %s\* o, int32_t layers, double\* backed, void\* stream\);")
    lib, text = assert_exports(((LEARN, "PulseTfeNtLearnBacked"),), [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    assert re.search(r"typedef struct PulseTfeNtLearnBacked \{", text) and "Zero-initialise it" in text
    s, tc = _native.TfeNtLearnBacked, _native.TfeNtLearnTc
    assert C.sizeof(s) == 208
    assert [f[0] for f in s._fields_] == [f[0] for f in tc._fields_] + ["backed"]    # PulseTfeNtLearnTc's fields in order, then backed
    assert all(getattr(s, f[0]).offset == getattr(tc, f[0]).offset for f in tc._fields_) and (s.reserved0.offset, s.backed.offset) == (192, 200)
    assert "static_assert(sizeof(PulseTfeNtLearnBacked) == 208" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_backed.hip").read_text()
    assert C.sizeof(_native.TfeNtRollout) == 232 and C.sizeof(tc) == 200 and lib.pulse_version() == 1


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
@pytest.mark.parametrize("layers", [1, 2])
def test_the_recording_launch_refuses_what_the_rollout_refuses(layers):
    from pulselib_amd import _native
    cases, make = CASES["pulse_tfe_nt_rollout"], functools.partial(opts, _native.TfeNtRollout)
    errors = assert_refusals(_native.lib(), ROLLOUT, make, cases, layers, PTR)
    plain = assert_refusals(_native.lib(), "pulse_tfe_nt_rollout", make, cases)
    assert len(errors) == len(cases) and all(e.startswith(ROLLOUT.encode() + b": ") for e in errors)
    assert [e.split(b": ", 1)[1] for e in errors] == [e.split(b": ", 1)[1] for e in plain]     # the same messages, one copy of the checks


@pytest.mark.parametrize("layers", [0, 3, -1])
def test_other_depths_are_refused(layers):
    """on a struct every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib = _native.lib()
    rc = getattr(lib, ROLLOUT)(C.byref(opts(_native.TfeNtRollout)), layers, PTR, None)
    assert rc == -1 and lib.pulse_last_error() == ROLLOUT.encode() + b": layers must be 1 or 2"


@pytest.mark.parametrize("layers", [1, 2])
def test_a_null_or_misaligned_backed_is_refused(layers):
    from pulselib_amd import _native
    lib = _native.lib()
    for backed, msg in ((None, b"backed is null"), (PTR + 4, b"backed must be 8-byte aligned")):
        assert getattr(lib, ROLLOUT)(C.byref(opts(_native.TfeNtRollout)), layers, backed, None) == -1
        assert lib.pulse_last_error() == ROLLOUT.encode() + b": " + msg


def test_the_learner_refuses():
    """what check_moves refuses and pulse_tfe_nt_learn_lambda's own (lambda outside [0, 1], deltas null, misalignment), under its own
    name, then backed null or misaligned and acc_abs misaligned; acc_abs may be null"""
    from pulselib_amd import _native
    lib, make = _native.lib(), functools.partial(opts, _native.TfeNtLearnBacked)
    own = [(dict(backed=None), b"backed is null"), (dict(backed=4), b"backed must be 8-byte aligned"), (dict(acc_abs=4), b"acc_abs must be 8-byte aligned")]
    errors = assert_refusals(lib, LEARN, make, CASES["pulse_tfe_nt_learn_lambda"] + own)
    assert len(errors) == len(CASES["pulse_tfe_nt_learn_lambda"]) + 3
    assert any(b"reserved0 must be 0" in e for e in errors) and any(b"lambda must be in [0, 1]" in e for e in errors)
    assert sum(b"deltas is null" in e for e in errors) == 1
    o = make(acc_abs=None, net_weights=None, lengths=2)                     # no third accumulator and no weights: the next check refuses
    assert getattr(lib, LEARN)(C.byref(o), None) == -1 and b"lengths must be 4-byte aligned" in lib.pulse_last_error()
    for lam in (0.0, 1.0):                                                 # the ends of the interval are inside
        assert getattr(lib, LEARN)(C.byref(make(lam=lam, keys=None)), None) == -1 and b"keys is null" in lib.pulse_last_error()


# ------------------------------------------------------------------ the backed-up value on the host
@functools.lru_cache(maxsize=None)
def _crafted():
    keys = np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64)
    keys.setflags(write=False)
    return keys


@pytest.mark.parametrize("layers", [1, 2])
def test_backed_is_the_largest_q_over_the_candidates(layers):
    nt, keys = _nt(), _crafted()
    look = nt.search_nt_on_host(keys, weights("seeded"), TUPLES, True, 1.0, 77, 5, layers=layers)
    assert look["backed"].dtype == np.float64 and look["backed"].shape == (len(keys),)
    some = 0
    for i, key in enumerate(keys.tolist()):
        want = scalar_search_on_host(key, weights("seeded"), TUPLES, True, 1.0, 77, 5, layers)
        cand = [a for a in range(4) if want["candidates"] >> a & 1]
        best = max((want["q"][a] for a in cand), default=np.float64(0.0))
        assert bits(look["backed"][i]) == bits(best), (i, look["backed"][i], best)
        if cand:                                                           # greedy play takes a move of that q: at epsilon = 0 it is q[action]
            assert look["backed"][i] == look["q"][i, look["action"][i]], i
            some += 1
        else:
            assert bits(look["backed"][i]) == 0 and int(look["action"][i]) == -1
    assert some >= len(keys) - 2
    # the scan, on its own: the first candidate starts (a negative q too), a larger one replaces, a non-candidate's +0.0 never enters
    q = np.array([[0.0, -3.0, -2.0, 0.0], [5.0, 5.0, 7.0, 9.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]])
    cand = np.array([[0, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=bool)
    assert nt.search_backed_on_host(q, cand).tolist() == [-2.0, 7.0, 0.0, 1.0]


def test_one_board_worked_by_hand():
    """tests/test_tfe_nt_search_rollout_cpu.py's board: ONE_MERGE on the one tuple (0, 1, 2, 3) with the single weight 2.5, gamma 1, one
    layer: q_left = 4 + 5.5 P_2 and q_right = 4 + 6.5 P_1 + 5.5 P_2, up and down are no candidates.  backed of move 0 is the larger,
    q_right; the record beside it is still V = 2.5 of the network with the byte 18."""
    nt = _nt()
    tuples, key = ((0, 1, 2, 3),), key_of(CRAFTED["one_merge"])
    w = np.zeros(16 ** 4, dtype=np.float32)
    w[8481] = 2.5
    q_right = float(4 + Fraction(13, 2) * P[0] + Fraction(11, 2) * P[1])
    look = nt.search_nt_on_host([key], w, tuples, False, 1.0, 1, 0)
    assert look["backed"].tolist() == [q_right] and look["q"][0, 2] == q_right and look["q"][0, 0] < q_right
    boards0 = (1 << np.array(CRAFTED["one_merge"], dtype=np.int32)).reshape(1, 4, 4)
    for epsilon in (0.0, 1.0):                                             # whatever the action taken
        got = nt_games_on_host(1, 1, epsilon, 1.0, w, tuples, False, 11, 12, 1, 500, 0, depth=1, backed=True, boards0=boards0)
        assert got["backed"].shape == (1, 1) and got["backed"][0, 0] == q_right and got["lengths"].tolist() == [1]
    got = nt_games_on_host(1, 1, 0.0, 1.0, w, tuples, False, 11, 12, 1, 500, 0, depth=1, backed=True, boards0=boards0)
    assert got["values"][0, 0] == 2.5 and int(got["steps"][0, 0]) == 18


def test_recording_the_backed_value_does_not_change_play():
    """the roll-out one layer deep with and without `backed`; the records the two share come from one policy, so the values and the
    backed values are also held to the package's mirrors: value_on_host of the recorded afterstates, and search_backed_on_host of
    the search's q on the boards before the moves 0, 10 and 23"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_host import pack_boards
    nt = _nt()
    args = (5, 24, .25, 1.0, weights("seeded"), TUPLES, True, 2312, 2312 ^ AGENT_KEY, 2312 ^ TIE_KEY, BOARD_ID0, 0)
    got, want = nt_games_on_host(*args, depth=1, backed=True), nt_games_on_host(*args, depth=1, keep_boards="before")
    assert "backed" not in want
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward", "final_boards"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["values"]), bits(want["values"])) and got["greedy"] == want["greedy"] < int(want["lengths"].sum())
    played = np.arange(24)[:, None] < got["lengths"][None, :]
    assert got["backed"][played].all() and not got["backed"][~played].any()
    assert np.array_equal(bits(got["values"][played]), bits(nt.value_on_host(got["keys"][played], weights("seeded"), TUPLES, True)))
    for t in (0, 10, 23):
        live = np.flatnonzero(got["lengths"] > t)
        keys = pack_boards(want["boards"][t][live])
        look = nt.search_nt_on_host(keys, weights("seeded"), TUPLES, True, 1.0, 2312 ^ TIE_KEY, 0)
        assert live.size and np.array_equal(bits(got["backed"][t, live]), bits(nt.search_backed_on_host(look["q"], look["after"] != keys[:, None]))), t


# ------------------------------------------------------------------ the learner's mirror, worked by hand
def _worked():
    """Tuple (0, 3), board X = 0x1 in every move (it reads weight 0 four times, 1 and 16 twice each), gamma 1.  Game 0 ends at t = 3:
    V = 10, 20000, 2, 5 and backed = (unused), 20001, 7, 6, so delta = 19991, -19993, 4, -5 (the last: target 0).  Game 1 is cut at
    length 2: V = 1.5, 7 and backed = (unused), 9.25, so delta_0 = 7.75 and its last move is skipped.  backed of move 0 is nobody's
    target, and the rows beyond game 1's length hold NaN: neither may show."""
    keys = np.full((4, 2), 0x1, dtype=np.uint64)
    values = np.array([[10.0, 1.5], [20000.0, 7.0], [2.0, -99.0], [5.0, -99.0]])
    backed = np.array([[999.0, -999.0], [20001.0, 9.25], [7.0, np.nan], [6.0, np.nan]])
    steps = np.array([[0 | 0 << 2, 1 | 2 << 2], [2 | 1 << 2, 3 | 2 << 2], [1 | 3 << 2, 0xEE], [3 | 4 << 2 | 0x80, 0xEE]], dtype=np.uint8)
    return keys, values, backed, steps, [4, 2]


def test_a_hand_worked_game():
    """lambda .5.  Game 0: D_3 = -5; D_2 = 4 + .5 * -5 = 1.5; D_1 = -19993 + .75 = -19992.25, which its add clamps to -8,192; D_0 = 19991
    + .5 * -19992.25 = 9994.875 -- from the UNCLAMPED D_1 (the clamped one would give 15,895) -- which clamps to 8,192.  Game 1:
    D_1 = +0.0 (skipped), D_0 = 7.75.  Five moves learnt, one skipped, two clamped."""
    nt = _nt()
    keys, values, backed, steps, lengths = _worked()
    deltas = nt.backed_deltas_on_host(values, backed, steps, lengths, 1.0, 0.5)
    assert deltas.dtype == np.float64 and deltas.tolist() == [[9994.875, 7.75], [-19992.25, 0.0], [1.5, 0.0], [-5.0, 0.0]]
    assert bits(deltas)[1:, 1].tolist() == [0, 0, 0]                        # +0.0: the skipped move and the rows beyond game 1's length
    acc, ab = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    st = nt.learn_backed_nt_on_host(keys, values, backed, steps, lengths, ((0, 3),), True, 1.0, 0.5, acc, ab)
    assert np.array_equal(bits(st.pop("deltas")), bits(deltas)) and st == dict(learnt=5, skipped=1, clamped=2)
    d = [8192 * 65536, -8192 * 65536, 98304, -327680, 507904]
    want, want_ab = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    want[0], want[1], want[16] = (4 * sum(d), 20), (2 * sum(d), 10), (2 * sum(d), 10)
    want_ab[0], want_ab[1], want_ab[16] = 4 * sum(map(abs, d)), 2 * sum(map(abs, d)), 2 * sum(map(abs, d))
    assert np.array_equal(acc, want) and np.array_equal(ab, want_ab)
    acc2 = np.zeros((256, 2), dtype=np.int64)                              # without the third accumulator: the same acc
    assert nt.learn_backed_nt_on_host(keys, values, backed, steps, lengths, ((0, 3),), True, 1.0, 0.5, acc2)["learnt"] == 5 and np.array_equal(acc2, want)
    # the rewards of the step bytes are inside backed already: other reward bits, the same differences
    other = steps ^ np.uint8(0x7C)
    assert np.array_equal(bits(nt.backed_deltas_on_host(values, backed, other, lengths, 1.0, 0.5)), bits(deltas))
    # a length beyond the rows there are is clamped: game 0 as before
    assert nt.backed_deltas_on_host(values, backed, steps, [9, 2], 1.0, 0.5)[:, 0].tolist() == deltas[:, 0].tolist()


def test_lambda_zero_is_the_one_step_difference():
    nt = _nt()
    keys, values, backed, steps, lengths = _worked()
    for gamma in (1.0, 0.9):                                               # gamma is inside backed: at lambda 0 it does not enter again
        deltas = nt.backed_deltas_on_host(values, backed, steps, lengths, gamma, 0.0)
        assert bits(deltas)[:3, 0].tolist() == bits(backed[1:, 0] - values[:3, 0]).tolist() and deltas[3, 0] == 0.0 - 5.0
        assert deltas[:, 1].tolist() == [9.25 - 1.5, 0.0, 0.0, 0.0]
    # ... and where the product's rounding shows: gl = fl(.9 * .5)
    gl = np.float64(0.9) * np.float64(0.5)
    got = nt.backed_deltas_on_host(values, backed, steps, lengths, 0.9, 0.5)[:, 0]
    d3 = 0.0 - 5.0
    d2 = (6.0 - 2.0) + gl * d3
    d1 = (7.0 - 20000.0) + gl * d2
    d0 = (20001.0 - 10.0) + gl * d1
    assert bits(got).tolist() == bits([d0, d1, d2, d3]).tolist()


def test_lambda_one_is_the_sum_of_the_later_differences():
    nt = _nt()
    keys, values, backed, steps, lengths = _worked()
    deltas = nt.backed_deltas_on_host(values, backed, steps, lengths, 1.0, 1.0)
    one_step = [19991.0, -19993.0, 4.0, -5.0]
    assert deltas[:, 0].tolist() == [sum(one_step[t:]) for t in range(4)] == [-3.0, -19994.0, -1.0, -5.0]
    assert deltas[:, 1].tolist() == [7.75, 0.0, 0.0, 0.0]                   # the skipped move passes +0.0 down


# ------------------------------------------------------------------ the Python layer
def test_python_layer(tmp_path):
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    nt = _nt()
    assert NTupleTDAfterstateTFEGPU.backed_targets is False
    from tests.tfe_nt_support import assert_init_parameters
    assert_init_parameters(NTupleTDAfterstateTFEGPU)
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.rollout).parameters) == ["self", "layers"]
    assert inspect.signature(NTupleTDAfterstateTFEGPU.rollout).parameters["layers"].default is None
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.learn_batch).parameters) == ["self"]
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.rollout_backed_launch).parameters) == ["self", "layers"]
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.learn_backed_launch).parameters) == ["self", "lam"]
    assert callable(NTupleTDAfterstateTFEGPU.trajectory_backed)
    assert list(inspect.signature(nt.backed_deltas_on_host).parameters) == ["values", "backed", "steps", "lengths", "gamma", "lam"]
    assert list(inspect.signature(nt.learn_backed_nt_on_host).parameters) == ["keys", "values", "backed", "steps", "lengths", "tuples", "symmetric", "gamma",
                                                                              "lam", "acc", "acc_abs"]
    agent = NTupleTDAfterstateTFEGPU.__new__(NTupleTDAfterstateTFEGPU)        # (no device: refused before anything is touched)
    agent.backed_targets = True
    assert agent.rollout_layers == 0
    with pytest.raises(ValueError, match="backed_targets needs rollout_layers in"):
        agent.rollout()
    agent.rollout_layers = 2
    with pytest.raises(ValueError, match="backed_targets needs rollout_layers in"):
        agent.rollout(layers=0)                                            # the argument is the depth of this launch
    for bad in (3, True, -1):
        agent.rollout_layers = bad
        with pytest.raises(ValueError, match="rollout_layers must be 0, 1 or 2"):
            agent.rollout()
    for bad in (0, 3, True):
        with pytest.raises(ValueError, match="layers must be 1 or 2"):
            agent.rollout_backed_launch(bad)
    # the script refuses --backed without a search to back a value up, before it asks for a device
    from pulselib_amd.scripts import tfe_ntuple as script
    with pytest.raises(SystemExit):
        script.main(["--backed"])
    with pytest.raises(ValueError, match="--backed needs --train-layers"):
        script.run(None, 1, backed=True)
    # the checkpoint: today's keys and versions
    assert nt.CHECKPOINT_SCALARS == ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")
    assert (nt.CHECKPOINT_VERSION, nt.CHECKPOINT_VERSION_LAMBDA, nt.CHECKPOINT_VERSION_TC) == (1, 2, 4)
    scalars = dict(symmetric=1, gamma=1.0, epsilon=0.0, alpha=1.0, max_steps=64, seed=0, board_id0=0, round=3, n_games=8)
    nt.write_checkpoint(tmp_path / "net.npz", np.zeros(16, dtype=np.float32), ((0,),), **scalars)
    with np.load(tmp_path / "net.npz", allow_pickle=False) as raw:
        assert sorted(raw.files) == sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS)
    assert "backed_targets" not in nt.read_checkpoint(tmp_path / "net.npz")


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_backed_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_backed.hip with the Makefile's flags: the four game kernels and the walk with
    Backed set, none with scratch or a spilled vector register.  VGPRs as built: one layer 160 (symmetric) / 135, two layers 204 / 177,
    the walk 98."""
    names = assert_no_scratch("ntuple-backed-resource-usage",
                              {**play_kernels(32, True, backed=True), **play_kernels(256, True, backed=True), "tfe_nt_lambda_walk_kernel": 1}, 256)
    assert all("ILb1E" in n for n in names if "tfe_nt_lambda_walk_kernel" in n)      # the walk here is the Backed one
    assert "scatter" not in " ".join(names) and len(re.findall(r"Function Name:", remarks("ntuple-backed-resource-usage"))) == 5
