"""The 2048 n-tuple network's weight sets by tile stage without a GPU: the stages struct and the four entry
points with their refusals, the host's statement of the stage (stage_of_keys_on_host) and of the staged features, three moves worked by
hand, equal slices against the one-stage mirrors, weight promotion (add_stage_on_host), the Python layer and the checkpoint, and what
the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import io
import re

import numpy as np
import pytest

from tests import tfe_host
from tests.native_args import PTR, assert_refusals, resource_usage
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_staged_support import STAGE_TILES, adds_per_stage, staged, stages_struct
from tests.tfe_nt_support import (BOARD_ID0, CASES, LAMBDA, ROOT, SEARCH_CASES, STEP_SIZE, V, X, Y, assert_no_scratch, play_kernels, bits, opts)
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of

ROLLOUT, LEARN, EVALUATE, SEARCH = ("pulse_tfe_nt_rollout_staged", "pulse_tfe_nt_learn_staged", "pulse_tfe_nt_evaluate_staged", "pulse_tfe_nt_search_staged")
SMALL = ((0, 1, 2, 3), (4, 5, 6, 7))                                       # 131,072 weights a stage: three stages of everything fit a host test
GAMES, MAX_STEPS, SEED = 33, 96, 457


# ------------------------------------------------------------------ the exports and the pins
def test_library_exports_the_struct_and_the_four_entry_points():
    from pulselib_amd import _native
    lib, text = _native.lib(), (ROOT / "include" / "pulse_env.h").read_text()
    s = _native.TfeNtStages
    assert C.sizeof(s) == 16 and [f[0] for f in s._fields_] == ["n_stages", "threshold", "reserved0"]
    assert [getattr(s, f[0]).offset for f in s._fields_] == [0, 4, 8] and s.threshold.size == 4
    assert _native.TFE_NT_MAX_STAGES == 4 and re.search(r"#define PULSE_TFE_NT_MAX_STAGES 4\n", text)
    assert re.search(r"typedef struct PulseTfeNtStages \{ int32_t n_stages; uint8_t threshold\[4\]; int64_t reserved0; \} PulseTfeNtStages;", text)
    protos = {ROLLOUT: ([C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
                        r"const PulseTfeNtRollout\* o, const PulseTfeNtStages\* stages, int32_t layers, double\* backed, uint64_t\* start,\s+void\* stream"),
              LEARN: ([C.c_void_p, C.c_void_p, C.c_void_p], r"const PulseTfeNtLearnBacked\* o, const PulseTfeNtStages\* stages, void\* stream"),
              EVALUATE: ([C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p], r"const PulseTfeNtEval\* o, const PulseTfeNtStages\* stages, int32_t layers, void\* stream"),
              SEARCH: ([C.c_void_p, C.c_void_p, C.c_void_p], r"const PulseTfeNtSearch\* o, const PulseTfeNtStages\* stages, void\* stream")}
    for name, (argtypes, args) in protos.items():
        assert hasattr(lib, name) and _native.SYMBOLS[name] == (C.c_int, argtypes), name
        assert re.search(r"int %s\(%s\);" % (name, args), text), name
    assert "static_assert(sizeof(PulseTfeNtStages) == 16" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_staged.hip").read_text()
    assert C.sizeof(_native.TfeNtLearnBacked) == 208 and C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
def _entries():
    """per entry point: (struct, the parent's cases, what stands between the stages and the stream)"""
    from pulselib_amd import _native
    learn = CASES["pulse_tfe_nt_learn"] + LAMBDA + [(dict(keys=4), b"keys / values / deltas / stats must be 8-byte aligned"),
                                                      (dict(deltas=4), b"keys / values / deltas / stats must be 8-byte aligned"),
                                                      (dict(backed=4), b"backed must be 8-byte aligned"), (dict(acc_abs=4), b"acc_abs must be 8-byte aligned"),
                                                      (dict(deltas=None), b"deltas is null"), (dict(deltas=None, backed=None, lam=1.0), b"deltas is null"),
                                                      (dict(deltas=None, backed=None, lam=5e-324), b"deltas is null")]
    return {ROLLOUT: (_native.TfeNtRollout, CASES["pulse_tfe_nt_rollout"], (1, None, PTR)), LEARN: (_native.TfeNtLearnBacked, learn, ()),
            EVALUATE: (_native.TfeNtEval, CASES["pulse_tfe_nt_evaluate"], (1,)), SEARCH: (_native.TfeNtSearch, SEARCH_CASES, ())}


@pytest.mark.parametrize("name", [ROLLOUT, LEARN, EVALUATE, SEARCH])
def test_a_staged_entry_point_refuses_what_its_parent_refuses(name):
    from pulselib_amd import _native
    struct, cases, tail = _entries()[name]
    st = stages_struct()
    errors = assert_refusals(_native.lib(), name, functools.partial(opts, struct), cases, C.byref(st), *tail)
    assert len(errors) == len(cases) and all(e.startswith(name.encode() + b": ") for e in errors)
    parent = {ROLLOUT: "pulse_tfe_nt_rollout", EVALUATE: "pulse_tfe_nt_evaluate", SEARCH: "pulse_tfe_nt_search"}.get(name)
    if parent:                                                             # the same messages, one copy of the checks
        plain = assert_refusals(_native.lib(), parent, functools.partial(opts, struct), cases)
        assert [e.split(b": ", 1)[1] for e in errors] == [e.split(b": ", 1)[1] for e in plain]


BAD_STAGES = [(dict(n_stages=0), b"n_stages must be in 1..4"), (dict(n_stages=5), b"n_stages must be in 1..4"), (dict(n_stages=-1), b"n_stages must be in 1..4"),
              (dict(threshold=[0, 5, 0, 0]), b"a threshold must be a nibble in 1..15"), (dict(threshold=[3, 16, 0, 0]), b"a threshold must be a nibble in 1..15"),
              (dict(threshold=[5, 3, 0, 0]), b"strictly increasing"), (dict(threshold=[3, 3, 0, 0]), b"strictly increasing"),
              (dict(threshold=[3, 5, 7, 0]), b"at or beyond n_stages - 1 must be 0"), (dict(threshold=[3, 5, 0, 1]), b"at or beyond n_stages - 1 must be 0"),
              (dict(n_stages=1, threshold=[3, 0, 0, 0]), b"at or beyond n_stages - 1 must be 0"), (dict(n_stages=4, threshold=[3, 5, 7, 9]), b"at or beyond n_stages - 1 must be 0"),
              (dict(reserved0=1), b"stages.reserved0 must be 0")]


@pytest.mark.parametrize("name", [ROLLOUT, LEARN, EVALUATE, SEARCH])
def test_a_staged_entry_point_refuses_bad_stages(name):
    """on a struct every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib, (struct, _, tail) = _native.lib(), _entries()[name]
    fn, o = getattr(lib, name), opts(struct)
    assert fn(C.byref(o), None, *tail, None) == -1 and lib.pulse_last_error() == name.encode() + b": stages are null"
    for kw, msg in BAD_STAGES:
        st = stages_struct(**kw)
        assert fn(C.byref(o), C.byref(st), *tail, None) == -1, kw
        assert lib.pulse_last_error().startswith(name.encode() + b": ") and msg in lib.pulse_last_error(), (kw, lib.pulse_last_error())
    for kw in (dict(n_stages=1, threshold=[0, 0, 0, 0]), dict(n_stages=4, threshold=[1, 2, 15, 0]), dict()):   # valid stages reach the next check
        if name in (ROLLOUT, EVALUATE):
            args = (2, None, PTR) if name == ROLLOUT else (2,)
            assert fn(C.byref(o), C.byref(stages_struct(**kw)), *args, None) == -1
            assert lib.pulse_last_error() == name.encode() + b": layers must be 0 or 1 (two layers are not built on stages)", kw


def test_the_rollouts_and_the_evaluations_own_refusals():
    from pulselib_amd import _native
    lib, st = _native.lib(), stages_struct()
    o = opts(_native.TfeNtRollout)
    own = [((2, None, PTR), b"layers must be 0 or 1 (two layers are not built on stages)"), ((-1, None, PTR), b"layers must be 0 or 1"),
           ((3, PTR, PTR), b"layers must be 0 or 1"), ((0, PTR, PTR), b"backed needs layers = 1"), ((1, PTR + 4, PTR), b"backed must be 8-byte aligned"),
           ((0, None, None), b"start is null"), ((1, PTR, None), b"start is null"), ((0, None, PTR + 4), b"start must be 8-byte aligned")]
    for args, msg in own:
        assert getattr(lib, ROLLOUT)(C.byref(o), C.byref(st), *args, None) == -1, args
        assert lib.pulse_last_error().startswith(ROLLOUT.encode() + b": " + msg), (args, lib.pulse_last_error())
    e = opts(_native.TfeNtEval)
    for layers in (2, -1, 3):
        assert getattr(lib, EVALUATE)(C.byref(e), C.byref(st), layers, None) == -1
        assert lib.pulse_last_error() == EVALUATE.encode() + b": layers must be 0 or 1 (two layers are not built on stages)"
    # net.reserved0 is still refused, under the new names
    for name, (struct, _, tail) in _entries().items():
        assert getattr(lib, name)(C.byref(opts(struct, net_reserved0=1)), C.byref(st), *tail, None) == -1
        assert lib.pulse_last_error() == name.encode() + b": net.reserved0 must be 0 (zero-initialise the struct)"


# ------------------------------------------------------------------ the stage of a board
def test_stage_of_keys_on_host_on_crafted_boards():
    nt = _nt()
    below3, at3, above3 = key_of([2, 1, 0, 0] + [0] * 12), key_of([3, 1, 0, 0] + [0] * 12), key_of([4, 1, 0, 0] + [0] * 12)
    at5, above5 = key_of([1, 5, 0, 0] + [0] * 12), key_of([1, 6, 3, 0] + [0] * 12)
    upper3, upper5, top = key_of([0] * 12 + [1, 2, 0, 3]), key_of([1] * 8 + [2] * 7 + [5]), key_of([0] * 15 + [15])
    keys = [0, below3, at3, above3, at5, above5, upper3, upper5, top]
    assert nt.stage_of_keys_on_host(keys, (8, 32)).tolist() == [0, 0, 1, 1, 2, 2, 1, 2, 2]
    assert nt.stage_of_keys_on_host(keys, ()).tolist() == [0] * 9
    assert nt.stage_of_keys_on_host(keys, (2,)).tolist() == [0] + [1] * 8                          # every board but the empty one holds a 2
    assert nt.stage_of_keys_on_host(keys, (8, 32, 32768)).tolist() == [0, 0, 1, 1, 2, 2, 1, 2, 3]
    assert nt.stage_of_keys_on_host(keys, (16, 64, 32768)).tolist() == [0, 0, 0, 1, 1, 2, 0, 1, 3]
    out = nt.stage_of_keys_on_host(np.array(keys, dtype=np.uint64), (8,))
    assert out.dtype == np.int64 and out.shape == (9,)
    # the largest nibble in every one of the sixteen cells
    one_hot = [key_of([5 if c == cell else 2 for c in range(16)]) for cell in range(16)]
    assert nt.stage_of_keys_on_host(one_hot, (8, 32)).tolist() == [2] * 16 and nt.stage_of_keys_on_host(one_hot, (8, 64)).tolist() == [1] * 16
    for bad in ((8, 8), (32, 8), (3,), (1,), (65536,), (2, 4, 8, 16), (True,), (8.0,)):
        with pytest.raises(ValueError):
            nt.check_stage_tiles(bad)
    assert nt.check_stage_tiles([2, 32768]) == (2, 32768) and nt.check_stage_tiles(()) == ()


def test_staged_features_are_the_plain_features_in_the_boards_own_slice():
    nt = _nt()
    rng = np.random.default_rng(3)
    keys = np.array([key_of(rng.integers(0, 7, 16)) for _ in range(200)] + [0], dtype=np.uint64)
    for symmetric in (True, False):
        plain = nt.feature_indices_on_host(keys, SMALL, symmetric)
        got = nt.feature_indices_on_host(keys, staged(SMALL), symmetric)
        stage = nt.stage_of_keys_on_host(keys, STAGE_TILES)
        assert set(stage.tolist()) == {0, 1, 2} and np.array_equal(got, plain + stage[:, None] * 131072)
        assert np.array_equal(nt.feature_indices_on_host(keys, nt.with_stages(SMALL, ()), symmetric), plain)
    tuples = staged(SMALL)
    assert isinstance(tuples, tuple) and tuples == SMALL and tuples.stage_tiles == STAGE_TILES and nt.stage_tiles_of(SMALL) == ()
    assert nt.check_tuples(tuples).stage_tiles == STAGE_TILES and type(nt.check_tuples(SMALL)) is tuple and nt.tuple_offsets(tuples) == nt.tuple_offsets(SMALL)


# ------------------------------------------------------------------ three moves worked by hand
def test_three_moves_worked_by_hand():
    """Tuple (0, 3), symmetric, W = 256 (tfe_nt_support.tc_worked: board X = nibble 1 in cell 0 reads the weights 1, 0, 0, 16, 1, 0, 0, 16;
    Y = nibble 2 in all four corners reads weight 34 eight times; V = nibble 1 in cell 0 and nibble 3 in cell 15 reads 1, 48, 3, 16, 1,
    48, 3, 16).  Two stages, the second from tile 8 (nibble 3): X and Y are in stage 0, V is in stage 1, so V's indices are 257, 304,
    259, 272, 257, 304, 259, 272.  One game of three moves, gamma 1, TD(0): afterstates X, Y, V with values 10, 4, 2, rewards 0, 1, 3, the
    last move terminal.
      move 0 (X, stage 0): delta = (1 + 4) - 10 = -5, d = -327,680: slice 0 gets weight 0 four times, weights 1 and 16 twice
      move 1 (Y, stage 0): delta = (3 + 2) - 4 = 1, d = 65,536 -- the target is V's value, recorded in stage 1: the difference crosses
                           the boundary by itself -- slice 0 gets weight 34 eight times
      move 2 (V, stage 1): delta = 0 - 2 = -2, d = -131,072: slice 1 gets weights 1, 3, 16 and 48 twice each
    The apply at step 1 / 8 on zero weights: slice 0 has w[0] = w[1] = w[16] = -0.625 and w[34] = 0.125, slice 1 has w[1] = w[3] = w[16] =
    w[48] = -0.25.  Afterwards V(X) = 8 * -0.625 = -5, V(Y) = 1, V(V) = 8 * -0.25 = -2; read without stages the same array gives V(V) =
    4 * -0.625 = -2.5."""
    nt = _nt()
    tuples = nt.with_stages(((0, 3),), (8,))
    keys = np.array([[X], [Y], [V]], dtype=np.uint64)
    values = np.array([[10.0], [4.0], [2.0]])
    steps = np.array([[0 | 0 << 2], [2 | 1 << 2], [1 | 3 << 2 | 0x80]], dtype=np.uint8)
    assert nt.stage_of_keys_on_host(keys, (8,)).tolist() == [0, 0, 1]
    assert nt.feature_indices_on_host(keys, tuples).tolist() == [[1, 0, 0, 16, 1, 0, 0, 16], [34] * 8, [257, 304, 259, 272, 257, 304, 259, 272]]
    acc = np.zeros((512, 2), dtype=np.int64)
    assert nt.learn_nt_on_host(keys, values, steps, [3], tuples, True, 1.0, acc) == dict(learnt=3, skipped=0, clamped=0)
    want = np.zeros((512, 2), dtype=np.int64)
    want[0], want[1], want[16], want[34] = (4 * -327680, 4), (2 * -327680, 2), (2 * -327680, 2), (8 * 65536, 8)
    for i in (1, 3, 16, 48):
        want[256 + i] = (2 * -131072, 2)
    assert np.array_equal(acc, want) and adds_per_stage(acc, 2) == [16, 8]
    lam_acc = np.zeros((512, 2), dtype=np.int64)                           # lambda = 0 through the walk: the same adds
    assert nt.learn_lambda_nt_on_host(keys, values, steps, [3], tuples, True, 1.0, 0.0, lam_acc)["learnt"] == 3 and np.array_equal(lam_acc, want)
    w = np.zeros(512, dtype=np.float32)
    assert nt.apply_nt_on_host(w, acc, STEP_SIZE) == 8 and not acc.any()
    want_w = np.zeros(512, dtype=np.float32)
    want_w[[0, 1, 16]], want_w[34], want_w[[257, 259, 272, 304]] = -0.625, 0.125, -0.25
    assert np.array_equal(w.view(np.uint32), want_w.view(np.uint32))
    assert nt.value_on_host([X, Y, V], w, tuples).tolist() == [-5.0, 1.0, -2.0]
    assert nt.value_on_host([V], w[:256], ((0, 3),)).tolist() == [-2.5]


# ------------------------------------------------------------------ equal slices are the one-stage network
@functools.lru_cache(maxsize=None)
def _host_round(staged_tuples):
    """(the games of a host roll-out at epsilon .25 on seeded weights, acc after the host's TD(0) learner) for SMALL with or without stages"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    nt = _nt()
    one = (np.random.default_rng(5).standard_normal(131072) * 4).astype(np.float32)
    tuples = staged(SMALL) if staged_tuples else SMALL
    w = np.tile(one, 3) if staged_tuples else one
    rec = nt_games_on_host(GAMES, MAX_STEPS, .25, 1.0, w, tuples, True, SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0, 0)
    acc = np.zeros((len(w), 2), dtype=np.int64)
    counts = nt.learn_nt_on_host(rec["keys"], rec["values"], rec["steps"], rec["lengths"], tuples, True, 1.0, acc)
    return rec, acc, counts, w


def test_equal_slices_give_the_one_stage_games_and_adds():
    nt = _nt()
    (plain, acc1, counts1, w1), (rec, acc3, counts3, w3) = _host_round(False), _host_round(True)
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward", "final_boards"):
        assert np.array_equal(rec[k], plain[k]), k
    assert np.array_equal(bits(rec["values"]), bits(plain["values"])) and counts1 == counts3 and int(rec["lengths"].sum()) > 10 * GAMES
    per_stage = adds_per_stage(acc3, 3)
    print("adds per stage", per_stage)
    assert all(n > 0 for n in per_stage)                                   # every stage's slice received adds
    assert np.array_equal(acc3.reshape(3, -1, 2).sum(axis=0), acc1)
    assert sum(per_stage) == 16 * counts3["learnt"] and counts3["skipped"] >= 1 and counts3["learnt"] + counts3["skipped"] == int(rec["lengths"].sum())
    played = np.arange(MAX_STEPS)[:, None] < rec["lengths"][None, :]
    keys = rec["keys"][played][::7]
    assert np.array_equal(bits(nt.value_on_host(keys, w3, staged(SMALL))), bits(nt.value_on_host(keys, w1, SMALL)))
    # search on equal slices: the same q bits, actions and candidates
    boards = tfe_host.pack_boards(rec["final_boards"])[:16]
    a, b = nt.search_nt_on_host(boards, w3, staged(SMALL), True, 1.0, 9, 2), nt.search_nt_on_host(boards, w1, SMALL, True, 1.0, 9, 2)
    assert np.array_equal(bits(a["q"]), bits(b["q"])) and np.array_equal(a["action"], b["action"]) and np.array_equal(a["candidates"], b["candidates"])


def test_distinct_slices_change_the_values_of_late_boards_only():
    nt = _nt()
    rec, _, _, w3 = _host_round(True)
    w = w3.copy()
    w[2 * 131072:] += np.float32(1.0)                                      # stage 2 alone
    played = np.arange(MAX_STEPS)[:, None] < rec["lengths"][None, :]
    keys = rec["keys"][played]
    stage = nt.stage_of_keys_on_host(keys, STAGE_TILES)
    before, after = nt.value_on_host(keys, w3, staged(SMALL)), nt.value_on_host(keys, w, staged(SMALL))
    assert np.array_equal(bits(before[stage < 2]), bits(after[stage < 2])) and (before[stage == 2] != after[stage == 2]).all() and (stage == 2).any()


# ------------------------------------------------------------------ weight promotion
def test_add_stage_leaves_every_value_unchanged():
    nt = _nt()
    rng = np.random.default_rng(17)
    keys = np.array([key_of(rng.integers(0, (3, 5, 9, 12)[i % 4], 16)) for i in range(500)], dtype=np.uint64)       # largest nibbles up to 2, 4, 8, 11
    w = (rng.standard_normal(131072) * 4).astype(np.float32)
    tuples, arrays = SMALL, [w]
    want = bits(nt.value_on_host(keys, w, SMALL))
    for tile, tiles in ((32, (32,)), (8, (8, 32)), (512, (8, 32, 512))):
        arrays, tuples = nt.add_stage_on_host(arrays, tuples, tile)
        assert tuples.stage_tiles == tiles and arrays[0].shape == ((len(tiles) + 1) * 131072,) and arrays[0].dtype == np.float32
        assert np.array_equal(bits(nt.value_on_host(keys, arrays[0], tuples)), want), tile
    assert len(set(nt.stage_of_keys_on_host(keys, tuples.stage_tiles).tolist())) == 4
    with pytest.raises(ValueError, match="stages already"):
        nt.add_stage_on_host(arrays, tuples, 2048)
    with pytest.raises(ValueError, match="begins at tile 8 already"):
        nt.add_stage_on_host([w, w], nt.with_stages(SMALL, (8,)), 8)
    # which slice is copied, and that accumulators start at zero: stages from (8, 512), split at 32 -> the new stage 2 copies stage 1
    three = np.repeat(np.arange(3, dtype=np.float32), 4)
    (grown, ints), t = nt.add_stage_on_host([three, three.astype(np.int64)], nt.with_stages(((0,),), (8, 512)), 32)
    assert grown.tolist() == ints.tolist() == [0] * 4 + [1] * 4 + [1] * 4 + [2] * 4 and t.stage_tiles == (8, 32, 512) and ints.dtype == np.int64
    (zeroed,), _ = nt.add_stage_on_host([three.astype(np.int64)], nt.with_stages(((0,),), (8, 512)), 32, copy=False)
    assert zeroed.tolist() == [0] * 4 + [1] * 4 + [0] * 4 + [2] * 4


# ------------------------------------------------------------------ the Python layer and the checkpoint
def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    nt = _nt()
    assert Agent.stage_tiles == () and nt.MAX_STAGES == 4 and nt.CHECKPOINT_VERSION_STAGED == 5
    assert list(inspect.signature(Agent.add_stage).parameters) == ["self", "tile"]
    assert list(inspect.signature(nt.stage_of_keys_on_host).parameters) == ["keys", "stage_tiles"]
    for bad in ((8, 8), (32, 8), (3,), (2, 4, 8, 16), (65536,)):           # refused by the call, before __init__ asks for a device
        with pytest.raises(ValueError, match="stage tile"):
            Agent(None, 8, stage_tiles=bad)
    agent = Agent.__new__(Agent)                                           # (no device: refused before anything is touched)
    agent.stage_tiles = (8, 32)
    assert agent.n_stages == 3
    st = agent._stages()
    assert st.n_stages == 3 and list(st.threshold) == [3, 5, 0, 0] and st.reserved0 == 0
    agent.rollout_layers = 2
    with pytest.raises(ValueError, match="two chance layers are not built on stages"):
        agent.rollout()
    with pytest.raises(ValueError, match="two chance layers are not built on stages"):
        agent.learn_batch()
    agent.rollout_layers = 0
    for call in (lambda: agent.rollout(layers=2), lambda: agent.search([1], layers=2), lambda: agent.evaluate_search(layers=2),
                 lambda: agent.evaluate_search_launch(layers=2), lambda: agent.search_launch(None, None, None, None, layers=2),
                 lambda: agent.rollout_staged_launch(2)):
        with pytest.raises(ValueError, match="two chance layers are not built on stages"):
            call()
    agent.backed_targets = True
    with pytest.raises(ValueError, match="backed_targets needs rollout_layers"):
        agent.rollout()
    with pytest.raises(ValueError, match="begins at tile 8 already"):
        agent.add_stage(8)
    agent.stage_tiles = (8, 32, 512)
    with pytest.raises(ValueError, match="4 stages already"):
        agent.add_stage(2048)
    with pytest.raises(ValueError, match="power of two"):
        agent.add_stage(24)
    from pulselib_amd.scripts import tfe_ntuple as script
    with pytest.raises(SystemExit):
        script.main(["--stages", "512,2048", "--train-layers", "2"])
    with pytest.raises(SystemExit):
        script.main(["--stages", "512;2048"])
    with pytest.raises(ValueError, match="do not go with two chance layers"):
        script.run(None, 1, stages=(512,), search=True, layers=2)
    with pytest.raises(SystemExit):
        script.main(["--add-stage", "3:256", "--add-stage", "3:512"])
    with pytest.raises(ValueError, match="names a round twice"):
        script.run(None, 8, add_stage=((3, 256), (3, 512)))
    for rounds, pairs in ((4, ((4, 256),)), (4, ((-1, 256),)), (0, ((0, 256),)), (6, ((2, 256), (9, 1024)))):
        with pytest.raises(ValueError, match="outside the rounds this run plays"):
            script.run(None, rounds, add_stage=pairs)
    assert script._promotions(((2, 256), (5, 1024)), 2, 4) == {2: 256, 5: 1024} and script._promotions((), 0, 0) == {}


SCALARS = dict(symmetric=1, gamma=1.0, epsilon=0.0, alpha=1.0, max_steps=64, seed=3, board_id0=5, round=7, n_games=8)


def _parents_bytes(weights, tuples, lam, tc):
    """the file the package wrote before it knew stages: np.savez of the same arrays in the same order"""
    nt = _nt()
    index = np.flatnonzero(weights.view(np.uint32) != 0)
    cells = np.full((len(tuples), nt.MAX_LEN), -1, dtype=np.int64)
    for i, t in enumerate(tuples):
        cells[i, :len(t)] = t
    dtypes = dict(gamma=np.float64, epsilon=np.float64, alpha=np.float64, seed=np.uint64, board_id0=np.uint64)
    arrays = {k: np.array(SCALARS[k], dtype=dtypes.get(k, np.int64)) for k in nt.CHECKPOINT_SCALARS}
    version = 1
    if lam != 0.0 or tc is not None:
        arrays["lam"], version = np.array(lam, dtype=np.float64), 2
    if tc is not None:
        at = np.flatnonzero((tc[0].view(np.uint64) != 0) | (tc[1].view(np.uint64) != 0))
        arrays.update(tc_index=at.astype(np.int64), tc_e=tc[0][at], tc_a=tc[1][at])
        version = 4
    fh = io.BytesIO()
    np.savez(fh, version=np.array(version, dtype=np.int64), index=index.astype(np.int64), value=weights[index],
             tuple_len=np.array([len(t) for t in tuples], dtype=np.int64), tuple_cells=cells, **arrays)
    return fh.getvalue()


def test_the_checkpoint(tmp_path):
    nt = _nt()
    tuples, W = ((0, 3), (5, 6, 9)), 256 + 4096
    rng = np.random.default_rng(2)
    w = np.zeros(3 * W, dtype=np.float32)
    w[rng.choice(3 * W, 200, replace=False)] = rng.standard_normal(200).astype(np.float32)
    w[[0, W, 3 * W - 1]] = (1.5, -2.5, 3.5)                                # the first weight of two stages and the very last one
    E, A = np.zeros(3 * W), np.zeros(3 * W)
    E[[1, W + 1, 3 * W - 1]], A[[1, 2 * W, 3 * W - 1]] = (0.5, -0.25, 2.0), (0.75, 1.0, 2.0)
    # without stages: the parent's bytes, for lam and tc off and on
    for lam, tc in ((0.0, None), (0.5, None), (0.0, (E[:W], A[:W])), (0.5, (E[:W], A[:W]))):
        path = tmp_path / f"plain_{lam}_{tc is not None}.npz"
        nt.write_checkpoint(path, w[:W], tuples, lam=lam, tc=tc, **SCALARS)
        assert path.read_bytes() == _parents_bytes(w[:W], tuples, lam, tc), (lam, tc is not None)
        nt.write_checkpoint(tmp_path / "again.npz", w[:W], tuples, lam=lam, tc=tc, stage_tiles=(), **SCALARS)
        assert (tmp_path / "again.npz").read_bytes() == path.read_bytes()
        f = nt.read_checkpoint(path)
        assert f["stage_tiles"] == () and f["n_weights"] == W and type(f["tuples"]) is tuple and f["tc"] == (tc is not None)
    # version 5, without and with tc
    for tc in (None, (E, A)):
        path = tmp_path / f"staged_{tc is not None}.npz"
        nt.write_checkpoint(path, w, tuples, lam=0.0, tc=tc, stage_tiles=(8, 32), **SCALARS)
        with np.load(path, allow_pickle=False) as raw:
            assert int(raw["version"]) == 5 and raw["stage_tiles"].tolist() == [8, 32] and raw["stage_tiles"].dtype == np.int64
            assert ("tc_index" in raw.files) == (tc is not None) and "lam" in raw.files and int(raw["index"][-1]) == 3 * W - 1
            arrays = {k: raw[k] for k in raw.files}
        f = nt.read_checkpoint(path)
        assert f["stage_tiles"] == (8, 32) and f["tuples"].stage_tiles == (8, 32) and f["n_weights"] == 3 * W and f["lam"] == 0.0 and f["tc"] == (tc is not None)
        assert np.array_equal(nt.weights_of_checkpoint(f).view(np.uint32), w.view(np.uint32)) and f["round"] == 7 and f["seed"] == 3
        if tc is not None:
            e, a = nt.coherence_of_checkpoint(f)
            assert np.array_equal(bits(e), bits(E)) and np.array_equal(bits(a), bits(A))

    def refused(match, **change):
        new = {k: v for k, v in {**arrays, **change}.items() if v is not None}
        with open(tmp_path / "bad.npz", "wb") as fh:
            np.savez(fh, **new)
        with pytest.raises(ValueError, match=match):
            nt.read_checkpoint(tmp_path / "bad.npz")
    refused("format version 6", version=np.array(6, dtype=np.int64))
    refused("format version 3", version=np.array(3, dtype=np.int64))
    refused("holds no stage_tiles", stage_tiles=None)
    refused("strictly increasing", stage_tiles=np.array([32, 8], dtype=np.int64))
    refused("power of two", stage_tiles=np.array([8, 24], dtype=np.int64))
    refused("at least one stage tile", stage_tiles=np.zeros(0, dtype=np.int64))
    refused("strictly ascending inside the network's", index=arrays["index"] + 1)       # the last index is beyond 3 * W
    refused("strictly ascending inside the network's", stage_tiles=np.array([8], dtype=np.int64))     # two stages do not hold index 3 W - 1


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_staged_kernels_use_no_scratch_and_stay_within_the_recorded_registers():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_staged.hip with the Makefile's flags: twenty kernels, none with scratch or a spilled
    vector register, each within the VGPR count of its line in profiles/tfe_mc/kernel_resource_usage.txt's latest listing of the unit."""
    staged = dict(net="NtStagedDev")
    counts = {**play_kernels(1, True, start=True, **staged), **play_kernels(32, True, start=True, **staged), **play_kernels(32, True, backed=True, start=True, **staged),
              **play_kernels(1, False, **staged), **play_kernels(32, False, **staged), "tfe_nt_search_kernel": 2, "tfe_nt_scatter_kernel": 8}
    names = assert_no_scratch("ntuple-staged-resource-usage", counts, 165 + 4)
    text = (ROOT / "profiles" / "tfe_mc" / "kernel_resource_usage.txt").read_text().rpartition("# tfe_ntuple_staged.hip")[2]
    recorded = dict(re.findall(r"^tfe_ntuple\w*\.h:\d+:\d+: Function Name: (\S+NtStagedDev\S+)\n.*\n.*VGPRs: (\d+)$", text, flags=re.M))
    _, vgprs, _, _ = resource_usage("ntuple-staged-resource-usage")
    assert sorted(recorded) == sorted(names) and len(names) == 20
    for name, v in zip(names, vgprs):
        assert v <= int(recorded[name]), (name, v, recorded[name])
