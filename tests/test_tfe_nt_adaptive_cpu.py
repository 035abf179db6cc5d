"""The 2048 n-tuple network's expectimax play at a depth the board's empty cells choose, without a GPU: the host
mirror search_adaptive_nt_on_host against the two searches it chooses between and against the definition one board at a time
(tests/tfe_search_host.py), the library's two new entry points with their refusals, the Python layer's and the script's refusals, what the
host's games of tests/test_tfe_nt_adaptive_gpu.py exercise, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

from tests.native_args import assert_refusals, remarks
from tests.tfe_nt_support import CASES, CRAFTED, MORE, ROOT, SEARCH_CASES, SEARCH_UNIT, TUPLES, assert_exports, assert_no_scratch, bits, listed, opts, play_kernel, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of, scalar_search_on_host

SEARCH, EVALUATE = "pulse_tfe_nt_search_adaptive", "pulse_tfe_nt_evaluate_search_adaptive"
EMPTY = [0, 0, 0, 1, 2, 7, 7, 14, 15]                                       # of CRAFTED + MORE, sorted


@functools.lru_cache(maxsize=None)
def _boards():
    keys = np.array([key_of(c) for c in list(CRAFTED.values()) + list(MORE.values())], dtype=np.uint64)
    keys.setflags(write=False)
    return keys


# ------------------------------------------------------------------ the mirror
def test_count_empty_on_host():
    nt = _nt()
    n = nt.count_empty_on_host(_boards())
    assert n.dtype == np.int64 and n.shape == (9,) and sorted(n.tolist()) == EMPTY
    names = list(CRAFTED) + list(MORE)
    assert n[names.index("fourteen_empty")] == 14 and n[names.index("corner")] == 15 and n[names.index("one_empty")] == 1
    assert nt.count_empty_on_host([0]).tolist() == [16] and nt.count_empty_on_host(np.zeros(0, dtype=np.uint64)).shape == (0,)


@pytest.mark.parametrize("name,symmetric", [("zero", True), ("seeded", True), ("seeded", False)])
def test_sixteen_is_two_layers_and_a_board_above_the_threshold_is_one(name, symmetric):
    nt, keys = _nt(), _boards()
    one = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5)
    two = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5, layers=2)
    n = nt.count_empty_on_host(keys)
    for E in (16, 0, 1, 2, 3, 7, 14, 15):
        look = nt.search_adaptive_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5, E)
        assert sorted(look) == sorted(list(one) + ["deep"]) and look["deep"].dtype == np.bool_
        assert np.array_equal(look["deep"], n <= E) and (E != 16 or look["deep"].all())
        for k in one:
            want = np.where(look["deep"].reshape((-1,) + (1,) * (one[k].ndim - 1)), two[k], one[k])
            assert look[k].dtype == one[k].dtype and np.array_equal(look[k].view(np.uint8), want.view(np.uint8)), (E, k)
    assert (bits(one["q"]) != bits(two["q"])).any(axis=1).sum() >= 5       # the depths differ on these boards: the choice is seen


@pytest.mark.parametrize("name,symmetric", [("seeded", True), ("zero", False)])
def test_mirror_equals_the_scalar_definition_at_the_depth_the_count_gives(name, symmetric):
    nt, keys = _nt(), _boards()
    look = nt.search_adaptive_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5, 3)
    assert sorted(look["deep"].tolist()) == [False] * 4 + [True] * 5
    for i, key in enumerate(keys.tolist()):
        empty = sum(1 for c in range(16) if not (key >> (4 * c)) & 15)
        want = scalar_search_on_host(key, weights(name), TUPLES, symmetric, 1.0, 77, 5, 2 if empty <= 3 else 1)
        assert np.array_equal(bits(look["q"][i]), bits(want["q"])), (i, look["q"][i], want["q"])
        assert int(look["action"][i]) == want["action"] and int(look["candidates"][i]) == want["candidates"], i
        assert np.array_equal(bits(look["terms"][i]), bits(want["terms"])), i


def test_check_deep_empty_max():
    nt = _nt()
    assert nt.check_deep_empty_max(None) is None and nt.check_deep_empty_max(0) == 0 and nt.check_deep_empty_max(np.int64(16)) == 16
    for bad in (True, False, -1, 17, 2.0, "3", (3,)):
        with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
            nt.check_deep_empty_max(bad)
    for bad in (None, True, 17):
        with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
            nt.search_adaptive_nt_on_host(_boards()[:2], weights("zero"), TUPLES, True, 1.0, 9, 4, bad)


# ------------------------------------------------------------------ the library, without a GPU
def test_library_exports_the_two_adaptive_entry_points():
    from pulselib_amd import _native
    lib, text = assert_exports([(SEARCH, "PulseTfeNtSearch")], [C.c_void_p, C.c_int32, C.c_void_p],
                               r"int %s\(const %s\* o, int32_t deep_empty_max, void\* stream\);")
    assert_exports([(EVALUATE, "PulseTfeNtEval")], [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
                   r"int %s\(const %s\* o, int32_t deep_empty_max, int64_t\* depth_stats, void\* stream\);")
    assert C.sizeof(_native.TfeNtSearch) == 176 and C.sizeof(_native.TfeNtEval) == 208 and lib.pulse_version() == 1
    assert "n <= E" in text and "deep_empty_max must be in 0..16" in text


@pytest.mark.parametrize("E", [0, 3, 16])
def test_search_adaptive_refuses_what_search_deep_refuses(E):
    from pulselib_amd import _native
    errors = assert_refusals(_native.lib(), SEARCH, functools.partial(opts, _native.TfeNtSearch), SEARCH_CASES, E)
    assert len(errors) == len(SEARCH_CASES) and all(e.startswith(SEARCH.encode() + b": ") for e in errors)


@pytest.mark.parametrize("E,stats", [(0, None), (3, None), (16, 8 * 4096)])
def test_evaluate_search_adaptive_refuses_what_evaluate_refuses(E, stats):
    """... with depth_stats null and with an aligned one: a threshold at either end and a null depth_stats pass their checks, since the
    struct's refusals, which come after them, are reached"""
    from pulselib_amd import _native
    cases = CASES["pulse_tfe_nt_evaluate"]
    errors = assert_refusals(_native.lib(), EVALUATE, functools.partial(opts, _native.TfeNtEval), cases, E, stats)
    assert len(errors) == len(cases) and all(e.startswith(EVALUATE.encode() + b": ") for e in errors)


@pytest.mark.parametrize("E", [-1, 17])
def test_thresholds_outside_are_refused(E):
    """on structs every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib = _native.lib()
    for name, make, tail in ((SEARCH, functools.partial(opts, _native.TfeNtSearch), ()), (EVALUATE, functools.partial(opts, _native.TfeNtEval), (None,))):
        rc = getattr(lib, name)(C.byref(make()), E, *tail, None)
        assert rc == -1 and lib.pulse_last_error() == name.encode() + b": deep_empty_max must be in 0..16"
        with pytest.raises(ValueError, match=re.escape("deep_empty_max must be in 0..16")):
            _native.check(rc, name)


def test_a_depth_stats_off_its_alignment_is_refused():
    from pulselib_amd import _native
    lib = _native.lib()
    assert getattr(lib, EVALUATE)(C.byref(opts(_native.TfeNtEval)), 3, 4, None) == -1
    assert lib.pulse_last_error() == EVALUATE.encode() + b": depth_stats must be 8-byte aligned"


# ------------------------------------------------------------------ Python and the script
def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    agent = Agent.__new__(Agent)                                           # (no device: refused before anything is touched)
    agent.stage_tiles = ()
    calls = lambda **kw: (lambda: agent.search([0], **kw), lambda: agent.search_launch(None, None, None, None, **kw),
                          lambda: agent.evaluate_search(**kw), lambda: agent.evaluate_search_launch(**kw))
    for name in ("search", "search_launch", "evaluate_search", "evaluate_search_launch"):
        p = inspect.signature(getattr(Agent, name)).parameters
        assert list(p)[-1] == "deep_empty_max" and p["deep_empty_max"].default is None and p["layers"].default == 1
    assert list(inspect.signature(Agent.evaluate_launch).parameters) == ["self", "n_games", "epsilon", "board_id0", "per_game"]
    for bad in (True, 17, -1, 3.0):
        for call in calls(layers=2, deep_empty_max=bad):
            with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
                call()
    for call in calls(layers=1, deep_empty_max=3) + calls(deep_empty_max=3):
        with pytest.raises(ValueError, match="deep_empty_max needs layers = 2") as err:
            call()
        assert "deep_empty_max" in str(err.value) and "layers" in str(err.value)
    agent.stage_tiles = (512,)
    for call in calls(layers=2, deep_empty_max=3):
        with pytest.raises(ValueError, match=re.escape("layers = 2 on an agent with stage_tiles: two chance layers are not built on stages")):
            call()
    assert Agent.depth_stats is None


def test_script_refuses_the_option_where_it_does_not_apply(capsys):
    from pulselib_amd.scripts import tfe_ntuple as script
    assert inspect.signature(script.run).parameters["deep_empty_max"].default is None
    for argv, message in ((["--deep-empty-max", "3"], "--deep-empty-max needs --search --layers 2"),
                          (["--search", "--deep-empty-max", "3"], "--deep-empty-max needs --search --layers 2"),
                          (["--layers", "2", "--deep-empty-max", "3"], "--deep-empty-max needs --search --layers 2"),
                          (["--search", "--layers", "2", "--deep-empty-max", "17"], "--deep-empty-max must be in 0..16"),
                          (["--search", "--layers", "2", "--deep-empty-max", "3", "--stages", "512"], "--deep-empty-max does not go with --stages"),
                          (["--search", "--layers", "2", "--deep-empty-max", "3", "--add-stage", "1:512"], "--deep-empty-max does not go with --stages")):
        with pytest.raises(SystemExit) as err:
            script.main(argv)
        assert err.value.code == 2 and message in capsys.readouterr().err, argv
    for kw, message in ((dict(deep_empty_max=3), "--deep-empty-max needs --search --layers 2"),
                        (dict(search=True, layers=1, deep_empty_max=3), "--deep-empty-max needs --search --layers 2"),
                        (dict(search=True, layers=2, deep_empty_max=True), "deep_empty_max must be None or an int in 0..16"),
                        (dict(search=True, layers=2, deep_empty_max=3, stages=(512,)), "--deep-empty-max does not go with --stages")):
        with pytest.raises(ValueError, match=re.escape(message)):
            script.run(None, 0, **kw)                                      # (refused before a device is asked for)


# ------------------------------------------------------------------ the games the device is held to
@pytest.mark.parametrize("name,epsilon,symmetric,ended,cut,deep,shallow", [
    ("seeded", 0.0, True, [213, 244], 5, 1043, 694), ("seeded", .25, True, [101, 132, 178, 209], 3, 762, 626),
    ("seeded", .25, False, [143, 155, 157, 244], 3, 593, 874), ("zero", .25, True, [], 7, 330, 1462)])
def test_the_hosts_games_end_are_cut_and_move_at_both_depths(name, epsilon, symmetric, ended, cut, deep, shallow):
    """tests/tfe_nt_adaptive_support.py's games, as tests/test_tfe_nt_adaptive_gpu.py holds the device to them (about 2 s per case): on the seeded
    weights at least two games end, no two of them equally long; in every case at least two are cut, none is capped and each depth
    decides at least 200 moves.  The counts are those of the rehearsal, so that a change of the host's games is seen here."""
    from tests.tfe_nt_adaptive_support import CASES as PLAYED, GAMES, MAX_STEPS, host_games
    assert (name, epsilon, symmetric) in PLAYED
    want = host_games(name, epsilon, symmetric)
    L = want["lengths"]
    lengths = sorted(L[L < MAX_STEPS].tolist())
    assert want["truncated"] >= 2 and want["capped"] == 0 and want["ended"] + want["truncated"] == GAMES
    assert len(set(lengths)) == len(lengths) == want["ended"] and (name == "zero" or want["ended"] >= 2)
    assert want["deep"] >= 200 and want["shallow"] >= 200 and want["deep"] + want["shallow"] == int(L.sum())
    assert (lengths, want["truncated"], want["deep"], want["shallow"]) == (ended, cut, deep, shallow)


# ------------------------------------------------------------------ the compiler's remarks
def test_adaptive_search_kernels_use_no_scratch_and_keep_their_siblings_occupancy():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_search.hip with the Makefile's flags: twelve kernels, none with scratch or a
    spilled vector register, each of the four on NtAdaptiveDev with at least the waves per SIMD of its two-layer sibling as
    profiles/tfe_mc/kernel_resource_usage.txt lists it ahead of the merged unit.  VGPRs as built: boards 157 (symmetric) / 130, games 192 / 165."""
    target, waves = "ntuple-search-resource-usage", "Occupancy [waves/SIMD]"
    assert_no_scratch(target, SEARCH_UNIT, 256)
    older = (ROOT / "profiles" / "tfe_mc" / "kernel_resource_usage.txt").read_text()
    older = older[:older.index("tfe_ntuple_search.hip (merged)")]          # (the siblings, not this unit's own lines)
    for img in (8, 1):
        for mine, sibling in (("tfe_nt_search_kernelILi256ELi%dENS_13NtAdaptiveDevE" % img, "tfe_nt_search2_kernelILi%dE" % img),
                              (play_kernel(256, img, False, net="NtAdaptiveDev"), play_kernel(256, img, False))):
            assert listed(remarks(target), mine, waves) >= listed(older, sibling, waves) >= 2, (mine, sibling)
