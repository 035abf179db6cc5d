"""The 2048 n-tuple network's expectimax play two chance layers deep without a GPU: the host mirror
search_nt_on_host(layers=2) against the definition restated one board at a time in plain Python (tests/tfe_search_host.py), a
hand-worked board, what does not change at one layer, the library's two new entry points with their refusals, and what the compiler
made of the kernels."""
import ctypes as C
import functools
import inspect

import numpy as np
import pytest

from tests.native_args import assert_refusals
from tests.tfe_nt_support import CASES, CRAFTED, P, SEARCH_CASES, SEARCH_UNIT, TUPLES, assert_exports, assert_no_scratch, bits, opts, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of, scalar_search_on_host

NAMES = (("pulse_tfe_nt_search_deep", "PulseTfeNtSearch"), ("pulse_tfe_nt_evaluate_search_deep", "PulseTfeNtEval"))
ONE_MERGE = key_of(CRAFTED["one_merge"])


@functools.lru_cache(maxsize=None)
def _boards():
    """uint64[18]: the crafted boards, then moves 6 and 40 of five one-layer host games on the seeded weights"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_host import pack_boards
    from tests.tfe_nt_host import nt_games_on_host
    games = nt_games_on_host(5, 41, .25, 1.0, weights("seeded"), TUPLES, True, 11, 11 ^ AGENT_KEY, 11 ^ TIE_KEY, 500, 0, depth=1, record=False, keep_boards="before")
    assert games["lengths"].min() == 41
    keys = np.concatenate([np.array([key_of(c) for c in CRAFTED.values()], dtype=np.uint64), pack_boards(games["boards"][6]),
                           pack_boards(games["boards"][40])])
    keys.setflags(write=False)
    return keys


# ------------------------------------------------------------------ the mirror against the definition, board by board
@pytest.mark.parametrize("name,symmetric", [("zero", True), ("seeded", True), ("zero", False), ("seeded", False)])
def test_mirror_equals_the_scalar_definition(name, symmetric):
    nt, keys = _nt(), _boards()
    look = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5, layers=2)
    assert sorted(look) == sorted(nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 77, 5))
    differs = 0
    for i, key in enumerate(keys.tolist()):
        want = scalar_search_on_host(key, weights(name), TUPLES, symmetric, 1.0, 77, 5, 2)
        assert np.array_equal(bits(look["q"][i]), bits(want["q"])), (i, look["q"][i], want["q"])
        assert int(look["action"][i]) == want["action"] and int(look["candidates"][i]) == want["candidates"], i
        assert np.array_equal(bits(look["terms"][i]), bits(want["terms"])), i
        differs += int(not np.array_equal(look["q"][i], scalar_search_on_host(key, weights(name), TUPLES, symmetric, 1.0, 77, 5, 1)["q"]))
    assert differs >= len(keys) - 4                                        # (the dead board, the board over after every spawn ...)
    names = list(CRAFTED)
    assert int(look["action"][names.index("dead")]) == -1 and int(look["candidates"][names.index("over_after_spawn")]) == 0


def test_the_scalar_definition_at_one_layer_is_the_mirror():
    """the restatement's inner level, held to the mirror as it stood"""
    nt, keys = _nt(), _boards()
    look = nt.search_nt_on_host(keys, weights("seeded"), TUPLES, True, 1.0, 77, 5)
    for i, key in enumerate(keys.tolist()):
        want = scalar_search_on_host(key, weights("seeded"), TUPLES, True, 1.0, 77, 5, 1)
        assert np.array_equal(bits(look["q"][i]), bits(want["q"])) and int(look["action"][i]) == want["action"], i


def test_a_hand_worked_board_on_zero_weights():
    """ONE_MERGE, rows 2 4 2 4 / 4 2 4 2 / 2 4 2 4 / 4 2 8 8, gamma 1, zero weights.  Left makes 4 2 16 . of the last row: reward 4, one
    empty cell (15), so two chance boards.  C(15, 1), a 2-tile under a 4: nothing merges, the game is over, W2 = +0.0.  C(15, 2), a
    4-tile under a 4: up and down are its candidates.  Up makes the column 4 2 8 . (reward 3) and either tile in cell 15 ends the game:
    q_up = 3.  Down makes the column . 4 2 8 (reward 3), rows 2 4 2 . / 4 2 4 4 / 2 4 2 2 / 4 2 16 8, one empty cell (3): a 2-tile there
    merges three rows left or right for 4 + 8 + 4 = 16, reward 4; a 4-tile merges two rows for 12 or the column for 8, reward 3:
    q_down = 3 + (4 P_1 + 3 P_2).  W2 = q_down, term_31 = P_2 * W2, E_0 = term_31 / 1 and q_0 = 4 + P_2 (3 + 4 P_1 + 3 P_2).  Every
    product and sum here is exact in float64 (P_k are multiples of 2^-24 below 1), so the float64 results are float(the rationals)."""
    nt = _nt()
    zero = weights("zero")
    look = nt.search_nt_on_host([ONE_MERGE], zero, TUPLES, True, 1.0, 1, 0, layers=2)
    inner = 3 + 4 * P[0] + 3 * P[1]
    assert int(look["candidates"][0]) == 0b0101 and look["rewards"][0].tolist() == [4, 0, 4, 0]
    assert look["terms"][0, 0, :31].tolist() == [0.0] * 31 and look["terms"][0, 0, 31] == float(P[1] * inner)
    assert look["E"][0, 0] == float(P[1] * inner) and look["q"][0, 0] == float(4 + P[1] * inner)
    assert look["q"][0, 1] == 0.0 and look["q"][0, 3] == 0.0 and not look["terms"][0, 1].any() and not look["terms"][0, 3].any()
    # the two chance boards and the second layer, by the one-layer mirror
    over, four = key_of([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 4, 1]), key_of([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 4, 2])
    below = nt.search_nt_on_host([over, four], zero, TUPLES, True, 1.0, 1, 0)
    assert below["candidates"].tolist() == [0, 0b1010] and below["q"][1].tolist() == [0.0, 3.0, 0.0, float(inner)]
    # right: . 4 2 16, the empty cell is 12; one layer deep E_2 > 3 (tests/test_tfe_nt_search_cpu.py), two layers add the rewards below
    one = nt.search_nt_on_host([ONE_MERGE], zero, TUPLES, True, 1.0, 1, 0, layers=1)
    assert look["q"][0, 2] > one["q"][0, 2] > 7 and np.count_nonzero(look["terms"][0, 2]) == 2 and look["terms"][0, 2, 24:26].all()
    assert one["q"][0, 0] == float(4 + 3 * P[1]) and int(look["action"][0]) == 2


def test_one_layer_is_what_it_was():
    nt, keys = _nt(), _boards()
    assert inspect.signature(nt.search_nt_on_host).parameters["layers"].default == 1
    for name, symmetric in (("zero", True), ("seeded", True), ("seeded", False)):
        plain = nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 9, 4)
        for other in (nt.search_nt_on_host(keys, weights(name), TUPLES, symmetric, 1.0, 9, 4, layers=1),):
            assert sorted(other) == sorted(plain)
            for k in plain:
                assert other[k].dtype == plain[k].dtype and np.array_equal(other[k].view(np.uint8), plain[k].view(np.uint8)), k
    for bad in (0, 3, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="layers must be 1 or 2"):
            nt.search_nt_on_host(keys[:2], weights("zero"), TUPLES, True, 1.0, 9, 4, layers=bad)


def test_gamma_zero_is_the_rewards_at_both_depths():
    nt, keys = _nt(), _boards()
    for layers in (1, 2):
        look = nt.search_nt_on_host(keys, weights("seeded"), TUPLES, True, 0.0, 9, 4, layers=layers)
        cand = look["after"] != keys[:, None]
        assert cand.any() and not cand.all()
        assert np.array_equal(bits(look["q"]), bits(np.where(cand, look["rewards"].astype(np.float64), 0.0)))
        assert np.array_equal(look["action"], nt.greedy_nt_on_host(keys, weights("seeded"), TUPLES, True, 0.0, 9, 4)["action"])


def test_two_layers_add_rewards_on_zero_weights():
    """zero weights, gamma 1: every value below is a sum of rewards, none negative, and the deeper tree adds a layer of them: q at two
    layers >= q at one on every candidate.  (Exact: the sums are of multiples of 2^-48 far below 2^5 and the divisors are the same.)"""
    nt = _nt()
    rng = np.random.default_rng(5)
    nib = (rng.integers(1, 7, (40, 16)) * (rng.random((40, 16)) < .6)).astype(np.uint64)
    keys = np.concatenate([_boards(), (nib << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)])
    one = nt.search_nt_on_host(keys, weights("zero"), TUPLES, True, 1.0, 9, 4)
    two = nt.search_nt_on_host(keys, weights("zero"), TUPLES, True, 1.0, 9, 4, layers=2)
    cand = one["after"] != keys[:, None]
    assert np.array_equal(one["candidates"], two["candidates"]) and (two["q"][cand] >= one["q"][cand]).all()
    assert (two["q"][cand] > one["q"][cand]).sum() > cand.sum() // 2 and not two["q"][~cand].any()


# ------------------------------------------------------------------ the library, without a GPU
def test_library_exports_the_two_deep_entry_points():
    from pulselib_amd import _native
    lib, _ = assert_exports(NAMES, [C.c_void_p, C.c_int32, C.c_void_p], r"int %s\(const %s\* o, int32_t layers, void\* stream\);")
    assert C.sizeof(_native.TfeNtSearch) == 176 and C.sizeof(_native.TfeNtEval) == 208 and lib.pulse_version() == 1


@pytest.mark.parametrize("layers", [1, 2])
def test_search_deep_refuses_what_search_refuses(layers):
    from pulselib_amd import _native
    errors = assert_refusals(_native.lib(), "pulse_tfe_nt_search_deep", functools.partial(opts, _native.TfeNtSearch), SEARCH_CASES, layers)
    assert len(errors) == len(SEARCH_CASES) and all(e.startswith(b"pulse_tfe_nt_search_deep: ") for e in errors)


@pytest.mark.parametrize("layers", [1, 2])
def test_evaluate_search_deep_refuses_what_evaluate_refuses(layers):
    from pulselib_amd import _native
    cases = CASES["pulse_tfe_nt_evaluate"]
    errors = assert_refusals(_native.lib(), "pulse_tfe_nt_evaluate_search_deep", functools.partial(opts, _native.TfeNtEval), cases, layers)
    assert len(errors) == len(cases) and all(e.startswith(b"pulse_tfe_nt_evaluate_search_deep: ") for e in errors)


@pytest.mark.parametrize("layers", [0, 3, -1])
def test_other_depths_are_refused(layers):
    """on structs every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib = _native.lib()
    for name, make in (("pulse_tfe_nt_search_deep", functools.partial(opts, _native.TfeNtSearch)),
                       ("pulse_tfe_nt_evaluate_search_deep", functools.partial(opts, _native.TfeNtEval))):
        rc = getattr(lib, name)(C.byref(make()), layers, None)
        assert rc == -1 and lib.pulse_last_error() == name.encode() + b": layers must be 1 or 2"
        with pytest.raises(ValueError, match="layers must be 1 or 2"):
            _native.check(rc, name)


def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    agent = NTupleTDAfterstateTFEGPU.__new__(NTupleTDAfterstateTFEGPU)        # (no device: the depth is refused before anything is touched)
    for name in ("search", "search_launch", "evaluate_search", "evaluate_search_launch"):
        assert inspect.signature(getattr(NTupleTDAfterstateTFEGPU, name)).parameters["layers"].default == 1
    for layers in (3, 0):
        for call in (lambda: agent.search([0], layers=layers), lambda: agent.search_launch(None, None, None, None, layers=layers),
                     lambda: agent.evaluate_search(layers=layers), lambda: agent.evaluate_search_launch(layers=layers)):
            with pytest.raises(ValueError, match="layers must be 1 or 2"):
                call()
    from tests.tfe_nt_support import assert_init_parameters
    assert_init_parameters(NTupleTDAfterstateTFEGPU)


def test_deep_search_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_search.hip with the Makefile's flags: twelve kernels, the four of two layers among
    them, none with scratch or a spilled vector register.  VGPRs as built: boards 157 (symmetric) / 131, games 191 / 165."""
    assert_no_scratch("ntuple-search-resource-usage", SEARCH_UNIT, 256)
