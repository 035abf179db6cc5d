"""The 2048 n-tuple network's training roll-out under expectimax search without a GPU: the library's new entry
point with its refusals, the Python layer's depth check, the host's statement of the recording games (tests/tfe_nt_host.py)
against the evaluation's games and against the one-ply roll-out, one board worked by hand, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
from fractions import Fraction

import numpy as np
import pytest

from tests.native_args import assert_refusals
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import BOARD_ID0, CASES, CRAFTED, P, ROLLOUT_UNIT, TUPLES, assert_exports, assert_no_scratch, bits, opts, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of

NAME = "pulse_tfe_nt_rollout_search"
GAMES, MAX_STEPS, EPSILON, SEED, ROUND = 17, 192, .25, 2312, 0           # the shape of tests/test_tfe_nt_search_gpu.py


def _seeds():
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, BOARD_ID0, ROUND


# ------------------------------------------------------------------ the library, without a GPU
def test_library_exports_the_entry_point():
    from pulselib_amd import _native
    lib, _ = assert_exports(((NAME, "PulseTfeNtRollout"),), [C.c_void_p, C.c_int32, C.c_void_p], r"int %s\(const %s\* o, int32_t layers, void\* stream\);")
    assert C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1


@pytest.mark.parametrize("layers", [1, 2])
def test_it_refuses_what_the_rollout_refuses(layers):
    from pulselib_amd import _native
    cases = CASES["pulse_tfe_nt_rollout"]
    errors = assert_refusals(_native.lib(), NAME, functools.partial(opts, _native.TfeNtRollout), cases, layers)
    plain = assert_refusals(_native.lib(), "pulse_tfe_nt_rollout", functools.partial(opts, _native.TfeNtRollout), cases)
    assert len(errors) == len(cases) and all(e.startswith(NAME.encode() + b": ") for e in errors)
    assert [e.split(b": ", 1)[1] for e in errors] == [e.split(b": ", 1)[1] for e in plain]     # the same messages, one copy of the checks


@pytest.mark.parametrize("layers", [0, 3, -1])
def test_other_depths_are_refused(layers):
    """on a struct every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib = _native.lib()
    rc = getattr(lib, NAME)(C.byref(opts(_native.TfeNtRollout)), layers, None)
    assert rc == -1 and lib.pulse_last_error() == NAME.encode() + b": layers must be 1 or 2"
    with pytest.raises(ValueError, match="layers must be 1 or 2"):
        _native.check(rc, NAME)


def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    nt = _nt()
    assert [nt.check_rollout_layers(x) for x in (0, 1, 2)] == [0, 1, 2] and type(nt.check_rollout_layers(np.int64(2))) is int
    for bad in (True, 3, -1, 1.5, None):
        with pytest.raises(ValueError):
            nt.check_rollout_layers(bad)
    assert inspect.signature(NTupleTDAfterstateTFEGPU.rollout).parameters["layers"].default is None
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.rollout_search_launch).parameters) == ["self", "layers"]
    assert list(inspect.signature(NTupleTDAfterstateTFEGPU.learn_batch).parameters) == ["self"]
    from tests.tfe_nt_support import assert_init_parameters
    assert_init_parameters(NTupleTDAfterstateTFEGPU)
    agent = NTupleTDAfterstateTFEGPU.__new__(NTupleTDAfterstateTFEGPU)        # (no device: the depth is refused before anything is touched)
    assert agent.rollout_layers == 0
    for bad in (3, True, -1):
        with pytest.raises(ValueError):
            agent.rollout(layers=bad)
        agent.rollout_layers = bad                                         # the attribute is checked at the launch
        with pytest.raises(ValueError):
            agent.rollout()
    for bad in (0, 3, True):
        with pytest.raises(ValueError, match="layers must be 1 or 2"):
            agent.rollout_search_launch(bad)
    assert nt.CHECKPOINT_SCALARS == ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")


# ------------------------------------------------------------------ the host's statement of the recording games
@functools.lru_cache(maxsize=None)
def _recorded(gamma=1.0):
    return nt_games_on_host(GAMES, MAX_STEPS, EPSILON, gamma, weights("seeded"), TUPLES, True, *_seeds(), depth=1)


def test_recording_does_not_change_play():
    got = _recorded()
    want = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, 1.0, weights("seeded"), TUPLES, True, *_seeds(), depth=1, record=False)
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward", "final_boards"):
        assert np.array_equal(got[k], want[k]), k
    assert all(got[k] == want[k] for k in ("ended", "truncated", "capped", "greedy")) and "values" not in want
    assert want["ended"] >= 2 and want["truncated"] >= 2 and 0 < want["greedy"] < int(want["lengths"].sum())


def test_the_recorded_values_are_the_networks():
    nt, got = _nt(), _recorded()
    played = np.arange(MAX_STEPS)[:, None] < got["lengths"][None, :]
    want = nt.value_on_host(got["keys"][played], weights("seeded"), TUPLES, True)
    assert got["values"].dtype == np.float64 and np.array_equal(bits(got["values"][played]), bits(want))
    assert np.unique(want).size > played.sum() // 2 and not got["values"][~played].any()
    # ... and not the search's: on the first boards, q of the chosen move is another number
    from tests.tfe_host import pack_boards
    first = nt_games_on_host(GAMES, 1, 0.0, 1.0, weights("seeded"), TUPLES, True, *_seeds(), depth=1, record=False, keep_boards="before")
    look = nt.search_nt_on_host(pack_boards(first["boards"][0]), weights("seeded"), TUPLES, True, 1.0, _seeds()[2], ROUND)
    q = look["q"][np.arange(GAMES), look["action"]]
    v = nt.value_on_host(look["after"][np.arange(GAMES), look["action"]], weights("seeded"), TUPLES, True)
    assert (q != v + look["rewards"][np.arange(GAMES), look["action"]]).all()


def test_gamma_zero_is_the_one_ply_rollout():
    got = _recorded(0.0)
    want = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, 0.0, weights("seeded"), TUPLES, True, *_seeds())
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["values"]), bits(want["values"])) and want["values"].any() and int(want["lengths"].sum()) > GAMES


# ------------------------------------------------------------------ one board worked by hand
def test_one_board_worked_by_hand():
    """The one tuple (0, 1, 2, 3) without symmetry: V of a board is the weight at the index its first row spells.  ONE_MERGE, rows
    2 4 2 4 / 4 2 4 2 / 2 4 2 4 / 4 2 8 8: its first row has the nibbles 1 2 1 2, index 1 + 2 * 16 + 1 * 256 + 2 * 4096 = 8481; that
    weight is 2.5 and every other is 0, gamma 1, one chance layer.  Left and right are the candidates, both merge the 8s (reward 4) and
    both leave the first row alone: V(B_left) = V(B_right) = 2.5.
    Left, last row 4 2 16 ., empty cell 15.  A 2-tile there ends the game: m = 0.  A 4-tile under the 4 of cell 11: up makes the column
    4 2 8 . (reward 3) and keeps cell 3: 3 + 2.5; down makes . 4 2 8 and empties cell 3, so the first row reads another weight: 3 + 0.
    m = 5.5, E_left = 5.5 P_2 and q_left = 4 + 5.5 P_2.
    Right, last row . 4 2 16, empty cell 12: the columns are now 2 4 2 . / 4 2 4 4 / 2 4 2 2 / 4 2 4 16.  A 2-tile in cell 12: up makes
    2 4 4 . / 4 2 8 . / 2 4 4 . of the first three columns, score 4 + 8 + 4 = 16, reward 4, and keeps the first row: 4 + 2.5; down merges
    the same tiles and empties three cells of the first row: 4 + 0; the last row 2 4 2 16 does not move; m = 6.5.  A 4-tile there, last
    row 4 4 2 16: left and right merge the 4s (reward 3) and keep the first row, up merges the second and third column (score 12,
    reward 3) and keeps it too: 5.5 each; down empties cells of the first row: 3 + 0; m = 5.5.  E_right = 6.5 P_1 + 5.5 P_2 and
    q_right = 4 + 6.5 P_1 + 5.5 P_2, about 10.4: the search moves right, action 2.  (One ply deep the two moves tie at 4 + 2.5.)
    The record: the key of B_right, the value 2.5 -- V of the afterstate from the network, neither q_right nor E_right -- and the byte
    2 | 4 << 2 = 18 without the game-over bit: whichever tile is spawned into cell 12 leaves a move, as worked above."""
    nt = _nt()
    tuples, key = ((0, 1, 2, 3),), key_of(CRAFTED["one_merge"])
    w = np.zeros(16 ** 4, dtype=np.float32)
    w[8481] = 2.5
    look = nt.search_nt_on_host([key], w, tuples, False, 1.0, 1, 0)
    right = key_of(CRAFTED["one_merge"][:12] + [0, 2, 1, 4])
    assert int(look["candidates"][0]) == 0b0101 and look["rewards"][0].tolist() == [4, 0, 4, 0] and int(look["after"][0, 2]) == right
    assert look["q"][0].tolist() == [float(4 + Fraction(11, 2) * P[1]), 0.0, float(4 + Fraction(13, 2) * P[0] + Fraction(11, 2) * P[1]), 0.0]
    assert int(look["action"][0]) == 2
    assert nt.value_on_host(look["after"][0, [0, 2]], w, tuples, False).tolist() == [2.5, 2.5]
    boards0 = (1 << np.array(CRAFTED["one_merge"], dtype=np.int32)).reshape(1, 4, 4)
    got = nt_games_on_host(1, 1, 0.0, 1.0, w, tuples, False, 11, 12, 1, 500, 0, depth=1, boards0=boards0)
    assert got["lengths"].tolist() == [1] and int(got["keys"][0, 0]) == right and got["total_score"].tolist() == [16]
    assert got["values"][0, 0] == 2.5 and int(got["steps"][0, 0]) == 18 and got["ended"] == 0 and got["greedy"] == 1


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_search_rollout_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_search_rollout.hip with the Makefile's flags: twelve kernels, this file's four among
    them, none with scratch or a spilled vector register.  VGPRs as built: one layer 158 (symmetric) / 133, two layers 202 / 175."""
    assert_no_scratch("ntuple-search-rollout-resource-usage", ROLLOUT_UNIT, 256)
