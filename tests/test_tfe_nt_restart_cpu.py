"""The 2048 n-tuple network's restarted roll-outs without a GPU: the library's two entry points with their
refusals, the pick struct's layout, the host's statement of the spawn and of the pick (spawn_on_host, restart_pick_on_host) against the
oracle's environment and on three games worked by hand, the host's restarted game loop (tests/tfe_nt_host.py), the Python layer's
attributes, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import math
import re

import numpy as np
import pytest

from tests import tfe_host, tfe_nt_host
from tests.native_args import PTR, assert_refusals, remarks, resource_usage
from tests.native_args import opts as plain_opts
from tests.tfe_nt_host import boards_of_keys, nt_games_on_host, usable_on_host
from tests.tfe_nt_support import BOARD_ID0, CASES, CRAFTED, ROOT, TUPLES, assert_exports, assert_no_scratch, play_kernel, play_kernels, bits, opts, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of

FROM, PICK = "pulse_tfe_nt_rollout_from", "pulse_tfe_nt_restart_pick"
GAMES, MAX_STEPS, SEED = 257, 256, 457
LIVE = key_of(CRAFTED["one_merge"])                                        # full; only the two 8s of the last row merge


# ------------------------------------------------------------------ the exports and the pins
def test_library_exports_the_two_entry_points():
    from pulselib_amd import _native
    assert_exports(((FROM, "PulseTfeNtRollout"),), [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
                   r"int %s\(const %s\* o, int32_t layers, double\* backed, uint64_t\* start, void\* stream\);")
    lib, text = assert_exports(((PICK, "PulseTfeNtRestartPick"),), [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    assert re.search(r"typedef struct PulseTfeNtRestartPick \{", text)
    s = _native.TfeNtRestartPick
    assert C.sizeof(s) == 72
    assert [f[0] for f in s._fields_] == ["n_games", "max_steps", "env_seed", "board_id0", "fraction", "min_length", "reserved0", "keys", "lengths", "start",
                                          "picked"]
    assert [getattr(s, f[0]).offset for f in s._fields_] == [0, 4, 8, 16, 24, 32, 36, 40, 48, 56, 64]
    assert "static_assert(sizeof(PulseTfeNtRestartPick) == 72" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_restart.hip").read_text()
    assert C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
@pytest.mark.parametrize("layers,backed", [(0, None), (1, None), pytest.param(1, PTR, id="1-PTR")])     # (PTR is an address: no two runs share it)
def test_the_rollout_refuses_what_the_rollout_refuses(layers, backed):
    from pulselib_amd import _native
    cases, make = CASES["pulse_tfe_nt_rollout"], functools.partial(opts, _native.TfeNtRollout)
    errors = assert_refusals(_native.lib(), FROM, make, cases, layers, backed, PTR)
    plain = assert_refusals(_native.lib(), "pulse_tfe_nt_rollout", make, cases)
    assert len(errors) == len(cases) and all(e.startswith(FROM.encode() + b": ") for e in errors)
    assert [e.split(b": ", 1)[1] for e in errors] == [e.split(b": ", 1)[1] for e in plain]     # the same messages, one copy of the checks


def test_the_rollouts_own_refusals():
    """on a struct every other check passes: nothing is launched"""
    from pulselib_amd import _native
    lib, o = _native.lib(), opts(_native.TfeNtRollout)
    own = [((2, None, PTR), b"layers must be 0 or 1"), ((3, None, PTR), b"layers must be 0 or 1"), ((-1, None, PTR), b"layers must be 0 or 1"),
           ((2, PTR, PTR), b"layers must be 0 or 1"), ((0, PTR, PTR), b"backed needs layers = 1"), ((1, PTR + 4, PTR), b"backed must be 8-byte aligned"),
           ((0, None, None), b"start is null"), ((1, PTR, None), b"start is null"), ((0, None, PTR + 4), b"start must be 8-byte aligned"),
           ((1, None, PTR + 4), b"start must be 8-byte aligned")]
    for args, msg in own:
        assert getattr(lib, FROM)(C.byref(o), *args, None) == -1, args
        assert lib.pulse_last_error().startswith(FROM.encode() + b": " + msg), (args, lib.pulse_last_error())


def _pick_opts(**kw):
    from pulselib_amd import _native
    base = dict(n_games=64, max_steps=32, env_seed=3, board_id0=5, fraction=0.5, min_length=2, keys=PTR, lengths=PTR, start=PTR, picked=PTR)
    return plain_opts(_native.TfeNtRestartPick, **{**base, **kw})


def test_the_pick_refuses():
    from pulselib_amd import _native
    cases = [(dict(n_games=0), b"n_games must be positive"), (dict(max_steps=0), b"max_steps must be in 1..65535"),
             (dict(max_steps=65536), b"max_steps must be in 1..65535")]
    cases += [(dict(fraction=f), b"fraction must be in (0, 1)") for f in (0.0, 1.0, -0.5, math.nan, 1.5)]
    cases += [(dict(min_length=1), b"min_length must be in 2..65535"), (dict(min_length=65536), b"min_length must be in 2..65535"),
              (dict(min_length=-3), b"min_length must be in 2..65535"), (dict(reserved0=1), b"reserved0 must be 0")]
    cases += [(dict([(f, None)]), f.encode() + b" is null") for f in ("keys", "lengths", "start", "picked")]
    cases += [(dict([(f, PTR + 4)]), b"keys / start / picked must be 8-byte aligned") for f in ("keys", "start", "picked")]
    cases += [(dict(lengths=PTR + 2), b"lengths must be 4-byte aligned")]
    errors = assert_refusals(_native.lib(), PICK, _pick_opts, cases)
    assert len(errors) == len(cases)
    for fraction in (5e-324, 1.0 - 2.0 ** -53):                            # the ends of the interval are outside, everything between is inside
        assert getattr(_native.lib(), PICK)(C.byref(_pick_opts(fraction=fraction, keys=None)), None) == -1
        assert _native.lib().pulse_last_error() == PICK.encode() + b": keys is null"
    for min_length in (2, 65535):
        assert getattr(_native.lib(), PICK)(C.byref(_pick_opts(min_length=min_length, keys=None)), None) == -1
        assert _native.lib().pulse_last_error() == PICK.encode() + b": keys is null"


# ------------------------------------------------------------------ the spawn and the pick on the host
@functools.lru_cache(maxsize=None)
def _recorded():
    """a host roll-out of 257 games of at most 256 moves on zero weights at epsilon .25, with the boards before every move kept"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    policy = tfe_nt_host._NTuple(GAMES, .25, SEED ^ AGENT_KEY, SEED ^ TIE_KEY, 0, weights=weights("zero"), tuples=TUPLES, symmetric=True, gamma=1.0)
    return tfe_host._play(policy, GAMES, 4, MAX_STEPS, SEED, BOARD_ID0, keep_boards="before", tile_cap=32768)


def test_spawn_on_host_is_the_oracles_spawn():
    """the board before move t of every game is the afterstate of move t - 1 with the spawn of draw t put into it"""
    nt, rec = _nt(), _recorded()
    ids = np.arange(GAMES, dtype=np.uint64) + np.uint64(BOARD_ID0)
    checked = 0
    for t in range(1, len(rec["boards"])):
        live = np.flatnonzero(rec["lengths"] > t)
        draws = nt.philox_many_on_host(SEED, ids[live], t)
        got = nt.spawn_on_host(rec["keys"][t - 1, live], draws[:, 0], draws[:, 1])
        assert got.dtype == np.uint64 and np.array_equal(got, tfe_host.pack_boards(rec["boards"][t][live])), t
        checked += live.size
    assert checked == int(rec["lengths"].sum()) - GAMES
    # a full board comes back as it is; one empty cell takes the tile whatever the first word; the tile's odds are the second word's
    dead = key_of(CRAFTED["dead"])
    assert nt.spawn_on_host([dead, dead], [0, 2 ** 32 - 1], [0, 2 ** 32 - 1]).tolist() == [dead, dead]
    one_empty = dead & ~(15 << 20)
    assert nt.spawn_on_host([one_empty] * 4, [0, 2 ** 32 - 1, 7, 7], [0, 15099494 << 8 | 255, 15099495 << 8, 2 ** 32 - 1]).tolist() == [
        one_empty | 1 << 20, one_empty | 1 << 20, one_empty | 2 << 20, one_empty | 2 << 20]
    two = 0x1                                                              # fifteen empty cells: k = (r * 15) >> 32 counts them in cell order
    assert nt.spawn_on_host([two, two, two], [0, 2 ** 32 - 1, 2 ** 31], [0, 0, 0]).tolist() == [two | 1 << 4, two | 1 << 60, two | 1 << 32]


def test_the_pick_takes_the_board_move_t_star_was_made_on():
    nt, rec = _nt(), _recorded()
    L = rec["lengths"].astype(np.int64)
    fraction, min_length = 0.5, int(np.median(L))
    at = np.floor(L * fraction).astype(np.int64)
    want = (L >= min_length) & (at >= 1) & (at <= L - 1)
    assert 8 <= int(want.sum()) <= GAMES - 8 and int((L < min_length).sum()) >= 8, (int(want.sum()), min_length)     # both kinds occur
    start, picked = nt.restart_pick_on_host(rec["keys"], rec["lengths"], MAX_STEPS, SEED, BOARD_ID0, fraction, min_length)
    assert start.dtype == np.uint64 and start.shape == (GAMES,) and np.array_equal(start != 0, want)
    for g in np.flatnonzero(want).tolist():
        assert int(start[g]) == int(tfe_host.pack_boards(rec["boards"][at[g]][g:g + 1])[0]), g
    assert picked == (int(want.sum()), int(at[want].sum()))
    assert usable_on_host(start[want]).all()                               # boards a game stood on and moved on
    # trimmed to the longest game, the records give the same; max_steps clamps a length beyond the rows
    T = int(L.max())
    again, _ = nt.restart_pick_on_host(rec["keys"][:T], rec["lengths"] + np.where(L == MAX_STEPS, 9, 0), MAX_STEPS, SEED, BOARD_ID0, fraction, min_length)
    assert np.array_equal(again, start)
    # another fraction picks other boards, nearer the end
    late, late_picked = nt.restart_pick_on_host(rec["keys"], rec["lengths"], MAX_STEPS, SEED, BOARD_ID0, 0.9, min_length)
    assert np.array_equal(late != 0, want) and late_picked[1] > picked[1] and not np.array_equal(late, start)


def test_three_games_worked_by_hand():
    """fraction .25, min_length 4.  Game 0 has 9 moves: t* = floor(2.25) = 2, the board move 2 was made on is the afterstate of move
    1 -- full but for cell 5 -- with the spawn of draw 2: the one empty cell takes the tile, a 2 or a 4 by word y.  Game 1 has 3 moves:
    too short.  Game 2 has 3 moves too, and at min_length 2 it is long enough, but t* = floor(.75) = 0: a game is not restarted from its
    own start.  Picked: one board, depth 2."""
    from pulselib_amd.agents.tfe_common import philox4x32
    nt = _nt()
    after = key_of(CRAFTED["dead"]) & ~(15 << 20)
    keys = np.full((9, 3), 0x21, dtype=np.uint64)
    keys[1, 0] = after
    word_y = philox4x32(11, 500 + 0, 2)[1]
    tile = 2 if (word_y >> 8) > 15099494 else 1
    start, picked = nt.restart_pick_on_host(keys, [9, 3, 3], 9, 11, 500, 0.25, 4)
    assert start.tolist() == [after | tile << 20, 0, 0] and picked == (1, 2)
    start, picked = nt.restart_pick_on_host(keys, [9, 3, 3], 9, 11, 500, 0.25, 2)
    assert start.tolist() == [after | tile << 20, 0, 0] and picked == (1, 2)          # games 1 and 2: L * fraction < 1
    start, picked = nt.restart_pick_on_host(keys, [9, 3, 4], 9, 11, 500, 0.25, 2)       # four moves: t* = 1, the board after move 0's spawn
    assert picked == (2, 3) and int(start[2]) == int(nt.spawn_on_host([0x21], *philox4x32(11, 502, 1)[:2])[0]) != 0x21
    assert nt.restart_summary_on_host([2, 3], start) == dict(picked=2, mean_depth=1.5, started=2)
    assert nt.restart_summary_on_host([0, 0], np.zeros(3, dtype=np.uint64)) == dict(picked=0, mean_depth=0.0, started=0)


# ------------------------------------------------------------------ the host's restarted game loop
def _args(n_games, max_steps, epsilon=.25, name="seeded"):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return (n_games, max_steps, epsilon, 1.0, weights(name), TUPLES, True, 2312, 2312 ^ AGENT_KEY, 2312 ^ TIE_KEY, BOARD_ID0, 0)


def test_a_start_of_zeros_gives_the_plain_games():
    args = _args(5, 24)
    got = nt_games_on_host(*args, start=np.zeros(5, dtype=np.uint64))
    want, start = nt_games_on_host(*args), got["start_left"]
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward", "final_boards"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(bits(got["values"]), bits(want["values"])) and not start.any()


def test_only_a_usable_board_starts_a_game():
    """a dead board (full, no equal neighbours), a board with nibble 15, a zero and a live board: three reset games and one from the
    live board"""
    dead, capped = key_of(CRAFTED["dead"]), key_of(CRAFTED["tile_32768"])
    given = np.array([dead, capped, 0, LIVE], dtype=np.uint64)
    assert usable_on_host(given).tolist() == [False, False, False, True]
    assert usable_on_host([key_of(CRAFTED["makes_32768"]), key_of(CRAFTED["corner"]), key_of(CRAFTED["over_after_spawn"])]).tolist() == [False, True, False]
    assert boards_of_keys([LIVE])[0].ravel().tolist() == [2, 4, 2, 4, 4, 2, 4, 2, 2, 4, 2, 4, 4, 2, 8, 8]
    args = _args(4, 24, epsilon=0.0)                                       # greedy: the live board's first move is one that changes it
    got = nt_games_on_host(*args, start=given)
    want, start = nt_games_on_host(*args), got["start_left"]
    assert start.tolist() == [0, 0, 0, LIVE] and np.count_nonzero(start) == 1
    for k in ("keys", "steps", "lengths", "total_score", "episode_reward"):
        assert np.array_equal(got[k][..., :3], want[k][..., :3]), k     # the three reset games
    # the game from the live board: its first move is one of the two that change it (left or right merge the 8s for 16 points)
    assert int(got["steps"][0, 3]) & 3 in (0, 2) and (int(got["steps"][0, 3]) >> 2) & 31 == 4 and int(got["keys"][0, 3]) != int(want["keys"][0, 3])
    assert int(got["total_score"][3]) >= 16 and int(got["lengths"][3]) >= 1
    # under the search, with and without the backed value, the same rule
    for backed in (False, True):
        searched = nt_games_on_host(*_args(4, 6, epsilon=0.0), depth=1, backed=backed, start=given)
        assert searched["start_left"].tolist() == [0, 0, 0, LIVE] and ("backed" in searched) == backed and (int(searched["steps"][0, 3]) >> 2) & 31 == 4


# ------------------------------------------------------------------ the Python layer
def test_python_layer(tmp_path):
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    nt = _nt()
    assert Agent.restart_fraction == 0.0 and Agent.restart_min_length == 64 and Agent.start is None and Agent.restart_stats is None
    from tests.tfe_nt_support import assert_init_parameters
    assert_init_parameters(Agent)
    assert list(inspect.signature(Agent.rollout).parameters) == ["self", "layers"] and inspect.signature(Agent.rollout).parameters["layers"].default is None
    assert list(inspect.signature(Agent.learn_batch).parameters) == ["self"]
    assert list(inspect.signature(Agent.restart_pick_launch).parameters) == ["self", "fraction", "min_length"]
    assert list(inspect.signature(Agent.rollout_from_launch).parameters) == ["self", "layers", "backed"]
    assert callable(Agent.restart_summary)
    assert list(inspect.signature(nt.spawn_on_host).parameters) == ["keys", "r_cell", "r_val"]
    assert list(inspect.signature(nt.restart_pick_on_host).parameters) == ["keys", "lengths", "max_steps", "env_seed", "board_id0", "fraction", "min_length"]
    agent = Agent.__new__(Agent)                                           # (no device: refused before anything is touched)
    agent.restart_fraction, agent.rollout_layers = 0.5, 2
    with pytest.raises(ValueError, match="restart_fraction > 0 needs rollout_layers in"):
        agent.rollout()
    with pytest.raises(ValueError, match="restart_fraction > 0 needs rollout_layers in"):
        agent.learn_batch()
    agent.rollout_layers = 0
    with pytest.raises(ValueError, match="restart_fraction > 0 needs rollout_layers in"):
        agent.rollout(layers=2)                                            # the argument is the depth of this launch
    for bad in (1.0, -0.25, math.nan, 1.5):
        agent.restart_fraction = bad
        with pytest.raises(ValueError, match="restart_fraction must be 0"):
            agent.rollout()
        with pytest.raises(ValueError, match="restart_fraction must be 0"):
            agent.restart_pick_launch()
    agent.restart_fraction = 0.0
    with pytest.raises(ValueError, match="the pick needs a fraction"):
        agent.restart_pick_launch()
    with pytest.raises(ValueError, match="holds no start"):
        agent.restart_summary()
    for bad in (2, True, -1):
        with pytest.raises(ValueError, match="layers must be 0 or 1"):
            agent.rollout_from_launch(bad)
    with pytest.raises(ValueError, match="backed needs layers = 1"):
        agent.rollout_from_launch(0, backed=True)
    # the script refuses --restart with --train-layers 2, before it asks for a device
    from pulselib_amd.scripts import tfe_ntuple as script
    with pytest.raises(SystemExit):
        script.main(["--restart", "0.5", "--train-layers", "2"])
    with pytest.raises(ValueError, match="--restart does not go with --train-layers 2"):
        script.run(None, 1, train_layers=2, restart=0.5)
    # the checkpoint: today's keys and versions, whatever the attributes
    assert nt.CHECKPOINT_SCALARS == ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")
    assert (nt.CHECKPOINT_VERSION, nt.CHECKPOINT_VERSION_LAMBDA, nt.CHECKPOINT_VERSION_TC) == (1, 2, 4)
    agent.restart_fraction, agent.restart_min_length = 0.5, 32
    agent.tuples, agent.symmetric, agent.gamma, agent.epsilon, agent.alpha, agent.max_steps = ((0,),), True, 1.0, 0.0, 1.0, 64
    agent.seed, agent.board_id0, agent.round, agent.n_games, agent.lam, agent.tc = 0, 0, 3, 8, 0.0, False
    agent.weights = lambda: np.zeros(16, dtype=np.float32)
    agent.save(tmp_path / "net.npz")
    with np.load(tmp_path / "net.npz", allow_pickle=False) as raw:
        assert sorted(raw.files) == sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS) and int(raw["version"]) == 1
    f = nt.read_checkpoint(tmp_path / "net.npz")
    assert "restart_fraction" not in f and "restart_min_length" not in f and "start" not in f


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_restart_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_restart.hip with the Makefile's flags: the six game kernels and the pick, none
    with scratch or a spilled vector register.  The ceiling of a mapping is its sibling's count in profiles/tfe_mc/kernel_resource_usage.txt
    (one ply 117 symmetric / 61; one layer 158 / 133; one layer with the backed value 160 / 135) plus four: the start word and its
    address, two registers each.  VGPRs as built: one ply 117 / 61, one layer 159 / 133, with the backed value 161 / 135, the pick 16."""
    names = assert_no_scratch("ntuple-restart-resource-usage",
                              {**play_kernels(1, True, start=True), **play_kernels(32, True, start=True), **play_kernels(32, True, backed=True, start=True),
                               "tfe_nt_restart_pick_kernel": 1}, 160 + 4)
    assert len(re.findall(r"Function Name:", remarks("ntuple-restart-resource-usage"))) == 7
    ceiling = {play_kernel(1, 8, True, start=True): 117, play_kernel(1, 1, True, start=True): 61,
               play_kernel(32, 8, True, start=True): 158, play_kernel(32, 1, True, start=True): 133,
               play_kernel(32, 8, True, backed=True, start=True): 160, play_kernel(32, 1, True, backed=True, start=True): 135, "restart_pick_kernel": 32 - 4}
    _, vgprs, _, _ = resource_usage("ntuple-restart-resource-usage")
    for name, v in zip(names, vgprs):
        key = [k for k in ceiling if k in name]
        assert len(key) == 1 and v <= ceiling[key[0]] + 4, (name, v)
