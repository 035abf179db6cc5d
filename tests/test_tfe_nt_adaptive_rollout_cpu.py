"""The 2048 n-tuple network's training roll-out at the adaptive search depth, without a GPU: the library's new
entry point with its refusals in their order, check_options' new rows in the agent's words and in the script's with the two relaxed rows
still firing while the threshold is off, the agent's and the script's refusals on an object without a device, the host's policy of
tests/tfe_nt_host.py with and without its records, against the searches it composes and against the two-layer roll-out at E = 16, the
games from `start` as the header of tests/tfe_nt_adaptive_support.py lists them, and what the compiler made of the kernels as profiles/tfe_mc/kernel_resource_usage.txt lists it."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

from tests.native_args import PTR, assert_refusals, resource_usage
from tests.tfe_nt_support import CASES, ROLLOUT_UNIT, ROOT, TUPLES, assert_exports, assert_no_scratch, bits, listed, opts, play_kernel, seeds, weights
from tests.tfe_nt_support import nt as _nt

ENTRY = "pulse_tfe_nt_rollout_adaptive"
ALIGNED = PTR + 8 * 4                                                      # inside native_args' host words, 8-byte aligned


def _rollout_opts(**kw):
    from pulselib_amd import _native
    return opts(_native.TfeNtRollout, **kw)


def _refused(*args):
    """the message `ENTRY`(*args, stream) is refused with, without the entry point's name"""
    from pulselib_amd import _native
    lib = _native.lib()
    assert getattr(lib, ENTRY)(*args, None) == -1
    message = lib.pulse_last_error()
    assert message.startswith(ENTRY.encode() + b": ")
    return message[len(ENTRY) + 2:]


def _said(call):
    try:
        call()
    except ValueError as refused:
        return str(refused)
    return None


# ------------------------------------------------------------------ the library, without a GPU
def test_library_exports_the_entry_point():
    from pulselib_amd import _native
    lib, text = assert_exports([(ENTRY, "PulseTfeNtRollout")], [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                               r"int %s\(const %s\* o, int32_t deep_empty_max, double\* backed, uint64_t\* start,\s+int64_t\* depth_stats, void\* stream\);")
    assert C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1
    at = text.index("int " + ENTRY)
    assert text.index("int pulse_tfe_nt_rollout_from(") < at < text.index("int pulse_tfe_nt_rollout_staged(")
    comment = text[text.rindex("/* ----", 0, at):at]
    for words in ("n <= deep_empty_max", "NETWORK's V", "never zeroed", "deep_empty_max must be in", "in this order", "backed:", "start:", "depth_stats:"):
        assert words in comment, words
    unit = (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_search_device.h").read_text()          # ... of which the one game kernel's 256-lane branch:
    unit = unit[unit.index("static_assert(LANES == kSearchBlock"):unit.index("int launch_play(")]
    assert "play_game<Record, Backed, From>" in unit and "search_q_adaptive<IMG>" in unit and "values4<IMG>" in unit
    assert unit.index("values4<IMG>") < unit.index("search_q_adaptive<IMG>(net")         # V of the afterstates before the search starts


def test_the_refusals_come_in_the_stated_order():
    """null options; the threshold; depth_stats, backed, start off their alignment; then the struct's: each case breaks every later rule too"""
    bad, odd = C.byref(_rollout_opts(n_games=0)), 4
    from pulselib_amd import _native
    lib = _native.lib()
    assert getattr(lib, ENTRY)(None, 17, odd, odd, odd, None) == -1 and lib.pulse_last_error() == ENTRY.encode() + b": options are null"
    for E in (-1, 17):
        assert _refused(bad, E, odd, odd, odd) == b"deep_empty_max must be in 0..16"
        assert _refused(C.byref(_rollout_opts()), E, None, None, None) == b"deep_empty_max must be in 0..16"
    assert _refused(bad, 3, odd, odd, odd) == b"depth_stats must be 8-byte aligned"
    assert _refused(bad, 3, odd, odd, ALIGNED) == b"backed must be 8-byte aligned"
    assert _refused(bad, 3, ALIGNED, odd, None) == b"start must be 8-byte aligned"
    assert _refused(bad, 3, ALIGNED, ALIGNED, ALIGNED) == b"n_games must be positive"
    with pytest.raises(ValueError, match=re.escape("deep_empty_max must be in 0..16")):
        _native.check(getattr(lib, ENTRY)(C.byref(_rollout_opts()), 17, None, None, None, None), ENTRY)
    # each misaligned pointer alone, on a struct every check passes
    good = C.byref(_rollout_opts())
    assert _refused(good, 0, None, None, odd) == b"depth_stats must be 8-byte aligned"
    assert _refused(good, 16, odd, None, None) == b"backed must be 8-byte aligned"
    assert _refused(good, 16, None, odd, None) == b"start must be 8-byte aligned"


@pytest.mark.parametrize("E,backed,start,stats", [(0, None, None, None), (16, ALIGNED, ALIGNED, ALIGNED), (3, None, ALIGNED, ALIGNED), (3, ALIGNED, None, ALIGNED),
                                                   (3, ALIGNED, ALIGNED, None)], ids=["all-null", "all-set", "no-backed", "no-start", "no-stats"])
def test_it_refuses_what_the_rollout_refuses(E, backed, start, stats):
    """a threshold at either end and a NULL of each of the three pointers pass their checks: the struct's refusals, which come after
    them, are reached"""
    from pulselib_amd import _native
    cases = CASES["pulse_tfe_nt_rollout"]
    errors = assert_refusals(_native.lib(), ENTRY, _rollout_opts, cases, E, backed, start, stats)
    assert len(errors) == len(cases) and all(e.startswith(ENTRY.encode() + b": ") for e in errors)


# ------------------------------------------------------------------ which options go together
NEEDS_TWO = ("rollout_deep_empty_max needs rollout_layers = 2", "--train-deep-empty-max needs --train-layers 2")
NO_STAGES = ("rollout_deep_empty_max on an agent with stage_tiles", "--train-deep-empty-max does not go with --stages / --add-stage")
RELAXED = ((dict(depth=2, continue_games=True, max_steps=16), "continue_games needs rollout_layers in (0, 1)", "--continue-games does not go with --train-layers 2"),
           (dict(depth=2, restart_fraction=0.5), "restart_fraction > 0 needs rollout_layers in (0, 1)", "--restart does not go with --train-layers 2"))


def test_check_options_new_rows_in_both_vocabularies():
    nt = _nt()
    p = inspect.signature(nt.check_options).parameters
    assert p["rollout_deep_empty_max"].kind is inspect.Parameter.KEYWORD_ONLY and p["rollout_deep_empty_max"].default is None
    for depth in (0, 1):
        for kw in (dict(), dict(backed_targets=bool(depth)), dict(continue_games=True, max_steps=16), dict(restart_fraction=0.5), dict(staged=True)):
            for script, want in enumerate(NEEDS_TWO):
                said = _said(lambda: nt.check_options(depth, rollout_deep_empty_max=3, script=bool(script), **kw))
                assert said is not None and said.startswith(want) and ": " in said, (depth, kw, said)
    for script, want in enumerate(NO_STAGES):
        assert _said(lambda: nt.check_options(2, staged=True, rollout_deep_empty_max=3, script=bool(script))).startswith(want)
    # what the threshold goes with, the return value still the 4-tuple
    assert nt.check_options(2, rollout_deep_empty_max=0) == (2, False, 0, None)
    assert nt.check_options(2, True, 0.0, True, 16, rollout_deep_empty_max=3) == (2, True, 0, None)
    assert nt.check_options(2, True, 0.5, rollout_deep_empty_max=np.int64(16), script=True) == (2, True, 0, None)
    assert nt.check_options(2, rollout_deep_empty_max=3, search=True, layers=2, deep_empty_max=5) == (2, False, 2, 5)
    # the other rules hold beside it, and a bad threshold is check_deep_empty_max's
    assert _said(lambda: nt.check_options(2, False, 0.5, True, 16, rollout_deep_empty_max=3)).startswith("continue_games does not go with restart_fraction > 0")
    assert _said(lambda: nt.check_options(2, continue_games=True, max_steps=1, rollout_deep_empty_max=3)).startswith("continue_games needs max_steps >= 2")
    for bad in (True, -1, 17, 3.0, "3"):
        with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
            nt.check_options(2, rollout_deep_empty_max=bad)


def test_the_relaxed_rows_still_fire_with_the_threshold_off():
    nt = _nt()
    for kw, mine, flags in RELAXED:
        for extra in (dict(), dict(rollout_deep_empty_max=None)):
            assert _said(lambda: nt.check_options(**kw, **extra)).startswith(mine) and _said(lambda: nt.check_options(**kw, **extra, script=True)).startswith(flags)
        assert nt.check_options(**kw, rollout_deep_empty_max=3)[:2] == (2, True)


# ------------------------------------------------------------------ Python and the script
def test_the_agent_refuses_before_anything_is_touched():
    """on an object without a device: a refused round raises check_options' words, an accepted one goes on to buffers it has not got"""
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    nt = _nt()
    assert Agent.rollout_deep_empty_max is None and Agent.depth_stats is None
    assert list(inspect.signature(Agent.rollout_adaptive_launch).parameters) == ["self", "deep_empty_max", "backed", "from_start"]
    assert inspect.signature(Agent.rollout_depth_summary).parameters["clear"].default is True
    for name in ("rollout_deep_empty_max", "rollout_adaptive_launch", "pulse_tfe_nt_rollout_adaptive", "13.13"):
        assert name in Agent.__doc__ + nt.__doc__, name
    agent = Agent.__new__(Agent)
    agent.max_steps, agent.stage_tiles = 16, ()
    rounds = ((dict(rollout_layers=1, rollout_deep_empty_max=3), NEEDS_TWO[0]), (dict(rollout_layers=0, rollout_deep_empty_max=0), NEEDS_TWO[0]),
              (dict(rollout_layers=2, rollout_deep_empty_max=3, stage_tiles=(8,)), NO_STAGES[0]),
              (dict(rollout_layers=2, rollout_deep_empty_max=17), "deep_empty_max must be None or an int in 0..16"),
              (dict(rollout_layers=2, rollout_deep_empty_max=True), "deep_empty_max must be None or an int in 0..16"),
              (dict(rollout_layers=2, rollout_deep_empty_max=None, continue_games=True), RELAXED[0][1]),
              (dict(rollout_layers=2, rollout_deep_empty_max=None, restart_fraction=0.5), RELAXED[1][1]),
              (dict(rollout_layers=2, rollout_deep_empty_max=3), None), (dict(rollout_layers=2, rollout_deep_empty_max=3, continue_games=True), None),
              (dict(rollout_layers=2, rollout_deep_empty_max=3, restart_fraction=0.5, backed_targets=True), None))
    for attributes, want in rounds:
        a = Agent.__new__(Agent)
        vars(a).update({**dict(max_steps=16, stage_tiles=()), **attributes})
        for call in (a.rollout, a.learn_batch):
            if want is None:
                with pytest.raises(AttributeError):
                    call()
            else:
                assert _said(call).startswith(want), attributes
        assert vars(a).keys() == {"max_steps", "stage_tiles"} | set(attributes)
    for bad in (None, True, -1, 17):
        with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
            agent.rollout_adaptive_launch(bad)
    with pytest.raises(ValueError, match="holds no depth_stats"):
        agent.rollout_depth_summary()


def test_the_script_says_the_functions_words(capsys):
    from pulselib_amd.scripts import tfe_ntuple as script
    nt = _nt()
    assert inspect.signature(script.run).parameters["train_deep_empty_max"].default is None and "--train-deep-empty-max" in script.__doc__
    for kw, argv in ((dict(train_layers=1, train_deep_empty_max=3), ["--train-layers", "1", "--train-deep-empty-max", "3"]),
                     (dict(train_deep_empty_max=3), ["--train-deep-empty-max", "3"]),
                     (dict(train_layers=2, train_deep_empty_max=3, stages=(512,)), ["--train-layers", "2", "--train-deep-empty-max", "3", "--stages", "512"]),
                     (dict(train_layers=2, continue_games=True, max_steps=16), ["--train-layers", "2", "--continue-games", "--max-steps", "16"]),
                     (dict(train_layers=2, restart=0.5), ["--train-layers", "2", "--restart", "0.5"])):
        want = _said(lambda: nt.check_options(kw.get("train_layers", 0), False, kw.get("restart", 0.0), kw.get("continue_games", False), kw.get("max_steps", 4096),
                                              bool(kw.get("stages")), rollout_deep_empty_max=kw.get("train_deep_empty_max"), script=True))
        assert want is not None and _said(lambda: script.run(None, 1, **kw)) == want, kw      # (refused before a device is asked for)
        with pytest.raises(SystemExit) as err:
            script.main(argv)
        assert err.value.code == 2 and want in capsys.readouterr().err, argv
    with pytest.raises(SystemExit) as err:
        script.main(["--train-layers", "2", "--train-deep-empty-max", "17"])
    assert err.value.code == 2 and "--train-deep-empty-max must be in 0..16" in capsys.readouterr().err
    with pytest.raises(ValueError, match=re.escape("deep_empty_max must be None or an int in 0..16")):
        script.run(None, 1, train_layers=2, train_deep_empty_max=True)


# ------------------------------------------------------------------ the host's policy
def test_recording_does_not_change_the_games_the_policy_plays():
    """the policy with its records against the policy without them: 3 games of 48 moves at E = 5 (both depths within the opening),
    every record the two share and the counters; the recorded values and backed values are the mirrors' of the boards before the
    moves; and on those boards the one search per move (search_adaptive_nt_on_host) is, row for row, the split by empty cells
    written out by hand: search_nt_on_host one layer deep on the boards with more than 5 empty cells, two layers deep on the others"""
    from tests.tfe_host import pack_boards
    from tests.tfe_nt_host import nt_games_on_host
    nt, w = _nt(), weights("seeded")
    args = (3, 48, .25, 1.0, w, TUPLES, True, *seeds(7))
    played, recorded = nt_games_on_host(*args, deep_empty_max=5, record=False, keep_boards="before"), nt_games_on_host(*args, deep_empty_max=5, backed=True)
    for k in ("keys", "steps", "moved", "lengths", "total_score", "episode_reward", "final_boards"):
        assert np.array_equal(played[k], recorded[k]), k
    assert all(played[k] == recorded[k] for k in ("ended", "truncated", "capped", "greedy", "deep", "shallow"))
    assert played["deep"] >= 5 and played["shallow"] >= 5 and "values" not in played and "backed" not in nt_games_on_host(*args, deep_empty_max=5)
    for t in (0, 20, 47):
        live = np.flatnonzero(recorded["lengths"] > t)
        keys = pack_boards(played["boards"][t][live])
        look = nt.search_adaptive_nt_on_host(keys, w, TUPLES, True, 1.0, seeds(7)[2], 0, 5)
        assert np.array_equal(bits(recorded["backed"][t, live]), bits(look["backed"])) and look["deep"].dtype == np.bool_
        assert np.array_equal(bits(recorded["values"][t, live]), bits(nt.value_on_host(recorded["keys"][t, live], w, TUPLES, True)))
        deep = nt.count_empty_on_host(keys) <= 5
        assert np.array_equal(deep, look["deep"]), t
        for rows, layers in ((~deep, 1), (deep, 2)):
            split = nt.search_nt_on_host(keys[rows], w, TUPLES, True, 1.0, seeds(7)[2], 0, layers=layers)
            for k in ("action", "after", "rewards"):
                assert split[k].dtype == look[k].dtype and np.array_equal(split[k], look[k][rows]), (t, layers, k)
            assert np.array_equal(bits(split["backed"]), bits(look["backed"][rows])), (t, layers)


def test_sixteen_is_the_two_layer_rollout_on_the_host():
    """3 games of 24 moves: the roll-out at E = 16 (search_adaptive_nt_on_host) equals the one at depth 2 (search_nt_on_host(layers=2)),
    with search_backed_on_host of its q (the roll-out at depth 2 with `backed` keeps it)"""
    from tests.tfe_nt_host import nt_games_on_host
    args = (3, 24, .25, 1.0, weights("seeded"), TUPLES, True, *seeds(7))
    mine, two, backed = nt_games_on_host(*args, deep_empty_max=16, backed=True), nt_games_on_host(*args, depth=2), nt_games_on_host(*args, depth=2, backed=True)
    for k in ("keys", "steps", "lengths", "total_score", "episode_reward"):
        assert np.array_equal(mine[k], two[k]) and np.array_equal(mine[k], backed[k]), k
    assert np.array_equal(bits(mine["values"]), bits(two["values"])) and np.array_equal(bits(mine["backed"]), bits(backed["backed"]))
    assert (mine["deep"], mine["shallow"]) == (int(mine["lengths"].sum()), 0) and mine["backed"].any() and mine["values"].any()


def test_the_games_from_start_are_those_of_the_header():
    """tests/tfe_nt_adaptive_support.py's start boards and the games from them (about 4 s with the case they are taken from)"""
    from tests.tfe_nt_adaptive_support import FROM_REHEARSED, GAMES, UNUSABLE, host_rollout_from, start_boards
    from tests.tfe_nt_host import usable_on_host
    nt, start = _nt(), start_boards()
    usable = usable_on_host(start)
    assert sorted(np.flatnonzero(~usable).tolist()) == sorted(UNUSABLE) and len(start) == GAMES and start[0] == 0
    assert nt.count_empty_on_host(start[usable]).tolist() == [3, 5, 2, 1] and nt.count_empty_on_host(start[[2]]).tolist() == [0]
    assert ((start[5] >> np.uint64(4 * np.arange(16))) & np.uint64(15) == 15).any()
    want = host_rollout_from()
    assert {k: (want[k].tolist() if k == "lengths" else want[k]) for k in FROM_REHEARSED} == FROM_REHEARSED
    assert np.array_equal(want["start_left"], np.where(usable, start, np.uint64(0))) and want["backed"].any()


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_the_kernels_use_no_scratch_and_keep_their_siblings_occupancy():
    """profiles/tfe_mc/kernel_resource_usage.txt's section of the merged csrc/tfe_ntuple_search_rollout.hip: twelve kernels, none with
    scratch or a spilled vector register, each of the eight on NtAdaptiveDev with the waves per SIMD of its two-layer recording sibling
    tfe_nt_play_kernel<256, IMG, true, Backed, false, NtDev> as the file lists it ahead of the section (2); and hipcc --offload-arch=gfx950 on the unit with the Makefile's
    flags gives the section's figures.  VGPRs as built: the sibling's, 202 (symmetric) / 175 and with the backed value 204 / 177; 178 with the backed value and From, not symmetric."""
    text = (ROOT / "profiles" / "tfe_mc" / "kernel_resource_usage.txt").read_text()
    older, _, mine = text.partition("tfe_ntuple_search_rollout.hip (merged)")
    assert len(re.findall(r"Function Name:", mine)) == 12
    target = "ntuple-search-rollout-resource-usage"
    names = assert_no_scratch(target, ROLLOUT_UNIT, 256)
    _, vgprs, _, _ = resource_usage(target)
    for img in (8, 1):
        for backed in (0, 1):
            sibling = play_kernel(256, img, True, bool(backed))
            for start in (0, 1):
                kernel = play_kernel(256, img, True, bool(backed), bool(start), net="NtAdaptiveDev")
                assert listed(mine, kernel, "ScratchSize [bytes/lane]") == 0 and listed(mine, kernel, "VGPRs Spill") == 0, kernel
                assert listed(mine, kernel, "Occupancy [waves/SIMD]") >= listed(older, sibling, "Occupancy [waves/SIMD]") == 2, kernel
                built = vgprs[next(i for i, name in enumerate(names) if kernel in name)]
                assert built == listed(mine, kernel, " VGPRs") <= listed(older, sibling, " VGPRs") + 2, (kernel, built)
