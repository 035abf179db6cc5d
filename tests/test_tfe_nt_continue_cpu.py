"""The 2048 n-tuple network's games continued across rounds without a GPU: the library's entry point with its
refusals, the pick struct's layout, the host's statement of the pick (continue_pick_on_host) on three games worked by hand and on a
chain of eight rounds of 257 games of 16 moves (tests/tfe_continue_host.py), the Python layer's attributes, and what the compiler
made of the kernel."""
import ctypes as C
import functools
import inspect
import re

import numpy as np
import pytest

from tests.native_args import PTR, assert_refusals, remarks
from tests.native_args import opts as plain_opts
from tests.tfe_continue_host import WORDS, Carried, round_on_host
from tests.tfe_nt_support import CRAFTED, MORE, ROOT, TUPLES, assert_exports, assert_no_scratch, weights
from tests.tfe_nt_support import nt as _nt
from tests.tfe_search_host import key_of

PICK = "pulse_tfe_nt_continue_pick"
FIELDS = ["n_games", "max_steps", "env_seed", "board_id0", "reserved0", "keys", "steps", "lengths", "total_score", "start", "carry_score", "carry_moves", "finished"]
GAMES, MAX_STEPS, EPSILON, ROUNDS = 257, 16, .25, 8                        # 257 games: one full workgroup and one of one lane
ENV_SEED, AGENT_SEED, TIE_SEED, BOARD_ID0 = 11, 12, 13, 1000


# ------------------------------------------------------------------ the export and the pins
def test_library_exports_the_entry_point():
    from pulselib_amd import _native
    lib, text = assert_exports(((PICK, "PulseTfeNtContinuePick"),), [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    assert re.search(r"typedef struct PulseTfeNtContinuePick \{", text)
    s = _native.TfeNtContinuePick
    assert C.sizeof(s) == 96
    assert [f[0] for f in s._fields_] == FIELDS
    assert [getattr(s, f[0]).offset for f in s._fields_] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88]
    assert "static_assert(sizeof(PulseTfeNtContinuePick) == 96" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_continue.hip").read_text()
    # nothing that was there moved: the restart pick's struct, the roll-out's, the version
    assert C.sizeof(_native.TfeNtRestartPick) == 72 and C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
def _pick_opts(**kw):
    from pulselib_amd import _native
    base = dict(n_games=64, max_steps=32, env_seed=3, board_id0=5, **{f: PTR for f in FIELDS[5:]})
    return plain_opts(_native.TfeNtContinuePick, **{**base, **kw})


def test_the_pick_refuses():
    from pulselib_amd import _native
    cases = [(dict(n_games=0), b"n_games must be positive"), (dict(n_games=-4), b"n_games must be positive"),
             (dict(max_steps=1), b"max_steps must be in 2..65535"), (dict(max_steps=0), b"max_steps must be in 2..65535"),
             (dict(max_steps=65536), b"max_steps must be in 2..65535"), (dict(reserved0=1), b"reserved0 must be 0 (zero-initialise the struct)")]
    cases += [(dict([(f, None)]), f.encode() + b" is null") for f in FIELDS[5:]]
    cases += [(dict([(f, PTR + 4)]), b"keys / total_score / start / carry_score / finished must be 8-byte aligned")
              for f in ("keys", "total_score", "start", "carry_score", "finished")]
    cases += [(dict([(f, PTR + 2)]), b"lengths / carry_moves must be 4-byte aligned") for f in ("lengths", "carry_moves")]
    errors = assert_refusals(_native.lib(), PICK, _pick_opts, cases)
    assert len(errors) == len(cases) and [e.split(b": ", 1)[1] for e in errors] == [msg for _, msg in cases]     # message for message
    for max_steps in (2, 65535):                                            # the ends of the range are inside
        assert getattr(_native.lib(), PICK)(C.byref(_pick_opts(max_steps=max_steps, keys=None)), None) == -1
        assert _native.lib().pulse_last_error() == PICK.encode() + b": keys is null"
    assert getattr(_native.lib(), PICK)(C.byref(_pick_opts(steps=PTR + 1, finished=None)), None) == -1     # (bytes: steps has no alignment)
    assert _native.lib().pulse_last_error() == PICK.encode() + b": finished is null"


# ------------------------------------------------------------------ three games by hand
def test_three_games_worked_by_hand():
    """max_steps K = 3, env_seed 11, boards 500 + g; the carries as the launch finds them: (50, 7), (5, 4), (0, 0).
    Game 0 is over after 2 moves (terminal bit) with 100 points: FINISHED with 50 + 100 = 150 points and 7 + 2 = 9 moves, continued
      before.  Its last afterstate is full but for cell 5, so the last spawn fills that cell with a 2 or a 4 and the largest tile stays
      the 4 (nibble 2): bin 2.
    Game 1 played 3 moves, no terminal bit, 40 points: CUT.  The afterstate of move 1 is full -- only the two 8s of its last row merge
      -- so the spawn leaves it as it is: start = that board.  Move 2 went left (action 0): the 8s merge for 16 points, the afterstate
      is the row 4 2 16 . in place of 4 2 8 8.  carry_score = 5 + 40 - 16 = 29, carry_moves = 4 + 2 = 6.
    Game 2 stopped after 1 move with a 32,768 tile in its afterstate, 7,000 points, no terminal bit: FINISHED, 7,000 points, 1 move,
      never continued, stopped at the tile, bin 15.
    finished = games 2, moves 10, score 7,150, squares 150^2 + 7,000^2, max 7,000, continued 1, resumed 1, capped 1; bins 2 and 15."""
    nt = _nt()
    one_empty_5 = key_of(CRAFTED["dead"]) & ~(15 << 20)
    full, after_left, capped = key_of(CRAFTED["one_merge"]), key_of(MORE["one_empty"]), key_of(CRAFTED["tile_32768"])
    keys = np.full((3, 3), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    steps = np.full((3, 3), 0xEE, dtype=np.uint8)
    keys[1, 0], steps[1, 0] = one_empty_5, 0x80 | 1 | 3 << 2
    keys[1, 1], keys[2, 1], steps[2, 1] = full, after_left, 0 | 4 << 2
    keys[0, 2], steps[0, 2] = capped, 2 | 15 << 2
    args = (keys, steps, [2, 3, 1], [100, 40, 7000], 3, 11, 500, [50, 5, 0], [7, 4, 0])
    start, score, moves, words = nt.continue_pick_on_host(*args)
    assert start.dtype == np.uint64 and start.tolist() == [0, full, 0]
    assert score.dtype == np.int64 and score.tolist() == [0, 29, 0] and moves.dtype == np.int32 and moves.tolist() == [0, 6, 0]
    hist = [0] * 16
    hist[2], hist[15] = 1, 1
    assert len(words) == WORDS == 24 and words == [2, 10, 7150, 150 ** 2 + 7000 ** 2, 7000, 1, 1, 1] + hist
    assert nt.FINISHED_SUMMARY == ("games", "moves", "score_sum", "score_sq_sum", "max_score", "continued", "resumed", "tile_capped")
    summary = nt.finished_summary_on_host(words)
    assert summary["games"] == 2 and summary["continued"] == 1 and summary["resumed"] == 1 and summary["tile_capped"] == 1
    assert summary["mean_score"] == 3575.0 and summary["mean_length"] == 5.0 and summary["max_tile_hist"] == hist
    assert nt.add_finished_on_host(words, words) == [4, 20, 14300, 2 * (150 ** 2 + 7000 ** 2), 7000, 2, 2, 2] + [2 * x for x in hist]
    # a length beyond the rows is clamped to them; a terminal bit or a 32,768 tile at move K itself finishes the game all the same
    again = nt.continue_pick_on_host(keys, steps, [2, 9, 1], *args[3:])
    assert again[0].tolist() == [0, full, 0] and again[3] == words
    steps[2, 1] |= 0x80
    start, score, moves, over = nt.continue_pick_on_host(*args)
    assert start.tolist() == [0, 0, 0] and not score.any() and not moves.any() and over[:3] == [3, 17, 7195] and over[5:8] == [0, 2, 1]
    steps[2, 1] &= 0x7F
    keys[2, 1] = capped
    start, _, _, stopped = nt.continue_pick_on_host(*args)
    assert start.tolist() == [0, 0, 0] and stopped[:3] == [3, 17, 7195] and stopped[5:8] == [0, 2, 2] and stopped[8 + 15] == 2
    # the mirror asserts what the device does not check: the cut move made again gives the recorded afterstate
    keys[2, 1] = full
    with pytest.raises(AssertionError, match="does not give the recorded afterstate"):
        nt.continue_pick_on_host(*args)
    with pytest.raises(ValueError, match="max_steps must be in 2..65535"):
        nt.continue_pick_on_host(keys[:1], steps[:1], [1, 1, 1], [0, 0, 0], 1, 11, 500, [0, 0, 0], [0, 0, 0])


# ------------------------------------------------------------------ the host chain at its smallest useful shape
@functools.lru_cache(maxsize=None)
def _chain():
    """eight rounds of 257 games of 16 moves at epsilon .25 on the seeded weights, round r on the boards 1000 + 257 r and the tie
    coins of round r; pick_on_host asserts on every round what the test's docstring lists"""
    c, rounds = Carried(GAMES), []
    for r in range(ROUNDS):
        games, words, cut = round_on_host(c, GAMES, MAX_STEPS, EPSILON, 1.0, weights("seeded"), TUPLES, True, ENV_SEED, AGENT_SEED, TIE_SEED,
                                          BOARD_ID0 + GAMES * r, r)
        rounds.append((games, words, cut, c.start.copy()))
    return rounds, c


def test_eight_rounds_of_continued_games_on_the_host():
    """On every round (tests/tfe_continue_host.py: pick_on_host): the re-made move gives the recorded afterstate, `start` is usable,
    finished plus continued games are the 257, and a finished game's length is the sum of its segments' L - 1 plus its last L, counted
    by the test beside the carries.  Rehearsed: rounds 3 to 7 end 17, 33, 52, 47 and 39 games and cut 240, 224, 205, 210 and 218."""
    rounds, c = _chain()
    ended, cut = [w[0] for _, w, _, _ in rounds], [w[5] for _, w, _, _ in rounds]
    print("ended", ended, "cut", cut, "finished", c.finished)
    assert ended[:2] == [0, 0] and all(e >= 10 and k >= 10 for e, k in zip(ended[3:], cut[3:])) and all(e + k == GAMES for e, k in zip(ended, cut))
    assert ended[3:] == [17, 33, 52, 47, 39]                               # (the mirrors are exact: the rehearsed numbers)
    for r, (games, words, was_cut, start) in enumerate(rounds):
        assert (games["lengths"][was_cut] == MAX_STEPS).all() and np.array_equal(start != 0, was_cut), r
        if r:                                                               # a continued game began on its start board: its first afterstate is a move of it
            began = rounds[r - 1][3]
            after, _ = _nt().moves_on_host(began[began != 0])
            assert (after == games["keys"][0, began != 0][:, None]).any(axis=1).all(), r
    # every finished game had been continued (no game of 2048 ends within 16 moves), and the words add up over the rounds
    assert c.finished[0] == c.finished[6] == sum(ended) and c.finished[5] == sum(cut) and c.finished[7] == 0
    assert c.finished[4] == max(w[4] for _, w, _, _ in rounds) and c.finished[1] > MAX_STEPS * c.finished[0]


# ------------------------------------------------------------------ the Python layer
def test_python_layer(tmp_path):
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    nt = _nt()
    assert Agent.continue_games is False and Agent.eval_max_steps is None
    assert Agent.carry_score is None and Agent.carry_moves is None and Agent.finished is None
    assert Agent.restart_fraction == 0.0 and Agent.start is None            # (what was there stays)
    from tests.tfe_nt_support import assert_init_parameters
    assert_init_parameters(Agent)
    assert list(inspect.signature(Agent.rollout).parameters) == ["self", "layers"] and inspect.signature(Agent.rollout).parameters["layers"].default is None
    assert list(inspect.signature(Agent.learn_batch).parameters) == ["self"]
    assert list(inspect.signature(Agent.restart_pick_launch).parameters) == ["self", "fraction", "min_length"]
    assert list(inspect.signature(Agent.rollout_from_launch).parameters) == ["self", "layers", "backed"]
    assert list(inspect.signature(Agent.evaluate_launch).parameters) == ["self", "n_games", "epsilon", "board_id0", "per_game"]
    assert list(inspect.signature(Agent.continue_pick_launch).parameters) == ["self"]
    assert list(inspect.signature(Agent.finished_summary).parameters) == ["self", "clear"] and inspect.signature(Agent.finished_summary).parameters["clear"].default is True
    assert list(inspect.signature(nt.continue_pick_on_host).parameters) == ["keys", "steps", "lengths", "total_score", "max_steps", "env_seed", "board_id0",
                                                                            "carry_score", "carry_moves"]
    agent = Agent.__new__(Agent)                                           # (no device: refused before anything is touched)
    agent.continue_games, agent.rollout_layers, agent.max_steps = True, 2, 64
    with pytest.raises(ValueError, match="continue_games needs rollout_layers in"):
        agent.rollout()
    with pytest.raises(ValueError, match="continue_games needs rollout_layers in"):
        agent.learn_batch()
    agent.rollout_layers = 0
    with pytest.raises(ValueError, match="continue_games needs rollout_layers in"):
        agent.rollout(layers=2)                                            # the argument is the depth of this launch
    agent.restart_fraction = 0.5
    with pytest.raises(ValueError, match="continue_games does not go with restart_fraction > 0"):
        agent.rollout()
    with pytest.raises(ValueError, match="continue_games does not go with restart_fraction > 0"):
        agent.learn_batch()
    agent.restart_fraction, agent.max_steps = 0.0, 1
    with pytest.raises(ValueError, match="continue_games needs max_steps >= 2"):
        agent.rollout()
    with pytest.raises(ValueError, match="continue_games needs max_steps >= 2"):
        agent.continue_pick_launch()
    with pytest.raises(ValueError, match="holds no finished"):
        agent.finished_summary()
    for bad in (0, 65536, True, 4096.0, "64"):
        agent.eval_max_steps = bad
        with pytest.raises(ValueError, match="eval_max_steps must be None or an int in 1..65535"):
            agent._eval_cap()
    agent.eval_max_steps, agent.max_steps = None, 64
    assert agent._eval_cap() == 64
    agent.eval_max_steps = 4096
    assert agent._eval_cap() == 4096
    # the script refuses --continue-games with --restart, with --train-layers 2 and with --max-steps 1, before it asks for a device
    from pulselib_amd.scripts import tfe_ntuple as script
    for more in (["--restart", "0.5"], ["--train-layers", "2"], ["--max-steps", "1"]):
        with pytest.raises(SystemExit):
            script.main(["--continue-games", "--max-steps", "64"] + more)
    with pytest.raises(ValueError, match="--continue-games does not go with --restart"):
        script.run(None, 1, max_steps=64, restart=0.5, continue_games=True)
    with pytest.raises(ValueError, match="--continue-games does not go with --train-layers 2"):
        script.run(None, 1, max_steps=64, train_layers=2, continue_games=True)
    with pytest.raises(ValueError, match="--continue-games needs --max-steps 2 or more"):
        script.run(None, 1, max_steps=1, continue_games=True)
    assert script.CONTINUE_EVAL_MAX_STEPS == 4096
    # the checkpoint: today's keys and versions, whatever the attributes
    assert nt.CHECKPOINT_SCALARS == ("symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "round", "n_games")
    assert (nt.CHECKPOINT_VERSION, nt.CHECKPOINT_VERSION_LAMBDA, nt.CHECKPOINT_VERSION_TC, nt.CHECKPOINT_VERSION_STAGED) == (1, 2, 4, 5)
    agent.continue_games, agent.eval_max_steps = True, 4096
    agent.tuples, agent.symmetric, agent.gamma, agent.epsilon, agent.alpha, agent.max_steps = ((0,),), True, 1.0, 0.0, 1.0, 64
    agent.seed, agent.board_id0, agent.round, agent.n_games, agent.lam, agent.tc = 0, 0, 3, 8, 0.0, False
    agent.weights = lambda: np.zeros(16, dtype=np.float32)
    agent.save(tmp_path / "net.npz")
    with np.load(tmp_path / "net.npz", allow_pickle=False) as raw:
        assert sorted(raw.files) == sorted(("version", "index", "value", "tuple_len", "tuple_cells") + nt.CHECKPOINT_SCALARS) and int(raw["version"]) == 1
    f = nt.read_checkpoint(tmp_path / "net.npz")
    assert not {"continue_games", "eval_max_steps", "start", "carry_score", "carry_moves", "finished"} & set(f)


# ------------------------------------------------------------------ what the compiler made of the kernel
def test_continue_kernel_uses_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_continue.hip with the Makefile's flags: one kernel, no scratch, no spilled
    vector register.  30 VGPRs as built (occupancy 8); the ceiling is 64, the most at which eight waves still fit a SIMD."""
    names = assert_no_scratch("ntuple-continue-resource-usage", {"tfe_nt_continue_pick_kernel": 1}, 64)
    assert len(names) == 1 and len(re.findall(r"Function Name:", remarks("ntuple-continue-resource-usage"))) == 1
