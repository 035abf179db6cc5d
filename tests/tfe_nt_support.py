"""What the 2048 n-tuple network's tests (tests/test_tfe_nt_*.py) share, once each: the network and weights most of them use, the networks
at the ABI's limits and the late boards of the shapes file, the crafted boards, the hand-worked games, the refusal tables with the one struct builder, the export and no-scratch checks of the CPU files, and
for the GPU files the learner regime, the guarded agents and the one device round held to the host (learner_round).  Each test file
keeps what only it uses, its caches and its assertions.  A helper, not a test."""
import ctypes as C
import functools
import math
import re
from fractions import Fraction
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from tests.native_args import PTR, nt_opts, resource_usage
from tests.tfe_gpu_support import PATTERNS, guard, guarded, rollout

ROOT = Path(__file__).resolve().parent.parent
TUPLES = ((0, 1, 2, 3), (4, 5, 6, 8, 9, 10))                              # the 6-tuple gives indices above 2^16 and reads the board's upper word


def nt():
    from pulselib_amd.agents import tfe_ntuple_td_gpu
    return tfe_ntuple_td_gpu


def assert_init_parameters(Agent):
    """The agent's __init__ takes, by position, exactly the parameters it took before the opt-ins that are attributes, ending in `tc`;
    `stage_tiles` is keyword-only with default (); and inspect.signature of the class is __init__'s without `self`: nothing stands
    between the call and __init__.  Returns __init__'s parameters."""
    import inspect
    p = inspect.signature(Agent.__init__).parameters
    positional = [k for k, v in p.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional == ["self", "device", "n_games", "tuples", "symmetric", "gamma", "epsilon", "alpha", "max_steps", "seed", "board_id0", "lam", "tc"]
    assert list(p) == positional + ["stage_tiles"] and p["stage_tiles"].kind is inspect.Parameter.KEYWORD_ONLY and p["stage_tiles"].default == ()
    assert type(Agent) is type and list(inspect.signature(Agent).parameters.values()) == list(p.values())[1:]
    return p


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _weights(name, tuples):
    n = nt().tuple_offsets(tuples)[1]
    w = np.zeros(n, dtype=np.float32) if name == "zero" else (np.random.default_rng(7).standard_normal(n) * 4).astype(np.float32)
    w.setflags(write=False)
    return w


def weights(name, tuples=TUPLES):
    """float32[n_weights] of `tuples`, read-only and made once per (name, tuples): all zero ("zero"), or a seeded normal array of
    scale 4 ("seeded": V of the order of the rewards)"""
    return _weights(name, tuple(tuple(t) for t in tuples))


# The networks of tests/test_tfe_nt_shapes_gpu.py.  "eight": the limit of 8 tuples, of lengths 1, 2, 3, 4 and 5, on descending and
# scattered cells, overlapping, one a diagonal; 1,188,368 weights, no multiple of 256: the apply launch's last workgroup is ragged.
# "one6": the other limit, one tuple of the greatest length, descending, in the board's upper word; 16,777,216 weights.
SHAPES = dict(eight=((15,), (3, 0), (5, 10, 6), (12, 8, 4, 0), (1, 2, 5, 6, 9), (0, 5, 10, 15), (7, 11), (13, 14, 9)),
              one6=((15, 14, 13, 11, 10, 9),),
              default=nt().DEFAULT_TUPLES)


@functools.lru_cache(maxsize=None)
def late_start(n_games, seed):
    """uint64[n_games], read-only: a `start` of boards late in a game.  Games with g % 4 == 3 get 0 (they begin at their reset
    boards); every other game gets nibbles drawn from 6..14 with 5 cells emptied, and games with g % 4 == 1 also two adjacent 14s in
    a row: one move from the 32,768 tile.  Every board that is not 0 is usable: it has empty cells and no nibble 15."""
    rng = np.random.default_rng(seed)
    start = np.zeros(n_games, dtype=np.uint64)
    for g in range(n_games):
        if g % 4 == 3:
            continue
        nib = rng.integers(6, 15, 16)
        nib[rng.choice(16, 5, replace=False)] = 0
        if g % 4 == 1:
            row, col = int(rng.integers(4)), int(rng.integers(3))
            nib[4 * row + col] = nib[4 * row + col + 1] = 14
        start[g] = sum(int(x) << (4 * i) for i, x in enumerate(nib))
    start.setflags(write=False)
    return start


# ------------------------------------------------------------------ boards and games made by hand
P = (Fraction(15099495, 2 ** 24), Fraction(1677721, 2 ** 24))            # the odds of a 2-tile and of a 4-tile, as the kernels round them
CRAFTED = dict(                                                            # lists of nibbles for tfe_search_host.key_of
    worked=[1, 1, 0, 0,                                                    # the row 1 1 . . over a filling no 2- or 4-tile merges with:
            3, 4, 3, 4,                                                    # tests/test_tfe_nt_search_cpu.py works these three out by hand
            4, 3, 4, 3,
            3, 4, 3, 4],
    dead=[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1],
    one_merge=[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 3],            # full; only the two 8s of the last row merge
    over_after_spawn=[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 4, 1],
    corner=[1] + [0] * 15,                                                 # right and down are mirror images: two equal best q on zero weights
    fourteen_empty=[0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],
    tile_32768=[15, 3, 0, 1, 2, 5, 1, 0, 0, 0, 4, 0, 1, 0, 0, 2],
    makes_32768=[15, 14, 14, 3, 0, 1, 2, 0, 0, 0, 0, 0, 13, 13, 0, 1])
MORE = dict(one_empty=[1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 4, 0])   # one_merge after its move to the left: the two-layer files' ninth board


def worked_games():
    """(keys, values, steps, lengths) of two games on the tuple (0, 3), board X = 0x1 in all five moves: game 0 ends at t = 2 (values
    10, 20000, 2; rewards 0, 1, 3), game 1 is cut at length 2 (values 1.5, 7; rewards 2, 2).  tests/test_tfe_nt_cpu.py works the TD(0)
    learner out on them, tests/test_tfe_nt_lambda_cpu.py the lambda-differences."""
    keys = np.full((3, 2), 0x1, dtype=np.uint64)
    values = np.array([[10.0, 1.5], [20000.0, 7.0], [2.0, -99.0]])
    steps = np.array([[0 | 0 << 2, 1 | 2 << 2], [2 | 1 << 2, 3 | 2 << 2], [1 | 3 << 2 | 0x80, 0xEE]], dtype=np.uint8)
    return keys, values, steps, [3, 2]


X, Y, V = 0x1, 0x2002000000002002, 0x3000000000000001
STEP_SIZE = 0.125                                                          # alpha 1 over the 8 features of one symmetric tuple
RHO = 1.375 / 4098.375                                                     # |E| / A of weights 0, 1 and 16 after round 1


def tc_worked():
    """Tuple (0, 3), symmetric (its images read the corner pairs: test_tfe_nt_cpu.py), gamma 1, TD(0), 3 games of up to 3 moves.
    Boards: X = nibble 1 in cell 0 reads the weights 1, 0, 0, 16, 1, 0, 0, 16 (index = first nibble + 16 * second); Y = nibble 2 in all
    four corners reads weight 34 eight times; V = nibble 1 in cell 0 and nibble 3 in cell 15 reads 1, 48, 3, 16, 1, 48, 3, 16.

    Round 1.  Games 0 and 1 are worked_games(), every move on X: game 0 ends at t = 2 (values 10, 20000, 2; rewards 0, 1,
    3), game 1 is cut at length 2 (values 1.5, 7; rewards 2, 2).  Their four learnt differences are 19,991 -> 8,192 (clamped), -19,995 ->
    -8,192 (clamped), -2 and 7.5: as integers d = 536,870,912, -536,870,912, -131,072 and 491,520, so per add sum = 360,448 and
    |d| = 1,074,364,416.  Game 2 is one move on Y that ends the game with value 0: difference 0 - 0 = 0.
      weight 0: 16 adds, sum 4 * 360,448, abs 4 * 1,074,364,416: m = 360,448 / 4 / 65,536 = 1.375, a = 1,074,364,416 / 4 / 65,536 = 4,098.375
      weights 1 and 16: 8 adds each, half those sums: the same m and a
      weight 34: 8 adds of 0: m = 0, a = 0
    On zero state rho = 1: weights 0, 1, 16 become 0.125 * 1.375 = 0.171875 with E = 1.375, A = 4,098.375; weight 34 stays 0 with
    E = A = 0.  Moved 4, rho sum 4 * 2^32.

    Round 2.  Game 0 is one ending move on V with value 2: difference -2, d = -131,072.  Game 1 is one ending move on Y with value -3:
    difference 3, d = 196,608.  Game 2 has length 0.
      weights 1 and 16: 2 adds, m = -2, a = 2: the sign of round 1 turned, rho = 1.375 / 4,098.375 = 11 / 32,787 < 1:
        w = float32(0.171875 + (0.125 * rho) * -2), E = 1.375 - 2 = -0.625, A = 4,100.375
      weight 0: visited in round 1 only: its bits, E = 1.375 and A = 4,098.375 stay
      weight 34: every earlier difference was 0, so A = 0 and rho = 1: m = a = 3, w = 0.375, E = A = 3
      weights 3 and 48: never seen before, rho = 1: m = -2, a = 2, w = -0.25, E = -2, A = 2
    Moved 5, rho sum 3 * 2^32 + 2 * rint(rho * 2^32).
    Returns the two rounds as (keys, values, steps, lengths)."""
    keys = np.full((3, 3), X, dtype=np.uint64)
    keys[0, 2] = Y
    values = np.array([[10.0, 1.5, 0.0], [20000.0, 7.0, -55.0], [2.0, -99.0, -55.0]])
    steps = np.array([[0 | 0 << 2, 1 | 2 << 2, 0x80], [2 | 1 << 2, 3 | 2 << 2, 0xEE], [1 | 3 << 2 | 0x80, 0xEE, 0xEE]], dtype=np.uint8)
    keys2 = np.full((3, 3), X, dtype=np.uint64)
    keys2[0, 0], keys2[0, 1] = V, Y
    values2 = np.full((3, 3), -55.0)
    values2[0, 0], values2[0, 1] = 2.0, -3.0
    steps2 = np.full((3, 3), 0xEE, dtype=np.uint8)
    steps2[0, 0], steps2[0, 1] = 0x80, 0x80 | 1
    return (keys, values, steps, [3, 2, 1]), (keys2, values2, steps2, [1, 1, 0])


def tc_worked_state():
    """What tc_worked's docstring works out: per round (acc [W, 2], acc_abs [W], stats of the learn launch, weights float32[W] after the
    apply, E, A, (moved, rho sum)), W = 256"""
    out = []
    acc, ab = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    acc[0], acc[1], acc[16], acc[34] = (4 * 360448, 16), (2 * 360448, 8), (2 * 360448, 8), (0, 8)
    ab[0], ab[1], ab[16] = 4 * 1074364416, 2 * 1074364416, 2 * 1074364416
    w, E, A = np.zeros(256, dtype=np.float32), np.zeros(256), np.zeros(256)
    w[[0, 1, 16]], E[[0, 1, 16]], A[[0, 1, 16]] = 0.171875, 1.375, 4098.375
    out.append((acc, ab, dict(learnt=5, skipped=1, clamped=2), w, E, A, (4, 4 << 32)))
    acc, ab = np.zeros((256, 2), dtype=np.int64), np.zeros(256, dtype=np.int64)
    for i in (1, 16, 3, 48):
        acc[i], ab[i] = (2 * -131072, 2), 2 * 131072
    acc[34], ab[34] = (8 * 196608, 8), 8 * 196608
    w, E, A = w.copy(), E.copy(), A.copy()
    w[[1, 16]], E[[1, 16]], A[[1, 16]] = np.float32(0.171875 + (0.125 * RHO) * -2.0), -0.625, 4100.375
    w[34], E[34], A[34] = 0.375, 3.0, 3.0
    w[[3, 48]], E[[3, 48]], A[[3, 48]] = -0.25, -2.0, 2.0
    out.append((acc, ab, dict(learnt=2, skipped=0, clamped=0), w, E, A, (5, (3 << 32) + 2 * int(np.rint(np.ldexp(RHO, 32))))))
    return out


# ------------------------------------------------------------------ PULSE_EINVAL before anything is launched
DEFAULTS = dict(n_games=64, max_steps=32, gamma=1.0, epsilon=0.25, lam=0.5, step=1.0 / 16, n_boards=73)
SEARCH_DEFAULTS = dict(tie_seed=5, round=2)                                # of PulseTfeNtSearch alone: the roll-out's and the evaluation's seeds stay 0


def opts(struct, **kw):
    """A `_native` struct of the n-tuple network's entry points that every check passes -- TUPLES, symmetric; PTR in every pointer;
    DEFAULTS in the scalars it has -- then `kw` over it (native_args.nt_opts' keywords)."""
    fields = dict(struct._fields_)
    base = dict(tuples=[list(t) for t in TUPLES], net_n=4, net_symmetric=1, net_weights=PTR)
    base.update((f, PTR) for f, ctype in fields.items() if ctype is C.c_void_p)
    base.update((f, v) for f, v in {**DEFAULTS, **(SEARCH_DEFAULTS if "n_boards" in fields else {})}.items() if f in fields)
    return nt_opts(struct, base, **kw)


def null_and_odd(fields8, fields4=()):
    return [(dict([(f, None)]), f.encode() + b" is null") for f in fields8 + fields4] + \
        [(dict([(f, 4)]), b"8-byte aligned") for f in fields8] + [(dict([(f, 2)]), b"4-byte aligned") for f in fields4]


NET_CASES = [(dict(net_n=3), b"board side n must be 4"), (dict(net_n=5), b"board side n must be 4"),
             (dict(tuples=[], net_n_weights=0), b"n_tuples must be in 1..8"), (dict(net_n_tuples=9), b"n_tuples must be in 1..8"),
             (dict(net_len1=0), b"length must be in 1..6"), (dict(net_len1=7), b"length must be in 1..6"),
             (dict(tuples=[[0, 1, 2, 16]]), b"cell must be in 0..15"), (dict(tuples=[[0, 1, 2, 3], [4, 5, 4]]), b"repeated within a tuple"),
             (dict(net_n_weights=16 ** 4 + 16 ** 6 - 1), b"n_weights must be the sum of 16^len"), (dict(net_n_weights=0), b"n_weights must be the sum"),
             (dict(net_symmetric=2), b"symmetric must be 0 or 1"), (dict(net_symmetric=-1), b"symmetric must be 0 or 1"),
             (dict(net_reserved0=1), b"net.reserved0 must be 0")]
WEIGHTS = [(dict(net_weights=None), b"weights is null"), (dict(net_weights=2), b"weights must be 4-byte aligned")]
GAMMA = [(dict(gamma=-0.01), b"gamma must be in [0, 1]"), (dict(gamma=1.01), b"gamma must be in [0, 1]"), (dict(gamma=math.nan), b"gamma must be in [0, 1]")]
BATCH = [(dict(n_games=0), b"n_games must be positive"), (dict(max_steps=0), b"max_steps must be in 1..65535"),
         (dict(max_steps=65536), b"max_steps must be in 1..65535")] + GAMMA + [(dict(reserved0=1), b"reserved0 must be 0")]
EPSILON = [(dict(epsilon=-0.01), b"epsilon must be in [0, 1]"), (dict(epsilon=1.01), b"epsilon must be in [0, 1]"),
           (dict(epsilon=math.nan), b"epsilon must be in [0, 1]")]
LAMBDA = [(dict(lam=-0.01), b"lambda must be in [0, 1]"), (dict(lam=1.01), b"lambda must be in [0, 1]"), (dict(lam=math.nan), b"lambda must be in [0, 1]")]
STEPS = [(dict(steps=None), b"steps is null")]
ACC = [(dict(acc=None), b"acc is null"), (dict(acc=8), b"acc must be 16-byte aligned")]
STEP = [(dict(step=0.0), b"step must be in (0, 1]"), (dict(step=1.01), b"step must be in (0, 1]"), (dict(step=math.nan), b"step must be in (0, 1]"),
        (dict(step=-0.5), b"step must be in (0, 1]")]
RESERVED = [(dict(reserved0=1), b"reserved0 must be 0")]
_TC_STATE = ("acc_abs", "e", "a", "tc_stats")
CASES = {                                                                  # per entry point; pulse_tfe_nt_learn_tc's open with pulse_tfe_nt_learn_lambda's
    "pulse_tfe_nt_rollout": NET_CASES + WEIGHTS + BATCH + EPSILON + null_and_odd(("keys", "values", "total_score", "stats"), ("lengths", "episode_reward")) + STEPS,
    "pulse_tfe_nt_learn": NET_CASES + BATCH + null_and_odd(("keys", "values", "stats"), ("lengths",)) + STEPS + ACC,
    "pulse_tfe_nt_apply": NET_CASES + WEIGHTS + STEP + ACC + RESERVED,
    "pulse_tfe_nt_evaluate": NET_CASES + WEIGHTS + BATCH + EPSILON + null_and_odd(("summary", "max_tile_hist"))
    + [(dict(total_score=4), b"total_score must be 8-byte aligned"), (dict(lengths=2), b"lengths must be 4-byte aligned")],
    "pulse_tfe_nt_learn_lambda": NET_CASES + BATCH + LAMBDA + null_and_odd(("keys", "values", "deltas", "stats"), ("lengths",)) + STEPS + ACC,
    "pulse_tfe_nt_apply_tc": NET_CASES + WEIGHTS + STEP + ACC + [(dict([(f, None)]), f.encode() + b" is null") for f in _TC_STATE] + [
        (dict([(f, 4)]), b"acc_abs / e / a / tc_stats must be 8-byte aligned") for f in _TC_STATE] + RESERVED,
}
CASES["pulse_tfe_nt_learn_tc"] = CASES["pulse_tfe_nt_learn_lambda"] + [
    (dict(acc_abs=None), b"acc_abs is null"), (dict(acc_abs=4), b"acc_abs must be 8-byte aligned"),
    (dict(deltas=None, lam=1.0), b"deltas is null"), (dict(deltas=None, lam=5e-324), b"deltas is null")]
SEARCH_CASES = NET_CASES + WEIGHTS + [(dict(n_boards=0), b"n_boards must be positive"), (dict(n_boards=-3), b"n_boards must be positive")] + GAMMA + [
    (dict(reserved0=1), b"reserved0 / reserved1 must be 0"), (dict(reserved1=1), b"reserved0 / reserved1 must be 0"),
    (dict(boards=None), b"boards is null"), (dict(q=None), b"q is null"), (dict(action=None), b"action is null"),
    (dict(candidates=None), b"candidates is null"), (dict(boards=4), b"boards / q must be 8-byte aligned"), (dict(q=4), b"boards / q must be 8-byte aligned")]


# ------------------------------------------------------------------ what opens and what closes every CPU file
def assert_exports(names_and_structs, argtypes, header_pattern):
    """Every (entry point, options struct) is a symbol of the library, is in _native.SYMBOLS as int(*argtypes), and is declared in
    include/pulse_env.h as header_pattern % (entry point, struct).  Returns (the library, the header's text)."""
    from pulselib_amd import _native
    lib, text = _native.lib(), (ROOT / "include" / "pulse_env.h").read_text()
    for name, struct in names_and_structs:
        assert hasattr(lib, name) and _native.SYMBOLS[name] == (C.c_int, list(argtypes)), name
        assert re.search(header_pattern % (name, struct), text), name
    return lib, text


def play_kernel(lanes, img, record, backed=False, start=False, net="NtDev"):
    """What names one instance of csrc's tfe_nt_play_kernel<LANES, IMG, Record, Backed, From, Net> in a kernel's mangled name."""
    return "tfe_nt_play_kernelILi%dELi%dELb%dELb%dELb%dENS_%d%sEEE" % (lanes, img, record, backed, start, len(net), net)


def play_kernels(lanes, record, backed=False, start=False, net="NtDev"):
    """assert_no_scratch's counts of the symmetric and the plain instance of play_kernel(lanes, IMG, ...): one each"""
    return {play_kernel(lanes, img, record, backed, start, net): 1 for img in (8, 1)}


# The twelve kernels each of csrc/tfe_ntuple_search.hip -- tfe_nt_search_kernel<LANES, IMG, Net> and the evaluations' games at one layer, at two
# and at the adaptive depth -- and of csrc/tfe_ntuple_search_rollout.hip: the recording games at one layer, at two and, Backed x From, at the adaptive depth
SEARCH_UNIT = {**{"tfe_nt_search_kernelILi%dELi%dENS_%sEEE" % (lanes, img, net): 1 for lanes, net in ((32, "5NtDev"), (256, "5NtDev"), (256, "13NtAdaptiveDev")) for img in (8, 1)},
               **play_kernels(32, False), **play_kernels(256, False), **play_kernels(256, False, net="NtAdaptiveDev")}
ROLLOUT_UNIT = {**play_kernels(32, True), **play_kernels(256, True), **{k: 1 for b in (False, True) for f in (False, True) for k in play_kernels(256, True, b, f, "NtAdaptiveDev")}}


def listed(text, kernel, field):
    """`field` of the LAST block of the compiler's remarks in `text` whose kernel's name holds `kernel`"""
    found = re.findall(r"Function Name: \S*" + re.escape(kernel) + r"\S*.*?" + re.escape(field) + r": (\d+)", text, flags=re.S)
    assert found, kernel
    return int(found[-1])


def assert_no_scratch(target, counts, max_vgprs):
    """The kernels of csrc's `make <target>` are those of `counts` {a substring of the name: how many}, none with scratch or a spilled
    vector register, none above max_vgprs.  Returns their names."""
    names, vgprs, scratch, spills = resource_usage(target)
    n = sum(counts.values())
    assert len(names) == n and all(sum(k in name for name in names) == c for k, c in counts.items()), names
    assert scratch == [0] * n and spills == [0] * n and len(vgprs) == n and max(vgprs) <= max_vgprs
    return names


# ------------------------------------------------------------------ on the device: the learners' regime
# 257 games = one full workgroup and one of one lane.  Rehearsed on the host for exactly these values: every round from zero weights has
# at least 8 games that end (the `terminal` bit, target 0) and at least 8 cut at move 256 (the skipped last move).
GAMES, MAX_STEPS, ROUNDS, EPSILON_PLAY = 257, 256, 3, .25
SEED, BOARD_ID0 = 457, 3000
BUFFERS = ("weights_dev", "acc", "keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters", "_eval")
PER_MOVE = ("keys", "values", "steps")


def seeds(seed, board_id0=BOARD_ID0, round=0):
    """(env_seed, agent_seed, tie_seed, board_id0, round) as the agent derives them from its `seed`: the tail of the host roll-out's
    positional arguments"""
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return seed, seed ^ AGENT_KEY, seed ^ TIE_KEY, board_id0, round


def plain_learner(n_games=GAMES, **kw):
    """the agent of the regime, `kw` over it, on buffers of its own"""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    kw = dict(dict(tuples=TUPLES, epsilon=EPSILON_PLAY, max_steps=MAX_STEPS, seed=SEED, board_id0=BOARD_ID0), **kw)
    return NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), n_games, **kw)


def learner_agent(n_games=GAMES, extra_buffers=(), patterns=PATTERNS, **kw):
    """plain_learner with every device buffer re-seated between guard words -- BUFFERS and those of `extra_buffers` the agent has --
    holding `patterns` (keys / values / steps: what a launch must keep at and beyond a game's length) or zero."""
    a = plain_learner(n_games, **kw)
    extra = tuple(k for k in extra_buffers if getattr(a, k) is not None)
    a = guard(a, BUFFERS + extra, **patterns)
    assert a.acc.data_ptr() % 16 == 0 and all(getattr(a, k).data_ptr() % 8 == 0 for k in extra)
    return a


def search_agent(games, max_steps, seed, name, symmetric=True, **kw):
    """the agent of a search file's shape with every device buffer re-seated between guard words and weights(name) of its tuples
    uploaded"""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    kw = dict(dict(tuples=TUPLES, symmetric=symmetric, max_steps=max_steps, seed=seed, board_id0=BOARD_ID0), **kw)
    a = guard(NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), games, **kw), BUFFERS, **PATTERNS)
    a.weights_dev.copy_(torch.from_numpy(weights(name, kw["tuples"]).copy()))
    return a


def search_outputs(n, dev):
    """(q, action, candidates) of n boards between guard words, holding patterns, and the guards"""
    import torch
    q, gq, nq = guarded(torch.zeros((n, 4), dtype=torch.float64, device=dev), -12345.678)
    action, ga, na = guarded(torch.zeros(n, dtype=torch.int8, device=dev), 0x55)
    cand, gc, nc = guarded(torch.zeros(n, dtype=torch.uint8, device=dev), 0x55)
    return q, action, cand, [("q", gq, nq), ("action", ga, na), ("candidates", gc, nc)]


def learner_round(a, after_learn=None, after_apply=None, coherence=None):
    """One round on the device -- roll-out, learn(), apply() -- with the learn and the apply launch held to the host's on the device's
    own records, the host's learner and apply chosen by the agent's own `tc` and `lam`; `coherence` = the host's (E, A) of a tc agent,
    advanced in place.  Returns a record of verdicts and counts, not of the big arrays (acc of TUPLES is 268 MB, and the records are
    kept for the session): those are compared here, where they are, and a file's further verdicts come from its hooks, each called as
    hook(a, h) and returning a dict for the record.  h holds the arrays in hand: after learn() policy (the weights the round played on),
    got (the roll-out read back), L, played, values (float64), acc, visited (the mask acc[:, 1] > 0), acc_abs, stats (the counters'
    differences), host (the host learner's counts), host_acc, host_abs, host_deltas (or None); after apply() also weights, host_w and
    host_tc (the host's (moved, rho sum), or None)."""
    n, h = nt(), SimpleNamespace(policy=a.weights(), got=rollout(a, PER_MOVE), acc_abs=None, host_abs=None, host_tc=None)
    before = a.stats()
    a.learn()
    h.acc, st = a.acc.cpu().numpy(), a.stats()
    h.visited = h.acc[:, 1] > 0                                            # (acc of TUPLES: every pass over it is felt, so this one is shared)
    h.L = h.got["lengths"].astype(np.int64)
    h.played, h.values = np.arange(a.max_steps)[:, None] < h.L[None, :], h.got["values"].view(np.float64)
    last = h.got["steps"][np.minimum(h.L, a.max_steps) - 1, np.arange(a.n_games)]
    records, h.host_acc = (h.got["keys"], h.values, h.got["steps"], h.L, a.tuples, a.symmetric, a.gamma), np.zeros_like(h.acc)
    if a.tc:
        h.acc_abs = a.acc_abs.cpu().numpy()
        h.host_abs = np.zeros_like(h.acc_abs)
        host = n.learn_tc_nt_on_host(*records, a.lam, h.host_acc, h.host_abs)
    elif a.lam:
        host = n.learn_lambda_nt_on_host(*records, a.lam, h.host_acc)
    else:
        host = n.learn_nt_on_host(*records, h.host_acc)
    h.host, h.host_deltas = host, host.pop("deltas", None)
    h.stats = {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")}
    rec = dict(ended=int((last >> 7 != 0).sum()), cut=int((last >> 7 == 0).sum()), moves=int(h.L.sum()), lengths=h.L, host=host, stats=h.stats,
               acc_equal=np.array_equal(h.acc, h.host_acc), acc_adds=int(h.acc[:, 1].sum()), visited=int(np.count_nonzero(h.visited)),
               values_any=bool(h.values[h.played].any()))
    rec.update(after_learn(a, h) if after_learn else {})
    a.apply()
    h.weights, h.host_w = a.weights(), h.policy.copy()
    if a.tc:
        h.host_tc = n.apply_tc_nt_on_host(h.host_w, h.host_acc, h.host_abs, *coherence, a.alpha / a.n_features)
    rec["moved"] = h.host_tc[0] if a.tc else n.apply_nt_on_host(h.host_w, h.host_acc, a.alpha / a.n_features)
    rec.update(weights_equal=np.array_equal(h.weights.view(np.uint32), h.host_w.view(np.uint32)),
               acc_zero=not bool(a.acc.any().item()) and not (a.tc and bool(a.acc_abs.any().item())))
    rec.update(after_apply(a, h) if after_apply else {})
    a.round += 1
    return rec
