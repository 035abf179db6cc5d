"""What the two files of the 2048 n-tuple network's rank-parallel rounds share (tests/test_tfe_nt_ranks_cpu.py, _gpu.py; DESIGN.md section
13.14): the regime, the list struct built from keywords with its refusal table, and a list made by hand.  A helper, not a test."""
import ctypes as C

import numpy as np

from tests.native_args import opts as plain_opts
from tests.tfe_nt_support import BOARD_ID0, DEFAULTS, SEED, SHAPES

PACK, UNPACK, STRUCT = "pulse_tfe_nt_acc_pack", "pulse_tfe_nt_acc_unpack", "PulseTfeNtAccList"
FIELDS = ["n_entries", "acc", "acc_abs", "capacity", "list", "stats", "reserved0"]
TUPLES = SHAPES["eight"]                                                   # 1,188,368 cells: no multiple of 1,024 nor of 256, so the last workgroup is ragged
GAMES, MAX_STEPS, ROUNDS, EPSILON, GAMMA, LAM = 13, 24, 3, DEFAULTS["epsilon"], DEFAULTS["gamma"], 0.5
SPLITS = ((7, 6), (5, 4, 4))                                               # sharding.shard_tables of 13 games over 2 and 3 ranks
assert (SEED, BOARD_ID0, EPSILON, GAMMA) == (457, 3000, 0.25, 1.0)

# The options of the sharded cases beyond the first four (tests/test_tfe_nt_ranks_gpu.py: CASES); tests/test_tfe_nt_ranks_cpu.py plays
# every regime on the host mirrors, so that no case passes by never reaching what it is there for.
RESTART = dict(restart_fraction=0.5, restart_min_length=8)                 # a game of 24 moves is picked at move 12; most games are cut at 24
STAGE_TILES, GROWN_FROM, GROWN_TILE = (8, 16), (16,), 8                    # early tiles: a game from reset crosses both inside 24 moves
DEEP_EMPTY_MAX = 11                                                        # E of the adaptive case: boards with 5 tiles or more are searched two layers deep
EVAL_GAMES = 11
# The adaptive case rehearsed on the host (tests/test_tfe_nt_ranks_cpu.py: adaptive_case_on_host(ROUNDS), about 80 s; the test there plays
# round 0, about 15 s): every game is cut at 24 moves and every round picks all 13 games at move 12, so rounds 1 and 2 begin on boards
# of 5 tiles or more.  Moves two layers / one layer deep at E = 11: round 0 208 / 104, round 1 307 / 5, round 2 312 / 0; the 11
# evaluation games on the weights after round 2, round 3's tie coins, epsilon 0: 175 / 89.  (E = 12: 271 / 41, 312 / 0, 312 / 0 and
# 230 / 34; E = 13: 295 / 17, 312 / 0, 312 / 0 and 251 / 13 -- both depths too, with fewer shallow moves.)
ADAPTIVE_REHEARSED = dict(per_round=((208, 104), (307, 5), (312, 0)), rounds=dict(moves_deep=827, moves_shallow=109), evaluation=(175, 89))

_WORDS = (C.c_int64 * 16)()
HOST = (C.addressof(_WORDS) + 31) & ~31                                    # host words, 32-byte aligned: they pass every check, and no refusal reads them


def list_opts(**kw):
    from pulselib_amd import _native
    base = dict(n_entries=1000, acc=HOST, acc_abs=HOST, capacity=16, list=HOST, stats=HOST)
    return plain_opts(_native.TfeNtAccList, **{**base, **kw})


LIST_CASES = [(dict(n_entries=0), b"n_entries must be in 1..2^32"), (dict(n_entries=2 ** 32 + 1), b"n_entries must be in 1..2^32"),
              (dict(acc=None), b"acc is null"), (dict(acc=HOST + 8), b"acc must be 16-byte aligned"),
              (dict(acc_abs=HOST + 4), b"acc_abs must be 8-byte aligned"), (dict(capacity=0), b"capacity must be positive"),
              (dict(list=None), b"list is null"), (dict(list=HOST + 16), b"list must be 32-byte aligned"), (dict(list=HOST + 8), b"list must be 32-byte aligned"),
              (dict(stats=HOST + 4), b"stats must be 8-byte aligned"), (dict(reserved0=1), b"reserved0 must be 0 (zero-initialise the struct)")]
UNPACK_ONLY = [(dict(stats=None), b"stats is null")]


def assert_list_refusals():
    """both entry points, through the one refusal runner, message for message"""
    from pulselib_amd import _native
    from tests.native_args import assert_refusals
    for name, cases in ((PACK, LIST_CASES), (UNPACK, LIST_CASES + UNPACK_ONLY)):
        errors = assert_refusals(_native.lib(), name, list_opts, cases)
        assert [e.split(b": ", 1)[1] for e in errors] == [msg for _, msg in cases]


def list_words(entries, capacity, found=None, written=None):
    """int64[4 + 4 * capacity]: the header {found, written, 0, 0} (default: both the number of entries) and the entries int64[k, 4]"""
    entries = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    words = np.zeros(4 + 4 * capacity, dtype=np.int64)
    words[0], words[1] = len(entries) if found is None else found, len(entries) if written is None else written
    words[4:4 + 4 * len(entries)] = entries.reshape(-1)
    return words


def by_index(entries):
    entries = np.asarray(entries, dtype=np.int64).reshape(-1, 4)
    return entries[np.argsort(entries[:, 0], kind="stable")]


# ------------------------------------------------------------------ synthetic accumulators and lists at the shapes where the kernels' loops turn
TILE, BLOCK = 1024, 256                                                    # the pack kernel's cells per workgroup and pass; the unpack kernel's entries
TINY = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)              # n_entries either side of a wavefront, a wavefront's 256 cells, a tile, two tiles
TINY_PATTERNS = ("all", "last", "first", "none")
DEAD = ((77, 0), (5, -1))                                                  # never visited, whatever the sum; no count at all: neither is an entry


def device_launcher():
    """What a launch of the two entry points needs of an agent, without one: the library, the device and the agents' `_launch`."""
    import torch
    from pulselib_amd import _native
    from pulselib_amd.agents.tfe_common import _TFEGamesGPU

    class _Launcher:
        _lib, device, _launch = _native.lib(), torch.device("cuda:0"), _TFEGamesGPU._launch
    return _Launcher()


def passes(n_items, per_pass, cap):
    """how often workgroup 0 of a grid of min(ceil(n_items / per_pass), cap) workgroups goes round its grid-stride loop"""
    blocks = -(-n_items // per_pass)
    return len(range(0, blocks, min(blocks, cap)))


def _make_live(rng, acc, ab, at):
    at = np.asarray(at, dtype=np.int64)
    acc[at, 0], acc[at, 1], ab[at] = rng.integers(-10 ** 12, 10 ** 12, len(at)), rng.integers(1, 99, len(at)), rng.integers(0, 10 ** 12, len(at))


def multi_pass_accumulators(cap, seed=11):
    """(acc int64[n, 2], acc_abs int64[n], tiles) for a pack grid capped at `cap` workgroups: n = (2 cap + 1) * 1,024 + 517 cells, 2 cap + 2
    tiles, the last ragged.  Only the workgroups 0 and 1 have a third pass (tiles 2 cap, the last full one, and 2 cap + 1, the ragged
    one), so the tiles are laid out by hand for the workgroups 0, 1 and 2 (`tiles`: {tile: live cells}):
      workgroup 0: tile 0 sparse (8 cells, cell 0 among them), tile cap without a live cell, tile 2 cap all 1,024 live -- the skipped
                   atomic, then a wg_base of the same parity as the one pass 0 left behind;
      workgroup 1: tile 1 without a live cell, tile cap + 1 all live, the ragged tile 4 cells, cell n - 1 among them -- its parity-0
                   words are first written in its third pass;
      workgroup 2: tile 2 without a live cell, tile cap + 2 all live (it has no third pass).
    0.2 % of all other cells are live.  Live cells hold random sums of either sign, cnt in 1..98 and abs; about 600 cells that are not
    live hold DEAD's two pairs and a non-zero abs, some of them inside the tiles without a live cell."""
    rng = np.random.default_rng(seed)
    n = (2 * cap + 1) * TILE + 517
    acc, ab = np.zeros((n, 2), dtype=np.int64), np.zeros(n, dtype=np.int64)
    tiles = {0: 8, cap: 0, 2 * cap: TILE, 1: 0, cap + 1: TILE, 2 * cap + 1: 4, 2: 0, cap + 2: TILE}
    free = np.ones(n, dtype=bool)
    for t in tiles:
        free[t * TILE:(t + 1) * TILE] = False
    _make_live(rng, acc, ab, np.flatnonzero(free & (rng.random(n) < 0.002)))
    _make_live(rng, acc, ab, [0, 5, 63, 64, 255, 256, 700, 1023])           # tile 0: cell 0, either side of a wavefront's 64 lanes and of its 256 cells, the tile's last
    for t in (2 * cap, cap + 1, cap + 2):
        _make_live(rng, acc, ab, np.arange(t * TILE, (t + 1) * TILE))
    _make_live(rng, acc, ab, [n - 517, n - 300, n - 2, n - 1])              # the ragged tile: its first cell, its last two
    dead = np.unique(np.concatenate([rng.choice(np.flatnonzero(acc[:, 1] == 0), 600, replace=False), [cap * TILE + 3, cap * TILE + 1023, 2 * TILE - 1, n - 3]]))
    acc[dead[::2]], acc[dead[1::2]], ab[dead] = DEAD[0], DEAD[1], 9
    return acc, ab, tiles


def tiny_accumulators(n, which, cells, decoy=(999, 7)):
    """(acc int64[cells, 2], acc_abs int64[cells]) for a launch with n_entries = n: the cells below n by TINY_PATTERNS' `which`, every
    cell from n on LIVE (`decoy`): a lane that took a cell beyond n_entries for a cell would add an entry."""
    acc, ab = np.zeros((cells, 2), dtype=np.int64), np.zeros(cells, dtype=np.int64)
    acc[n:], ab[n:] = decoy, 55
    at = dict(all=np.arange(n), last=np.array([n - 1]), first=np.array([0]), none=np.zeros(0, dtype=np.int64))[which]
    acc[at, 0], acc[at, 1], ab[at] = at * 3 - 100, 1 + at % 5, 1000 + at
    return acc, ab


def contended_entries(k, n_cells, rng, n_bad=300):
    """int64[k, 4]: one entry in eight on one of four hot cells, the others uniform over the n_cells cells; `n_bad` entries at random slots
    are to be refused, a fifth each: index == n_cells, an index beyond, a negative index, cnt 0, cnt < 0.  Returns (entries, n_bad)."""
    e = np.stack([rng.integers(0, n_cells, k), rng.integers(-10 ** 12, 10 ** 12, k), rng.integers(1, 99, k), rng.integers(0, 10 ** 12, k)], axis=1)
    hot = np.flatnonzero(np.arange(k) % 8 == 3)
    e[hot, 0] = np.array([0, 1234, 2500, n_cells - 1])[rng.integers(0, 4, len(hot))]
    bad = rng.choice(k, n_bad, replace=False)
    for i, slots in enumerate(np.array_split(bad, 5)):
        if i < 3:
            e[slots, 0] = (n_cells, n_cells + 1 + rng.integers(0, 1 << 40, len(slots)), -1 - rng.integers(0, 1 << 40, len(slots)))[i]
        else:
            e[slots, 2] = 0 if i == 3 else -rng.integers(1, 99, len(slots))
    return e, n_bad
