"""The 2048 n-tuple network's rank-parallel rounds without a GPU: the host's pack and unpack, the exactness
argument on the host -- the sum of the shards' accumulators IS the single run's, and so are the weights, E and A after every apply --
the exchange's collective logic on two gloo ranks with the host's pack and unpack on both paths, the list struct's layout, the two
entry points with their refusals, the Python layer, and what the compiler made of the kernels."""
import ctypes as C
import functools
import inspect
import os
import re
import socket

import numpy as np
import pytest

from pulselib_amd.sharding import shard_tables
from tests.native_args import remarks
from tests.tfe_nt_host import nt_games_on_host, usable_on_host
from tests.tfe_nt_ranks_support import (ADAPTIVE_REHEARSED, DEEP_EMPTY_MAX, EPSILON, EVAL_GAMES, FIELDS, GAMES, GAMMA, GROWN_FROM, GROWN_TILE, LAM, MAX_STEPS, PACK,
                                        RESTART, ROUNDS, SPLITS, STAGE_TILES, STRUCT, TUPLES, UNPACK, assert_list_refusals, by_index, list_words)
from tests.tfe_nt_support import BOARD_ID0, ROOT, SEED, assert_exports, assert_no_scratch, seeds
from tests.tfe_nt_support import nt as _nt


# ------------------------------------------------------------------ the mirrors
def test_pack_and_unpack_round_trip_on_the_host():
    nt, rng = _nt(), np.random.default_rng(3)
    acc, ab = np.zeros((4000, 2), dtype=np.int64), np.zeros(4000, dtype=np.int64)
    at = rng.choice(4000, 300, replace=False)
    acc[at, 0], acc[at, 1], ab[at] = rng.integers(-10 ** 12, 10 ** 12, 300), rng.integers(1, 50, 300), rng.integers(0, 10 ** 12, 300)
    acc[at[0]] = (0, 2)                                                     # visited, and its differences cancel: kept
    acc[at[1]] = (77, 0)                                                    # never visited (cnt 0), whatever its sum: dropped
    acc[at[2]] = (5, -1)                                                    # no count at all: dropped
    before = acc.copy(), ab.copy()
    e = nt.pack_acc_on_host(acc, ab)
    assert e.dtype == np.int64 and e.shape == (298, 4) and (np.diff(e[:, 0]) > 0).all()
    assert np.array_equal(acc, before[0]) and np.array_equal(ab, before[1])                        # (only read)
    assert at[0] in e[:, 0] and at[1] not in e[:, 0] and at[2] not in e[:, 0]
    assert e[e[:, 0] == at[0]].tolist() == [[at[0], 0, 2, ab[at[0]]]]
    assert not nt.pack_acc_on_host(acc)[:, 3].any() and np.array_equal(nt.pack_acc_on_host(acc)[:, :3], e[:, :3])     # no acc_abs: abs is 0
    # into zeroed accumulators: the visited cells again; the others stay 0
    acc2, ab2 = np.zeros_like(acc), np.zeros_like(ab)
    assert nt.unpack_acc_on_host(acc2, ab2, e) == (298, 0)
    live = acc[:, 1] > 0
    assert np.array_equal(acc2[live], acc[live]) and np.array_equal(ab2[live], ab[live]) and not acc2[~live].any() and not ab2[~live].any()
    assert np.array_equal(nt.pack_acc_on_host(acc2, ab2), e)
    # a second time, shuffled: everything doubles; an index met twice in one list is added twice
    assert nt.unpack_acc_on_host(acc2, ab2, e[rng.permutation(298)]) == (298, 0) and np.array_equal(acc2[live], 2 * acc[live])
    assert nt.unpack_acc_on_host(acc2, None, np.array([[7, 1, 1, 9], [7, 2, 3, 9]])) == (2, 0) and ab2[7] == 2 * ab[7]
    # refused entries add nothing and are counted: index == len, beyond, negative (read as unsigned), cnt 0, cnt < 0
    kept = acc2.copy(), ab2.copy()
    bad = np.array([[4000, 1, 1, 1], [2 ** 40, 1, 1, 1], [-1, 1, 1, 1], [5, 9, 0, 9], [6, 9, -2, 9]])
    assert nt.unpack_acc_on_host(acc2, ab2, bad) == (0, 5) and np.array_equal(acc2, kept[0]) and np.array_equal(ab2, kept[1])
    assert nt.unpack_acc_on_host(acc2, ab2, np.vstack([bad, [[3999, -4, 1, 4]]])) == (1, 5) and acc2[3999].tolist() == [kept[0][3999, 0] - 4, kept[0][3999, 1] + 1]
    assert nt.unpack_acc_on_host(acc2, ab2, np.zeros((0, 4), dtype=np.int64)) == (0, 0)


def test_the_synthetic_buffers_of_the_device_tests():
    """tests/tfe_nt_ranks_support.py's buffers for the kernels' loops, at a cap of 24 workgroups: the tiles hold what their docstring
    says, the mirrors round-trip them, and the contended list's refusals are counted"""
    from tests.tfe_nt_ranks_support import BLOCK, DEAD, TILE, TINY, TINY_PATTERNS, contended_entries, multi_pass_accumulators, passes, tiny_accumulators
    nt, cap = _nt(), 24
    acc, ab, tiles = multi_pass_accumulators(cap)
    n = len(acc)
    assert n == (2 * cap + 1) * TILE + 517 and passes(n, TILE, cap) == 3 and [len(range(b, 2 * cap + 2, cap)) for b in (0, 1, 2, cap - 1)] == [3, 3, 2, 2]
    e = nt.pack_acc_on_host(acc, ab)
    per_tile = np.bincount(e[:, 0] // TILE, minlength=2 * cap + 2)
    assert {t: int(per_tile[t]) for t in tiles} == tiles and {0, n - 1} <= set(e[:, 0].tolist()) and (e[:, 1] < 0).any() and (e[:, 2] > 0).all()
    dead = np.flatnonzero((acc[:, 1] <= 0) & (acc[:, 0] != 0))
    assert len(dead) > 500 and sorted(set(map(tuple, acc[dead].tolist()))) == sorted(DEAD) and np.isin(dead // TILE, [cap, 1, 2 * cap + 1]).sum() >= 4
    acc2, ab2 = np.zeros_like(acc), np.zeros_like(ab)
    assert nt.unpack_acc_on_host(acc2, ab2, e) == (len(e), 0) and np.array_equal(nt.pack_acc_on_host(acc2, ab2), e)
    for n in TINY:
        for which in TINY_PATTERNS:
            acc, ab = tiny_accumulators(n, which, 3 * TILE)
            assert len(nt.pack_acc_on_host(acc[:n], ab[:n])) == dict(all=n, last=1, first=1, none=0)[which] and (acc[n:, 1] > 0).all()
    k = 2 * cap * BLOCK + 77
    entries, n_bad = contended_entries(k, 5000, np.random.default_rng(8))
    assert passes(k, BLOCK, cap) == 3 and nt.unpack_acc_on_host(np.zeros((5000, 2), dtype=np.int64), None, entries) == (k - n_bad, n_bad)
    hot = np.bincount(entries[:, 0][(entries[:, 0] >= 0) & (entries[:, 0] < 5000)], minlength=5000)[[0, 1234, 2500, 4999]]
    assert (hot > k // 40).all() and (entries[:, 0] == 5000).any() and (entries[:, 0] > 5000).any() and (entries[:, 0] < 0).any() and (entries[:, 2] == 0).any() and (entries[:, 2] < 0).any()


def test_the_shards_board_ids_are_the_single_process_s():
    nt = _nt()
    assert list(inspect.signature(nt.shard_round_board_id0).parameters) == ["board_id0", "round", "n_games_total", "game0"]
    assert nt.shard_round_board_id0(3000, 0, 13, 0) == 3000 and nt.shard_round_board_id0(3000, 2, 13, 7) == 3000 + 26 + 7
    for r in range(3):
        for split in SPLITS:
            ids = [nt.shard_round_board_id0(BOARD_ID0, r, GAMES, g0) + g for n, g0 in (shard_tables(GAMES, len(split), k) for k in range(len(split))) for g in range(n)]
            assert ids == [BOARD_ID0 + r * GAMES + g for g in range(GAMES)]
    assert [shard_tables(GAMES, len(s), k)[0] for s in SPLITS for k in range(len(s))] == [7, 6, 5, 4, 4]


# ------------------------------------------------------------------ exactness on the host
def _learn(nt, weights, n_games, board_id0, r):
    """one shard's (or the single run's) round r on the host: its accumulators from zero"""
    g = nt_games_on_host(n_games, MAX_STEPS, EPSILON, GAMMA, weights, TUPLES, True, *seeds(SEED, board_id0, r))
    W = nt.tuple_offsets(TUPLES)[1]
    acc, ab = np.zeros((W, 2), dtype=np.int64), np.zeros(W, dtype=np.int64)
    counts = nt.learn_tc_nt_on_host(g["keys"], g["values"], g["steps"], g["lengths"], TUPLES, True, GAMMA, LAM, acc, ab)
    return acc, ab, counts["learnt"]


@functools.lru_cache(maxsize=None)
def _rounds():
    """Three rounds of 13 games of up to 24 moves, epsilon .25, TD(.5) with temporal coherence, on the host.  Per round: the single
    run's accumulators as entries (pack_acc_on_host), per split the shards' entries, and the weights, E and A after the apply; every
    comparison of the big arrays is made here, where they are."""
    nt = _nt()
    W, F = nt.tuple_offsets(TUPLES)[1], 8 * len(TUPLES)
    w, E, A, out = np.zeros(W, dtype=np.float32), np.zeros(W), np.zeros(W), []
    for r in range(ROUNDS):
        acc, ab, learnt = _learn(nt, w, GAMES, BOARD_ID0 + r * GAMES, r)
        rec = dict(single=nt.pack_acc_on_host(acc, ab), learnt=learnt, shards={}, sums_equal=[], learnt_equal=[], applied_equal=[])
        after = w.copy(), E.copy(), A.copy()
        nt.apply_tc_nt_on_host(*after[:1], acc.copy(), ab.copy(), *after[1:], 1.0 / F)
        for split in SPLITS:
            parts = [_learn(nt, w, n, nt.shard_round_board_id0(BOARD_ID0, r, GAMES, g0), r) for n, g0 in (shard_tables(GAMES, len(split), k) for k in range(len(split)))]
            assert [n for n, _ in (shard_tables(GAMES, len(split), k) for k in range(len(split)))] == list(split)
            total, total_abs = sum(p[0] for p in parts), sum(p[1] for p in parts)
            rec["sums_equal"].append(np.array_equal(total, acc) and np.array_equal(total_abs, ab))
            rec["learnt_equal"].append(sum(p[2] for p in parts) == learnt)
            mine = w.copy(), E.copy(), A.copy()                             # every rank applies the merged accumulators to the same weights
            nt.apply_tc_nt_on_host(*mine[:1], total, total_abs, *mine[1:], 1.0 / F)
            rec["applied_equal"].append(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(mine, after)))
            rec["shards"][split] = [nt.pack_acc_on_host(p[0], p[1]) for p in parts]
        w, E, A = after
        rec["moved"] = int(np.count_nonzero(w))
        out.append(rec)
    return out, W


def test_the_shards_accumulators_sum_to_the_single_run_s():
    """split 7 + 6 and 5 + 4 + 4: acc and acc_abs of the shards, summed, equal the single run's word for word, and the weights, E and A
    after each apply are equal bit for bit; the rounds are real ones -- they learn moves, share cells between the shards and move
    weights"""
    rounds, W = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["sums_equal"] == [True, True] and rec["learnt_equal"] == [True, True] and rec["applied_equal"] == [True, True], r
        assert rec["learnt"] > 100 and len(rec["single"]) > 100 and rec["moved"] > 100, r   # (early boards hold few distinct tiles: hundreds of cells, not thousands)
        for split, shards in rec["shards"].items():
            assert all(len(s) for s in shards)
            assert sum(len(s) for s in shards) > len(rec["single"]), (r, split)       # some cell is met by two shards: the adds overlap
    assert rounds[1]["moved"] > rounds[0]["moved"]                                  # (round 1 played on round 0's weights)


# ------------------------------------------------------------------ the regimes of the device's sharded cases, on the host
# tests/test_tfe_nt_ranks_gpu.py asserts "> 0" of what a case is there for -- boards picked and started, moves at both depths, weights in
# two stages.  The host mirrors play the same 13 games here, so those hold by the constants of tests/tfe_nt_ranks_support.py and are not
# tuned on the device.
def test_the_restart_case_picks_and_starts_boards():
    """TD(0) from zero weights, restart_fraction .5, restart_min_length 8: rounds 0 and 1 on the host.  Both pick boards, and round 1
    begins games on the boards round 0 picked."""
    nt = _nt()
    W, F = nt.tuple_offsets(TUPLES)[1], 8 * len(TUPLES)
    w, start = np.zeros(W, dtype=np.float32), np.zeros(GAMES, dtype=np.uint64)
    for r in range(2):
        id0 = BOARD_ID0 + r * GAMES
        g = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, GAMMA, w, TUPLES, True, *seeds(SEED, id0, r), start=start)
        assert int(np.count_nonzero(g["start_left"])) == (0 if r == 0 else picked) and (r == 0 or picked > 0)    # started: the games begun on a picked board
        acc = np.zeros((W, 2), dtype=np.int64)
        assert nt.learn_nt_on_host(g["keys"], g["values"], g["steps"], g["lengths"], TUPLES, True, GAMMA, acc)["learnt"] > 100
        assert nt.apply_nt_on_host(w, acc, 1.0 / F) > 100
        start, (picked, depth) = nt.restart_pick_on_host(g["keys"], g["lengths"], MAX_STEPS, SEED, id0, RESTART["restart_fraction"], RESTART["restart_min_length"])
        print("round", r, "lengths", g["lengths"].tolist(), "picked", picked, "depth", depth)
        assert picked > 0 and depth > 0 and int(usable_on_host(start).sum()) == picked == int(np.count_nonzero(start))
        assert (g["lengths"] >= RESTART["restart_min_length"]).sum() == picked


def test_the_staged_case_reaches_two_stages():
    """stage_tiles (8, 16), TD(.5) with temporal coherence, round 0 from zero weights on the host: within 24 moves games reach the 8
    and some the 16, moves are learnt in at least two stages and their adds are not all zero.  The stage tiles (16,) of the grown
    case, split at 8, are the same three stages."""
    from tests.tfe_nt_staged_support import adds_per_stage
    nt = _nt()
    tuples = nt.with_stages(TUPLES, STAGE_TILES)
    W, S = nt.tuple_offsets(TUPLES)[1], len(STAGE_TILES) + 1
    g = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, GAMMA, np.zeros(S * W, dtype=np.float32), tuples, True, *seeds(SEED))
    top = g["final_boards"].reshape(GAMES, -1).max(axis=1)
    print("largest tiles", top.tolist())
    assert (top >= 8).sum() >= GAMES - 2 and (top >= 16).sum() >= 2
    acc, ab = np.zeros((S * W, 2), dtype=np.int64), np.zeros(S * W, dtype=np.int64)
    nt.learn_tc_nt_on_host(g["keys"], g["values"], g["steps"], g["lengths"], tuples, True, GAMMA, LAM, acc, ab)
    adds = adds_per_stage(acc, S)
    print("adds per stage", adds)
    assert sum(a > 0 for a in adds) >= 2 and sum(bool(x[:, 0].any()) for x in acc.reshape(S, -1, 2)) >= 2
    assert nt.split_stage_tiles(GROWN_FROM, GROWN_TILE)[0] == STAGE_TILES


def adaptive_case_on_host(rounds, evaluate=False):
    """The adaptive case on the host: `rounds` rounds of 13 games at E = DEEP_EMPTY_MAX with backed targets (TD(0)) and restarts, from
    zero weights; per round (moves two layers deep, one layer deep, boards picked); with `evaluate` also the depth words of the 11
    evaluation games on the weights as they stand.  adaptive_case_on_host(ROUNDS, True) is what ADAPTIVE_REHEARSED records."""
    nt = _nt()
    W, F = nt.tuple_offsets(TUPLES)[1], 8 * len(TUPLES)
    w, start, out = np.zeros(W, dtype=np.float32), np.zeros(GAMES, dtype=np.uint64), []
    for r in range(rounds):
        id0 = BOARD_ID0 + r * GAMES
        g = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, GAMMA, w, TUPLES, True, *seeds(SEED, id0, r), deep_empty_max=DEEP_EMPTY_MAX, backed=True, start=start)
        acc = np.zeros((W, 2), dtype=np.int64)
        nt.learn_backed_nt_on_host(g["keys"], g["values"], g["backed"], g["steps"], g["lengths"], TUPLES, True, GAMMA, 0.0, acc)
        nt.apply_nt_on_host(w, acc, 1.0 / F)
        start, (picked, _) = nt.restart_pick_on_host(g["keys"], g["lengths"], MAX_STEPS, SEED, id0, RESTART["restart_fraction"], RESTART["restart_min_length"])
        out.append((g["deep"], g["shallow"], picked))
    if evaluate:
        ev = nt_games_on_host(EVAL_GAMES, MAX_STEPS, 0.0, GAMMA, w, TUPLES, True, *seeds(SEED, BOARD_ID0 + (1 << 62), rounds), deep_empty_max=DEEP_EMPTY_MAX, record=False)
        out.append((ev["deep"], ev["shallow"]))
    return out


def test_the_adaptive_case_moves_at_both_depths():
    """Round 0 of the adaptive case on the host (the later rounds and the evaluation are recorded in ADAPTIVE_REHEARSED, which the
    device test holds the device to): moves at both depths, every one of them counted, boards picked.  The depth words only grow, so
    round 0 alone puts both above 0.  Whatever the weights, a game's first move is one layer deep at any E below 14: a reset board
    has 14 empty cells."""
    (deep, shallow, picked), = adaptive_case_on_host(1)
    print("E", DEEP_EMPTY_MAX, "deep", deep, "shallow", shallow, "picked", picked)
    assert (deep, shallow) == ADAPTIVE_REHEARSED["per_round"][0] and deep > 0 and shallow >= GAMES and picked > 0 and DEEP_EMPTY_MAX < 14
    assert tuple(map(sum, zip(*ADAPTIVE_REHEARSED["per_round"]))) == tuple(ADAPTIVE_REHEARSED["rounds"].values())
    assert all(x > 0 for x in ADAPTIVE_REHEARSED["evaluation"])


# ------------------------------------------------------------------ two gloo ranks on CPU tensors
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, W, shards, out):
    """the exchange's collective logic (tfe_ntuple_ranks.exchange_round) on the host's pack and unpack: first with a list that holds
    everything, then with room for 3 entries"""
    import torch.distributed as dist
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    from pulselib_amd.agents.tfe_ntuple_host import pack_acc_on_host, unpack_acc_on_host
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    ranks.init_ranks("gloo", rank, world)
    try:
        got = {}
        for name, capacity in (("roomy", len(shards[rank]) + (5 if rank else 0)), ("three", 3)):
            acc, ab = np.zeros((W, 2), dtype=np.int64), np.zeros(W, dtype=np.int64)
            unpack_acc_on_host(acc, ab, shards[rank])
            side = ranks.HostAccumulators(acc, ab, capacity)
            rec = ranks.exchange_round(side, None)
            got[name] = dict(rec, merged=pack_acc_on_host(acc, ab), added=side.added, refused=side.refused)
        got["shard_of"] = ranks.shard_of(GAMES)
        got["words"] = ranks.reduce_words([rank + 1, 10 * (rank + 1), 7 - rank], None, max_at=(2,))
        out[rank] = got
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_exchange_on_both_paths():
    """rank 0's list is exactly full (capacity == found), rank 1's has room to spare and is shorter than rank 0's count: the sparse
    path, named in the record; with room for 3 entries: the dense path, named too.  Both leave both ranks with the single run's
    accumulators."""
    import torch.multiprocessing as mp
    rounds, W = _rounds()
    single, shards = rounds[1]["single"], rounds[1]["shards"][(7, 6)]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), W, shards, out), nprocs=2, join=True)
    found = [len(s) for s in shards]
    for rank in range(2):
        got = out[rank]
        assert got["roomy"]["path"] == "sparse" and got["three"]["path"] == "dense", rank
        for name in ("roomy", "three"):
            assert got[name]["entries"] == found and np.array_equal(got[name]["merged"], single), (rank, name)
        assert (got["roomy"]["added"], got["roomy"]["refused"]) == (found[1 - rank], 0) and got["three"]["added"] == 0
        assert got["roomy"]["bytes"] == 2 * 32 + 2 * 8 * (4 + 4 * max(found)) and got["three"]["bytes"] == 2 * 32 + 8 * 3 * W
        assert got["shard_of"] == shard_tables(GAMES, 2, rank) and got["words"] == [3, 30, 7]


def test_a_world_of_one_moves_nothing():
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    nt = _nt()
    acc = np.zeros((50, 2), dtype=np.int64)
    acc[[3, 9, 40]] = [(5, 1), (0, 2), (-7, 3)]
    before = acc.copy()
    side = ranks.HostAccumulators(acc, None, 8)
    assert ranks.exchange_round(side, None) == dict(path="sparse", entries=[3], bytes=0) and np.array_equal(acc, before)
    assert ranks.group_of(None) == (None, 1, 0) and ranks.shard_of(13) == (13, 0) and ranks.reduce_words([4, 5], None, max_at=(1,)) == [4, 5]
    words = side.pack().numpy()
    assert np.array_equal(words, list_words(nt.pack_acc_on_host(acc), 8)) and words[:4].tolist() == [3, 3, 0, 0]
    small = ranks.HostAccumulators(acc, None, 2).pack().numpy()
    assert small[:4].tolist() == [3, 2, 0, 0] and len(small) == 12 and np.array_equal(by_index(small[4:]), nt.pack_acc_on_host(acc)[:2])
    assert ranks.GROUP_TIMEOUT_S == 60


# ------------------------------------------------------------------ the ABI
def test_library_exports_the_entry_points():
    from pulselib_amd import _native
    lib, text = assert_exports(((PACK, STRUCT), (UNPACK, STRUCT)), [C.c_void_p, C.c_void_p], r"int %s\(const %s\* o, void\* stream\);")
    body = re.search(r"typedef struct PulseTfeNtAccList \{(.*?)\} PulseTfeNtAccList;", text, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == FIELDS            # the header's fields, in the binding's order
    assert [t for t in re.findall(r"^\s*(\w+\*?) \w+;", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)] == ["uint64_t", "int64_t*", "int64_t*", "uint64_t", "int64_t*", "int64_t*", "int64_t"]
    s = _native.TfeNtAccList
    assert C.sizeof(s) == 56 and [f[0] for f in s._fields_] == FIELDS and [getattr(s, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48]
    assert [f[1] for f in s._fields_] == [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64]
    assert "static_assert(sizeof(PulseTfeNtAccList) == 56" in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_exchange.hip").read_text()
    assert "sizeof == 56" in text
    # nothing that was there moved
    assert C.sizeof(_native.TfeNtContinuePick) == 96 and C.sizeof(_native.TfeNtApplyTc) == 160 and C.sizeof(_native.TfeNtRollout) == 232 and lib.pulse_version() == 1


def test_the_entry_points_refuse():
    assert_list_refusals()


# ------------------------------------------------------------------ the Python layer
def test_python_layer():
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    from pulselib_amd.agents.tfe_common import _TFEGamesGPU
    from tests.tfe_nt_support import assert_init_parameters
    nt = _nt()
    assert_init_parameters(Agent)
    assert Agent._shard is None
    assert list(inspect.signature(Agent.set_shard).parameters) == ["self", "n_games_total", "game0", "group", "exchange_capacity"]
    assert [p.default for p in list(inspect.signature(Agent.set_shard).parameters.values())[3:]] == [None, None]
    assert list(inspect.signature(Agent.learn_batch).parameters) == ["self"] and list(inspect.signature(Agent.exchange).parameters) == ["self"]
    assert list(inspect.signature(nt.pack_acc_on_host).parameters) == ["acc", "acc_abs"] and inspect.signature(nt.pack_acc_on_host).parameters["acc_abs"].default is None
    assert list(inspect.signature(nt.unpack_acc_on_host).parameters) == ["acc", "acc_abs", "entries"]
    assert "round_board_id0" in vars(Agent) and "round_board_id0" in vars(_TFEGamesGPU)         # overridden in the n-tuple class only
    for name in ("set_shard", "pulse_tfe_nt_acc_pack", "pulse_tfe_nt_acc_unpack", "13.14"):
        assert name in Agent.__doc__ + nt.__doc__, name
    assert "host read" in Agent.exchange.__doc__.lower() and "host read" in ranks.__doc__.lower() and "OWN" in Agent._evaluate_with.__doc__
    agent = Agent.__new__(Agent)                                           # (no device)
    agent.board_id0, agent.round, agent.n_games = 3000, 2, 6
    assert agent.round_board_id0() == 3012 and agent.round_board_id0(0) == 3000                  # no shard: as it was
    for call in (agent.exchange, agent.exchange_summary):
        with pytest.raises(ValueError, match="no shard is set"):
            call()
    agent.n_weights, agent.max_steps, agent.n_features, agent.device = 1000, 4, 8, None     # (one stage: total_weights is n_weights)
    for total, game0 in ((5, 0), (13, 8), (13, -1)):
        with pytest.raises(ValueError, match="a shard must lie inside the job's games"):
            agent.set_shard(total, game0)
    for bad in (0, -3, True, 2.0):
        with pytest.raises(ValueError, match="exchange_capacity must be None or a positive int"):
            agent.set_shard(13, 7, exchange_capacity=bad)
    assert agent._shard is None
    assert agent.set_shard(13, 7) is agent and agent._shard.side.capacity == 6 * 4 * 8 and agent.round_board_id0() == 3000 + 26 + 7
    assert agent.round_board_id0(0) == 3007 and agent.set_shard(13, 7, exchange_capacity=5000)._shard.side.capacity == 192
    agent.n_weights = 100
    assert agent.set_shard(13, 0)._shard.side.capacity == 100 and agent.set_shard(13, 0, exchange_capacity=3)._shard.side.capacity == 3
    assert agent._shard.eval_shard(11, (1 << 62) + 5) == (11, (1 << 62) + 5)                    # (a world of one plays them all)
    # the depth words are read through the shard's reduce, as stats() is: a world of one reduces to itself; without a shard as it was
    import torch
    seen = []
    agent._shard.reduce = lambda words, max_at=(): seen.append(list(words)) or ranks.reduce_words(words, None, None, max_at)
    agent.depth_stats = torch.tensor([5, 7], dtype=torch.int64)
    assert agent._depth_read() == [5, 7] and agent.rollout_depth_summary(clear=False) == dict(moves_deep=5, moves_shallow=7)
    assert agent.rollout_depth_summary() == dict(moves_deep=5, moves_shallow=7) and agent.depth_stats.tolist() == [0, 0]
    assert seen == [[5, 7]] * 3
    sharded, agent._shard = agent._shard, None
    agent.depth_stats = torch.tensor([2, 3], dtype=torch.int64)
    assert agent.rollout_depth_summary() == dict(moves_deep=2, moves_shallow=3) and seen == [[5, 7]] * 3
    agent._shard, agent.depth_stats = sharded, None
    with pytest.raises(ValueError, match="no adaptive launch has run"):
        agent.rollout_depth_summary()
    assert "_depth_read" in inspect.getsource(Agent.evaluate_search) and "job-wide" in Agent._depth_read.__doc__
    assert "rollout_depth_summary()" in Agent.__doc__.split("job-wide")[0].rsplit("stats()", 1)[1]       # named in the list of job-wide read-backs
    # check_options takes the shard, and the shard goes with everything
    assert nt.check_options(shard=(13, 7, 6)) == (0, False, 0, None)
    assert nt.check_options(1, True, 0.5, False, 64, True, shard=(13, 0, 13)) == (1, True, 0, None)
    assert nt.check_options(2, True, 0.0, True, 16, rollout_deep_empty_max=3, shard=(13, 7, 6), script=True) == (2, True, 0, None)
    with pytest.raises(ValueError, match="a shard must lie inside"):
        nt.check_options(shard=(13, 8, 6))
    with pytest.raises(ValueError, match="must be ints"):
        nt.check_options(shard=(13, True, 6))
    assert inspect.signature(nt.check_options).parameters["shard"].kind is inspect.Parameter.KEYWORD_ONLY
    # the script
    from pulselib_amd.scripts import tfe_ntuple as script
    assert inspect.signature(script.run).parameters["shard"].default is False
    for argv in (["--ranks", "0"], ["--ranks-one-device"], ["--ranks", "2", "--continue-games", "--max-steps", "1"]):
        with pytest.raises(SystemExit) as err:                              # (refused before a process is started or a device asked for)
            script.main(argv)
        assert err.value.code == 2


# ------------------------------------------------------------------ what the compiler made of the kernels
def test_exchange_kernels_use_no_scratch():
    """hipcc --offload-arch=gfx950 on csrc/tfe_ntuple_exchange.hip with the Makefile's flags: three kernels, no scratch, no spilled
    register.  46, 3 and 20 VGPRs as built; the ceiling is 64, the most at which eight waves still fit a SIMD.  No inline assembly."""
    names = assert_no_scratch("ntuple-exchange-resource-usage", {"tfe_nt_acc_pack_kernel": 1, "tfe_nt_acc_pack_tail_kernel": 1, "tfe_nt_acc_unpack_kernel": 1}, 64)
    assert len(names) == 3 and len(re.findall(r"Function Name:", remarks("ntuple-exchange-resource-usage"))) == 3
    assert "asm" not in (ROOT / "pulselib_amd" / "csrc" / "tfe_ntuple_exchange.hip").read_text()
    lines = (ROOT / "profiles" / "tfe_mc" / "kernel_resource_usage.txt").read_text()
    assert all(n in lines for n in names)
