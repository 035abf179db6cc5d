"""The 2048 n-tuple network's rank-parallel rounds on the device (csrc/tfe_ntuple_exchange.hip:
pulse_tfe_nt_acc_pack, pulse_tfe_nt_acc_unpack) against the host's pack and unpack, and two gloo ranks on one device against one
process on all the games.  Every comparison is exact: integers word for word, float32 and float64 as bit patterns.  Every buffer a
launch is handed sits between guard words.

Shapes: the network "eight" of tests/tfe_nt_support.py, 1,188,368 cells -- no multiple of the pack's 1,024-cell tile nor of 256, so
the last workgroup is ragged and the launch takes 1,161 tiles --; the accumulators of a real learn launch on 8 games of 16 moves
with cells set by hand on top; synthetic int64 buffers, no agent, where the kernels' grid-stride loops turn three times under the cap
of eight workgroups per compute unit ((2 cap + 1) * 1,024 + 517 cells, 2 cap * 256 + 77 entries: about 4.2 M cells and 1 M entries at
256 compute units), n_entries from 1 to 2,049, and one entry in eight on four cells; for the ranks 13 games (7 + 6) of at most 24
moves, 3 rounds, epsilon .25, under every option that goes with a shard."""
import os
import socket

import numpy as np
import pytest

from tests.tfe_gpu_support import guarded, guards_intact
from tests.tfe_nt_ranks_support import (ADAPTIVE_REHEARSED, BLOCK, DEAD, DEEP_EMPTY_MAX, EVAL_GAMES, GAMES, GROWN_FROM, GROWN_TILE, LAM, MAX_STEPS, PACK, RESTART, ROUNDS,
                                        STAGE_TILES, TILE, TINY, TINY_PATTERNS, TUPLES, UNPACK, assert_list_refusals, by_index, contended_entries, device_launcher,
                                        list_words, multi_pass_accumulators, passes, tiny_accumulators)
from tests.tfe_nt_support import learner_agent, nt, plain_learner

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A                                               # what a list holds before the pack launch
TC_STATE = ("acc_abs", "E", "A", "tc_stats")
FULL_WAVE, FULL_CELLS = 8192, 512                                          # cells 8,192 .. 8,703: the first two wavefronts of tile 8, all four cells of all their lanes


def _launch_list(a, name, acc, acc_abs, words, capacity, stats=None, n_entries=None):
    from pulselib_amd import _native
    o = _native.TfeNtAccList()
    o.n_entries, o.acc, o.acc_abs = acc.shape[0] if n_entries is None else n_entries, acc.data_ptr(), None if acc_abs is None else acc_abs.data_ptr()
    o.capacity, o.list, o.stats = capacity, words.data_ptr(), None if stats is None else stats.data_ptr()
    assert o.list % 32 == 0 and o.acc % 16 == 0
    a._launch(name, o)


def _pack(a, capacity, with_abs):
    """one pack launch into a list of `capacity` entries between guard words, full of PATTERN: (the list's words, its guards)"""
    import torch
    words, flat, g = guarded(torch.zeros(4 + 4 * capacity, dtype=torch.int64, device=a.device), PATTERN)
    _launch_list(a, PACK, a.acc, a.acc_abs if with_abs else None, words, capacity)
    return words.cpu().numpy(), [("list", flat, g)]


@pytest.fixture(scope="module")
def learnt():
    """(the agent, acc and acc_abs on the host, the mirror's entries with and without acc_abs): a real learn launch -- TD(.5) with the
    third accumulator -- on 8 games of 16 moves from zero weights, and on top by hand: cells 0, 255, 256 and the last, a whole
    wavefront of live cells, and a visited cell whose differences cancel"""
    import torch
    a = learner_agent(8, extra_buffers=TC_STATE, tuples=TUPLES, max_steps=16, lam=LAM, tc=True)
    a.rollout()
    a.learn_tc_launch(LAM)
    W = a.total_weights
    assert W == 1188368 and W % 1024 and W % 256
    by_hand = {0: (11, 1, 11), 255: (-7, 2, 9), 256: (13, 3, 13), W - 1: (-(1 << 40), 5, 1 << 41), 100003: (0, 2, 6 << 16)}
    by_hand.update({FULL_WAVE + i: (i - 100, 1 + i % 3, 200 + i) for i in range(FULL_CELLS)})
    at = torch.tensor(sorted(by_hand), device=a.device)
    a.acc[at] = torch.tensor([by_hand[i][:2] for i in sorted(by_hand)], dtype=torch.int64, device=a.device)
    a.acc_abs[at] = torch.tensor([by_hand[i][2] for i in sorted(by_hand)], dtype=torch.int64, device=a.device)
    acc, ab = a.acc.cpu().numpy(), a.acc_abs.cpu().numpy()
    with_abs, without = nt().pack_acc_on_host(acc, ab), nt().pack_acc_on_host(acc)
    assert len(with_abs) > FULL_CELLS + 5 + 100 and a.stats()["learnt"] > 50          # (the launch learnt: the cells are not only the hand-made ones)
    assert set(by_hand) <= set(with_abs[:, 0].tolist()) and with_abs[with_abs[:, 0] == 100003].tolist() == [[100003, 0, 2, 6 << 16]]
    return a, acc, ab, with_abs, without


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("with_abs", (True, False))
def test_pack_is_the_mirror_s_set(learnt, with_abs):
    a, acc, ab, *mirrors = learnt
    want = mirrors[0] if with_abs else mirrors[1]
    found = len(want)
    print("cells", len(acc), "found", found)
    # capacity == found: the header {found, found}, the mirror's set
    words, guards = _pack(a, found, with_abs)
    assert words[:4].tolist() == [found, found, 0, 0] and np.array_equal(by_index(words[4:]), want)
    guards_intact(guards, a)
    # room to spare: the slots beyond `found` keep what they held; packing again gives the same set
    roomy, guards = _pack(a, found + 7, with_abs)
    assert roomy[:4].tolist() == [found, found, 0, 0] and np.array_equal(by_index(roomy[4:4 + 4 * found]), want)
    assert (roomy[4 + 4 * found:] == PATTERN).all()
    guards_intact(guards, a)
    # capacity == found - 1: one entry is counted and not written, every written one is a true one, nothing is written behind the list
    short, guards = _pack(a, found - 1, with_abs)
    assert short[:4].tolist() == [found, found - 1, 0, 0]
    got = by_index(short[4:])
    assert len(np.unique(got[:, 0])) == found - 1 and np.isin(got[:, 0], want[:, 0]).all()
    assert np.array_equal(got, want[np.isin(want[:, 0], got[:, 0])])
    guards_intact(guards, a)
    # one entry of room, and the accumulators are only read
    one, guards = _pack(a, 1, with_abs)
    assert one[:4].tolist() == [found, 1, 0, 0] and (want == one[4:8]).all(axis=1).sum() == 1
    guards_intact(guards, a)
    assert np.array_equal(a.acc.cpu().numpy(), acc) and np.array_equal(a.acc_abs.cpu().numpy(), ab)


# ------------------------------------------------------------------ unpack
N_CELLS = 5000


def _cells(a, seed):
    """non-zero acc int64[N_CELLS, 2] and acc_abs int64[N_CELLS] between guard words, and their host copies"""
    import torch
    rng = np.random.default_rng(seed)
    acc, ab = rng.integers(-10 ** 9, 10 ** 9, (N_CELLS, 2)), rng.integers(0, 10 ** 9, N_CELLS)
    dev = [guarded(torch.from_numpy(x).to(a.device)) for x in (acc, ab)]
    stats, sflat, sg = guarded(torch.zeros(2, dtype=torch.int64, device=a.device))
    guards = [("acc", dev[0][1], dev[0][2]), ("acc_abs", dev[1][1], dev[1][2]), ("stats", sflat, sg)]
    return acc, ab, dev[0][0], dev[1][0], stats, guards


def _list_on_device(a, words):
    import torch
    dev, flat, g = guarded(torch.from_numpy(words).to(a.device))
    return dev, [("list", flat, g)]


def _entries(rng, k, lo, hi):
    idx = rng.choice(np.arange(lo, hi), k, replace=False)
    return np.stack([idx, rng.integers(-10 ** 12, 10 ** 12, k), rng.integers(1, 99, k), rng.integers(0, 10 ** 12, k)], axis=1)


def test_unpack_adds_two_overlapping_lists(learnt):
    """700 and 900 entries (three and four workgroups, the last ragged) whose indices overlap on 2,000 .. 2,999, one launch behind the
    other, into non-zero accumulators; then a list with the same index twice; then without acc_abs"""
    a, rng = learnt[0], np.random.default_rng(5)
    acc, ab, dacc, dab, stats, guards = _cells(a, 1)
    first, second = _entries(rng, 700, 0, 3000), _entries(rng, 900, 2000, N_CELLS)
    assert len(np.intersect1d(first[:, 0], second[:, 0])) > 50
    twice = np.array([[0, 5, 1, 2], [N_CELLS - 1, -6, 2, 3], [0, 7, 4, 8]])
    lists = [(_list_on_device(a, list_words(e, cap)), cap) for e, cap in ((first, 700), (second, 1000), (twice, 3))]
    for (words, _), cap in lists:
        _launch_list(a, UNPACK, dacc, dab, words, cap, stats)
    for e in (first, second, twice):
        assert nt().unpack_acc_on_host(acc, ab, e) == (len(e), 0)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab) and stats.cpu().tolist() == [1603, 0]
    for ((words, lg), cap), e in zip(lists, (first, second, twice)):
        assert np.array_equal(words.cpu().numpy(), list_words(e, cap))      # a list is only read
        guards_intact(lg)
    (words, lg), cap = lists[0]
    _launch_list(a, UNPACK, dacc, None, words, cap, stats)                  # no acc_abs: sum and cnt only
    nt().unpack_acc_on_host(acc, None, first)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab) and stats.cpu().tolist() == [2303, 0]
    guards_intact(guards, lg)


def test_unpack_refuses_what_it_must_not_add(learnt):
    """entries are tested before memory is touched: index == n_entries (the word behind acc is a guard word), an index beyond, a
    negative one, cnt 0 and cnt < 0 add nothing and are counted, the good entries beside them are added; written = 0 adds nothing;
    written > capacity refuses the list whole"""
    a, rng = learnt[0], np.random.default_rng(6)
    acc, ab, dacc, dab, stats, guards = _cells(a, 2)
    good = _entries(rng, 300, 0, N_CELLS)
    bad = np.array([[N_CELLS, 1, 1, 1], [N_CELLS + 1, 1, 1, 1], [1 << 40, 1, 1, 1], [-1, 1, 1, 1], [5, 9, 0, 9], [6, 9, -2, 9]])
    mixed = np.vstack([good[:150], bad, good[150:]])
    words, lg = _list_on_device(a, list_words(mixed, 400))
    _launch_list(a, UNPACK, dacc, dab, words, 400, stats)
    assert nt().unpack_acc_on_host(acc, ab, mixed) == (300, 6)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab) and stats.cpu().tolist() == [300, 6]
    guards_intact(guards, lg)
    for header in (dict(found=300, written=0), dict(found=0, written=0)):  # nothing is added, nothing is counted
        words, lg = _list_on_device(a, list_words(good, 300, **header))
        _launch_list(a, UNPACK, dacc, dab, words, 300, stats)
        assert np.array_equal(dacc.cpu().numpy(), acc) and stats.cpu().tolist() == [300, 6]
    for written in (301, 1 << 40, -1):                                      # a header that says more than the list holds: stats[1] += capacity
        words, lg = _list_on_device(a, list_words(good, 300, written=written))
        _launch_list(a, UNPACK, dacc, dab, words, 300, stats)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab) and stats.cpu().tolist() == [300, 6 + 900]
    words, lg = _list_on_device(a, list_words(good, 300, written=200))      # written below the entries there are: the first 200
    _launch_list(a, UNPACK, dacc, dab, words, 300, stats)
    assert nt().unpack_acc_on_host(acc, ab, good[:200]) == (200, 0)
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab) and stats.cpu().tolist() == [500, 906]
    guards_intact(guards, lg)


def test_pack_then_unpack_into_zeroed_accumulators_round_trips(learnt):
    """the exchange's two launches back to back: the packed list of the learnt accumulators, added to zeroed ones, gives them again"""
    import torch
    a, acc, ab, want, _ = learnt
    found = len(want)
    words, flat, g = guarded(torch.zeros(4 + 4 * found, dtype=torch.int64, device=a.device), PATTERN)
    _launch_list(a, PACK, a.acc, a.acc_abs, words, found)
    acc2, f2, g2 = guarded(torch.zeros_like(a.acc))
    ab2, f3, g3 = guarded(torch.zeros_like(a.acc_abs))
    stats = torch.zeros(2, dtype=torch.int64, device=a.device)
    _launch_list(a, UNPACK, acc2, ab2, words, found, stats)
    live = acc[:, 1] > 0
    got, got_abs = acc2.cpu().numpy(), ab2.cpu().numpy()
    assert np.array_equal(got[live], acc[live]) and np.array_equal(got_abs[live], ab[live]) and not got[~live].any() and not got_abs[~live].any()
    assert stats.cpu().tolist() == [found, 0]
    guards_intact([("list", flat, g), ("acc2", f2, g2), ("abs2", f3, g3)], a)


# ------------------------------------------------------------------ synthetic buffers: the grid-stride loops turn, tiny counts, contended adds
# Both entry points take a raw pointer and n_entries, so these need no agent.  Both grids are capped at eight workgroups per compute unit.
def _cap():
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _on_device(x):
    """a host array on the device between guard words: (the tensor, its guards)"""
    import torch
    dev, flat, g = guarded(torch.from_numpy(x).to("cuda:0"))
    return dev, [("buffer", flat, g)]


def _pack_into(a, acc, ab, capacity, n_entries=None, words=None):
    """one pack launch of the device tensors acc (and ab, or None) into a list of `capacity` entries full of PATTERN between guard
    words (or into `words`, refilled): (the list's words on the host, its guards, the device tensor)"""
    import torch
    guards = []
    if words is None:
        words, flat, g = guarded(torch.zeros(4 + 4 * capacity, dtype=torch.int64, device=a.device), PATTERN)
        guards = [("list", flat, g)]
    else:
        words.fill_(PATTERN)
    _launch_list(a, PACK, acc, ab, words, capacity, n_entries=n_entries)
    return words.cpu().numpy(), guards, words


@pytest.fixture(scope="module")
def multi_pass():
    """(the launcher, the cap, acc and acc_abs on the host and on the device between guard words, their guards, the mirror's entries with
    and without acc_abs) of multi_pass_accumulators: about 4.2 M cells at a cap of 2,048, 67 MB + 34 MB.  The pass counts the size is
    chosen for are asserted, so a device with another count of compute units turns the loops as often or fails here."""
    a, cap = device_launcher(), _cap()
    acc, ab, tiles = multi_pass_accumulators(cap)
    n = len(acc)
    n_tiles = -(-n // TILE)
    print("compute units", cap // 8, "cap", cap, "cells", n, "tiles", n_tiles)
    assert n == (2 * cap + 1) * TILE + 517 and n_tiles == 2 * cap + 2 and passes(n, TILE, cap) == 3
    assert [len(range(b, n_tiles, cap)) for b in (0, 1, 2, cap - 1)] == [3, 3, 2, 2]                 # workgroups 0 and 1 go round three times, every other twice
    with_abs, without = nt().pack_acc_on_host(acc, ab), nt().pack_acc_on_host(acc)
    per_tile = np.bincount(with_abs[:, 0] // TILE, minlength=n_tiles)
    assert {t: int(per_tile[t]) for t in tiles} == tiles and len(with_abs) > 3 * TILE + 5000
    assert {0, n - 1} <= set(with_abs[:, 0].tolist()) and (with_abs[:, 1] < 0).sum() > 1000 and (with_abs[:, 1] > 0).sum() > 1000
    dead = np.flatnonzero((acc[:, 1] <= 0) & (acc[:, 0] != 0))
    assert len(dead) > 500 and sorted(set(map(tuple, acc[dead].tolist()))) == sorted(DEAD) and not np.isin(dead, with_abs[:, 0]).any()
    assert np.isin(dead // TILE, [cap, 1, 2 * cap + 1]).sum() >= 4                                   # some of them where a tile has no live cell, and in the ragged one
    (dacc, g1), (dab, g2) = _on_device(acc), _on_device(ab)
    return a, cap, acc, ab, dacc, dab, g1 + g2, with_abs, without


@pytest.mark.parametrize("with_abs", (True, False))
def test_pack_goes_round_its_grid_three_times(multi_pass, with_abs):
    """2 cap + 2 tiles under a grid of cap workgroups: the LDS words of either parity are written a second time, a workgroup skips its
    atomic in one pass and takes 1,024 slots in the next.  capacity == found: the mirror's set; 1,000 short: 1,000 entries are counted
    and not written, and every written one is the mirror's.  (Tried once on an MI355X: the kernel without its second barrier fails here,
    slots taken from a wg_base not yet written.  Without `parity ^= 1u` it passes: that only opens a race -- a wavefront a pass ahead
    would overwrite wave_total while a slower one still sums it for its slot0, but it first waits for its four loads from memory, far
    longer than the few LDS reads it would have to overtake -- so the double buffer rests on the argument in the kernel, not on a test.)"""
    a, cap, acc, ab, dacc, dab, guards, *mirrors = multi_pass
    want = mirrors[0] if with_abs else mirrors[1]
    found = len(want)
    print("found", found)
    words, lg, _ = _pack_into(a, dacc, dab if with_abs else None, found)
    assert words[:4].tolist() == [found, found, 0, 0]
    assert np.array_equal(by_index(words[4:]), want)
    guards_intact(lg, guards)
    assert found > 2000
    short, lg, _ = _pack_into(a, dacc, dab if with_abs else None, found - 1000)
    assert short[:4].tolist() == [found, found - 1000, 0, 0]
    got = by_index(short[4:])
    assert len(got) == found - 1000 and len(np.unique(got[:, 0])) == found - 1000                     # distinct indices
    at = np.searchsorted(want[:, 0], got[:, 0])
    assert (at < found).all() and np.array_equal(want[np.minimum(at, found - 1)], got)              # each is the mirror's entry of its index
    guards_intact(lg, guards)                                                                        # nothing lies beyond the list
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab)         # the accumulators are only read


def test_pack_at_tiny_and_boundary_counts():
    """n_entries of TINY under TINY_PATTERNS, one pair of buffers of three tiles for all of them: whole wavefronts -- at n_entries 1, all
    but one lane -- read only the clamped last cell, which must not be counted again; the cells from n_entries on are live decoys."""
    import torch
    a, cells = device_launcher(), -(-max(TINY) // TILE) * TILE
    dacc, g1 = _on_device(np.zeros((cells, 2), dtype=np.int64))
    dab, g2 = _on_device(np.zeros(cells, dtype=np.int64))
    words, flat, g = guarded(torch.zeros(4 + 4 * cells, dtype=torch.int64, device=a.device), PATTERN)
    for n in TINY:
        for which in TINY_PATTERNS:
            acc, ab = tiny_accumulators(n, which, cells)
            dacc.copy_(torch.from_numpy(acc))
            dab.copy_(torch.from_numpy(ab))
            want = nt().pack_acc_on_host(acc[:n], ab[:n])
            assert len(want) == dict(all=n, last=1, first=1, none=0)[which]
            got, _, _ = _pack_into(a, dacc, dab, cells, n_entries=n, words=words)
            assert got[:4].tolist() == [len(want), len(want), 0, 0], (n, which, got[:4].tolist())
            assert np.array_equal(by_index(got[4:4 + 4 * len(want)]), want), (n, which)
            assert (got[4 + 4 * len(want):] == PATTERN).all(), (n, which)                            # (no cell live: the whole body)
            assert np.array_equal(dacc.cpu().numpy(), acc), (n, which)
    guards_intact(g1, g2, [("list", flat, g)])


@pytest.mark.parametrize("with_abs", (True, False))
def test_unpack_goes_round_its_grid_on_contended_cells(with_abs):
    """2 cap * 256 + 77 entries under a grid of cap workgroups: every lane adds two entries, the first 77 three; one entry in eight adds
    into one of four cells, 300 are refused in place.  acc, acc_abs and the two counters equal numpy's add.at and its count."""
    a, cap, rng = device_launcher(), _cap(), np.random.default_rng(8)
    k = 2 * cap * BLOCK + 77
    assert -(-k // BLOCK) == 2 * cap + 1 > cap and passes(k, BLOCK, cap) == 3 and len(range(77, k, cap * BLOCK)) == 2
    print("cap", cap, "entries", k)
    entries, n_bad = contended_entries(k, N_CELLS, rng)
    assert (np.bincount(entries[:, 0][(entries[:, 0] >= 0) & (entries[:, 0] < N_CELLS)], minlength=N_CELLS)[[0, 1234, 2500, N_CELLS - 1]] > k // 40).all()
    acc, ab, dacc, dab, stats, guards = _cells(a, 4)
    before_abs = ab.copy()
    host_words = list_words(entries, k)
    words, lg = _list_on_device(a, host_words)
    _launch_list(a, UNPACK, dacc, dab if with_abs else None, words, k, stats)
    assert nt().unpack_acc_on_host(acc, ab if with_abs else None, entries) == (k - n_bad, n_bad)
    assert stats.cpu().tolist() == [k - n_bad, n_bad]
    assert np.array_equal(dacc.cpu().numpy(), acc) and np.array_equal(dab.cpu().numpy(), ab)
    assert with_abs or np.array_equal(ab, before_abs)
    assert np.array_equal(words.cpu().numpy(), host_words)                                           # the list is only read
    guards_intact(guards, lg)


def test_multi_pass_pack_then_unpack_round_trips(multi_pass):
    """the list of the multi-pass buffer, added into zeroed accumulators of its size: the live cells again, zeros elsewhere"""
    import torch
    a, cap, acc, ab, dacc, dab, guards, want, _ = multi_pass
    found = len(want)
    _, lg, words = _pack_into(a, dacc, dab, found)
    acc2, f2, g2 = guarded(torch.zeros_like(dacc))
    ab2, f3, g3 = guarded(torch.zeros_like(dab))
    stats = torch.zeros(2, dtype=torch.int64, device=a.device)
    _launch_list(a, UNPACK, acc2, ab2, words, found, stats)
    live = acc[:, 1] > 0
    got, got_abs = acc2.cpu().numpy(), ab2.cpu().numpy()
    assert stats.cpu().tolist() == [found, 0] and live.sum() == found
    assert np.array_equal(got[live], acc[live]) and np.array_equal(got_abs[live], ab[live]) and not got[~live].any() and not got_abs[~live].any()
    guards_intact(lg, guards, [("acc2", f2, g2), ("abs2", f3, g3)])


def test_the_entry_points_refuse():
    assert_list_refusals()




# ------------------------------------------------------------------ rounds: a world of one, and two ranks on one device
CASES = (("td0", dict(), dict(), None),                                    # (name, the agent's keywords, its attributes, exchange_capacity)
         ("tc", dict(lam=LAM, tc=True), dict(), None),
         ("continue", dict(max_steps=8), dict(continue_games=True), None),
         ("dense", dict(lam=LAM, tc=True), dict(), 3),
         # every other option the docstrings name beside a shard; tests/test_tfe_nt_ranks_cpu.py plays their regimes on the host
         ("lambda", dict(lam=LAM), dict(), None),
         ("staged", dict(stage_tiles=STAGE_TILES, lam=LAM, tc=True), dict(), None),
         ("staged-grown", dict(stage_tiles=GROWN_FROM), dict(), None),             # add_stage(GROWN_TILE) behind round 1: acc is reallocated under the shard
         ("restart", dict(), dict(RESTART), None),
         ("backed", dict(lam=LAM), dict(rollout_layers=1, backed_targets=True), None),
         ("search2", dict(), dict(rollout_layers=2), None),
         ("adaptive", dict(), dict(RESTART, rollout_layers=2, rollout_deep_empty_max=DEEP_EMPTY_MAX, backed_targets=True), None),
         ("resume", dict(lam=LAM, tc=True), dict(), None))                           # save() behind round 1, load() + set_shard, round 2
GROW_BEHIND = 1


def _sparse(x):
    """(the positions of the words that are not all zero bits, those words): an array for the comparison, small"""
    b = np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)
    at = np.flatnonzero(b)
    return at, b[at]


def _same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def _file_words(path):
    """an .npz as {name: (dtype, shape, bytes)}"""
    with np.load(path) as f:
        return {k: (str(f[k].dtype), f[k].shape, f[k].tobytes()) for k in f.files}


def _resumed(a, attrs, capacity, tmp, rank):
    """every rank saves; every rank loads RANK 0's file with its own share of the games and sets the shard again: (the loaded agent,
    the exchange summary of the agent it replaces, this rank's file)"""
    import torch.distributed as dist
    a.save(os.path.join(tmp, "rank%d.npz" % rank))
    dist.barrier()
    b = type(a).load(os.path.join(tmp, "rank0.npz"), a.device, n_games=a.n_games)
    for k, v in attrs.items():
        setattr(b, k, v)
    b.set_shard(a._shard.n_games_total, a._shard.game0, exchange_capacity=capacity)
    return b, a.exchange_summary(), _file_words(os.path.join(tmp, "rank%d.npz" % rank))


def _rounds(case, n_games, game0, sharded, tmp=None, rank=0):
    """three rounds of the case on `n_games` games that begin at game `game0` of the job's 13: (the agent, what it read back)"""
    name, kw, attrs, capacity = case
    a = plain_learner(n_games, **dict(dict(tuples=TUPLES, max_steps=MAX_STEPS), **kw))
    for k, v in attrs.items():
        setattr(a, k, v)
    if sharded:
        a.set_shard(GAMES, game0, exchange_capacity=capacity)
    out, before = dict(restarts=[]), None
    for r in range(ROUNDS):
        if name == "resume" and sharded and tmp is not None and r == ROUNDS - 1:
            a, before, out["file"] = _resumed(a, attrs, capacity, tmp, rank)
            assert a.round == ROUNDS - 1 and a.n_games == n_games
        a.learn_batch()
        if a.restart_fraction > 0.0:
            out["restarts"].append(a.restart_summary())                    # (with a shard: job-wide)
        if name == "staged-grown" and r == GROW_BEHIND:
            a.add_stage(GROWN_TILE)
    out.update(weights=_sparse(a.weights()), stats=a.stats(), round=a.round, stages=(a.n_stages, a.n_weights))
    if a.tc:
        E, A = a.coherence()
        out.update(E=_sparse(E), A=_sparse(A), tc=a.tc_summary())
    if a.continue_games:
        out["finished"] = a.finished_summary()
    if a.rollout_deep_empty_max is not None:                                # the rounds' depth words, then the evaluation's: job-wide with a shard
        out["depth"] = a.rollout_depth_summary()
        out["evaluate_adaptive"] = a.evaluate_search(n_games=EVAL_GAMES, layers=2, deep_empty_max=DEEP_EMPTY_MAX)
    if sharded:
        out["exchange"] = a.exchange_summary()
        if before is not None:                                              # the rounds of the agent that was saved, then the loaded one's
            out["exchange"] = {k: before[k] + out["exchange"][k] for k in ("rounds", "added", "refused")}
    return a, out


def _all_cases(n_games, game0, sharded, tmp=None, rank=0):
    out = {}
    for case in CASES:
        name = case[0]
        a, out[name] = _rounds(case, n_games, game0, sharded, tmp, rank)
        if name == "tc":                                                    # the trained network's evaluations: 11 games, job-wide
            out["evaluate"] = a.evaluate(n_games=EVAL_GAMES)
            out["evaluate_search"] = a.evaluate_search(n_games=EVAL_GAMES)
            own = a.evaluate(n_games=EVAL_GAMES, per_game=True)
            out["per_game"] = (own["total_score"], own["lengths"])
    return out


def _assert_case(got, want, where):
    assert got["round"] == want["round"] == ROUNDS and got["stats"] == want["stats"], where
    for k in ("weights", "E", "A"):
        assert (k in got) == (k in want) and (k not in got or _same(got[k], want[k])), (where, k)
    for k in ("tc", "finished"):
        assert got.get(k) == want.get(k), (where, k)
    assert len(got["weights"][0]) >= len(TUPLES) and want["stats"]["learnt"] > 100, where      # (a learnt move reads a cell of every tuple's table)


def test_a_world_of_one_is_the_agent_without_the_shard():
    """set_shard(n, 0) and no group: three rounds of TD(.5) with temporal coherence; weights, E and A bit for bit those of the agent
    without the shard; the summary names the sparse path, counts the entries and moves no byte"""
    _, want = _rounds(CASES[1], GAMES, 0, False)
    _, got = _rounds(CASES[1], GAMES, 0, True)
    _assert_case(got, want, "world of one")
    rounds = got["exchange"]["rounds"]
    assert [r["round"] for r in rounds] == [0, 1, 2] and all(r["path"] == "sparse" and r["bytes"] == 0 and r["entries"][0] > 100 for r in rounds)
    assert (got["exchange"]["added"], got["exchange"]["refused"]) == (0, 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, tmp, out):
    import torch.distributed as dist
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    ranks.init_ranks("gloo", rank, world)
    try:
        n_games, game0 = ranks.shard_of(GAMES)
        out[rank] = dict(_all_cases(n_games, game0, True, tmp, rank), shard=(n_games, game0))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_device_equal_one_process(tmp_path):
    """One spawn of two fresh processes (three with this one) for all the cases: each rank's weights -- and E, A, the job-wide stats(),
    finished_summary() and tc_summary() where the case has them -- equal one process's on 13 games exactly, the ranks equal each
    other, and the summary names the path: dense with room for 3 entries, sparse in every other case.  evaluate(n_games=11) and
    evaluate_search on the two ranks give the single process's summary and histogram word for word.  Beyond the first four cases:
    TD(.5) without tc; stages (two of them learnt in); a stage added between two rounds, so that the exchange meets a reallocated acc;
    restarts, with restart_summary() after every round; search-backed targets under one chance layer; roll-outs two layers deep; the
    adaptive depth with backed targets and restarts, with rollout_depth_summary() and the adaptive evaluate_search, whose depth words
    are the job's; and a run saved by both ranks behind round 1 and taken up from rank 0's file."""
    import torch.multiprocessing as mp
    want = _all_cases(GAMES, 0, False)
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), out), nprocs=2, join=True)
    got = [out[0], out[1]]
    assert [g["shard"] for g in got] == [(7, 0), (6, 7)]
    for name, *_ in CASES:
        for rank in range(2):
            if name == "resume":                                            # (stats() and tc_summary() are the agent's, not the file's: a loaded agent counts from 0)
                assert got[rank][name]["round"] == want[name]["round"] == ROUNDS and all(_same(got[rank][name][k], want[name][k]) for k in ("weights", "E", "A")), rank
                assert len(got[rank][name]["weights"][0]) >= len(TUPLES) and want[name]["stats"]["learnt"] > 100
            else:
                _assert_case(got[rank][name], want[name], (name, rank))
            rounds = got[rank][name]["exchange"]["rounds"]
            assert [r["round"] for r in rounds] == list(range(ROUNDS)), (name, rank)
            assert [r["path"] for r in rounds] == ["dense" if name == "dense" else "sparse"] * ROUNDS, (name, rank)
            assert all(len(r["entries"]) == 2 and min(r["entries"]) >= len(TUPLES) for r in rounds) and got[rank][name]["exchange"]["refused"] == 0
            added = sum(r["entries"][1 - rank] for r in rounds)
            assert got[rank][name]["exchange"]["added"] == (0 if name == "dense" else added), (name, rank)
        assert _same(got[0][name]["weights"], got[1][name]["weights"]) and got[0][name]["exchange"]["rounds"] == got[1][name]["exchange"]["rounds"]
    assert want["continue"]["finished"]["continued"] > 0
    for k in ("evaluate", "evaluate_search"):
        assert got[0][k] == got[1][k] == want[k] and want[k]["games"] == EVAL_GAMES and sum(want[k]["max_tile_hist"]) == EVAL_GAMES, k
    # per_game: the rank's own share of the 11 games, in order
    assert [len(g["per_game"][0]) for g in got] == [6, 5]
    for i in range(2):
        assert np.array_equal(np.concatenate([g["per_game"][i] for g in got]), want["per_game"][i])
    # stages: weights that are not zero in at least two of the three, and after the split in the stage that was added
    for name, n_stages in (("staged", 3), ("staged-grown", 3)):
        assert want[name]["stages"] == got[0][name]["stages"] == got[1][name]["stages"] == (n_stages, 1188368)
        assert len(np.unique(want[name]["weights"][0] // 1188368)) >= 2, name
    # restarts: the job's picks and started games after every round
    for name in ("restart", "adaptive"):
        assert got[0][name]["restarts"] == got[1][name]["restarts"] == want[name]["restarts"] and len(want[name]["restarts"]) == ROUNDS, name
        assert all(s["picked"] > 0 and s["mean_depth"] > 0 for s in want[name]["restarts"][:2]) and all(s["started"] > 0 for s in want[name]["restarts"][1:]), name
    # the adaptive depth: both words move, and they are the job's on either rank, the evaluation's too
    depth, ev = want["adaptive"]["depth"], want["adaptive"]["evaluate_adaptive"]
    assert got[0]["adaptive"]["depth"] == got[1]["adaptive"]["depth"] == depth and depth["moves_deep"] > 0 and depth["moves_shallow"] > 0
    assert depth["moves_deep"] + depth["moves_shallow"] == want["adaptive"]["stats"]["moves"]
    assert got[0]["adaptive"]["evaluate_adaptive"] == got[1]["adaptive"]["evaluate_adaptive"] == ev
    assert ev["games"] == EVAL_GAMES and ev["moves_deep"] > 0 and ev["moves_shallow"] > 0 and ev["moves_deep"] + ev["moves_shallow"] == ev["moves"]
    assert (depth, (ev["moves_deep"], ev["moves_shallow"])) == (ADAPTIVE_REHEARSED["rounds"], ADAPTIVE_REHEARSED["evaluation"])      # the host's, played ahead
    # resume: the two files differ in n_games alone
    files = [g["resume"]["file"] for g in got]
    assert sorted(files[0]) == sorted(files[1]) and {"n_games", "round", "index", "value"} <= set(files[0])
    assert [k for k in files[0] if files[0][k] != files[1][k]] == ["n_games"]
    assert [np.frombuffer(f["n_games"][2], dtype=f["n_games"][0]).tolist() for f in files] == [[7], [6]]
    assert np.frombuffer(files[0]["round"][2], dtype=files[0]["round"][0]).tolist() == [ROUNDS - 1] and len(files[0]["index"][2]) > 8 * len(TUPLES)
