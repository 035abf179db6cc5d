"""The 2048 n-tuple network's rank-parallel rounds on the device (csrc/tfe_ntuple_exchange.hip:
pulse_tfe_nt_acc_pack, pulse_tfe_nt_acc_unpack) against the host's pack and unpack, and two gloo ranks on one device against one
process on all the games.  Every comparison is exact: integers word for word, float32 and float64 as bit patterns.  Every buffer a
launch is handed sits between guard words.

Shapes: the network "eight" of tests/tfe_nt_support.py, 1,188,368 cells -- no multiple of the pack's 1,024-cell tile nor of 256, so
the last workgroup is ragged and the launch takes 1,161 tiles --; the accumulators of a real learn launch on 8 games of 16 moves
with cells set by hand on top; for the ranks 13 games (7 + 6) of at most 24 moves, 3 rounds, epsilon .25."""
import os
import socket

import numpy as np
import pytest

from tests.tfe_gpu_support import guarded, guards_intact
from tests.tfe_nt_ranks_support import GAMES, LAM, MAX_STEPS, PACK, ROUNDS, TUPLES, UNPACK, assert_list_refusals, by_index, list_words
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


def test_the_entry_points_refuse():
    assert_list_refusals()


# ------------------------------------------------------------------ rounds: a world of one, and two ranks on one device
CASES = (("td0", dict(), dict(), None),                                    # (name, the agent's keywords, its attributes, exchange_capacity)
         ("tc", dict(lam=LAM, tc=True), dict(), None),
         ("continue", dict(max_steps=8), dict(continue_games=True), None),
         ("dense", dict(lam=LAM, tc=True), dict(), 3))
EVAL_GAMES = 11


def _sparse(x):
    """(the positions of the words that are not all zero bits, those words): an array for the comparison, small"""
    b = np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)
    at = np.flatnonzero(b)
    return at, b[at]


def _same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def _rounds(n_games, game0, kw, attrs, capacity, sharded):
    """three rounds of the case on `n_games` games that begin at game `game0` of the job's 13: (the agent, what it read back)"""
    a = plain_learner(n_games, **dict(dict(tuples=TUPLES, max_steps=MAX_STEPS), **kw))
    for k, v in attrs.items():
        setattr(a, k, v)
    if sharded:
        a.set_shard(GAMES, game0, exchange_capacity=capacity)
    for _ in range(ROUNDS):
        a.learn_batch()
    out = dict(weights=_sparse(a.weights()), stats=a.stats(), round=a.round)
    if a.tc:
        E, A = a.coherence()
        out.update(E=_sparse(E), A=_sparse(A), tc=a.tc_summary())
    if a.continue_games:
        out["finished"] = a.finished_summary()
    if sharded:
        out["exchange"] = a.exchange_summary()
    return a, out


def _all_cases(n_games, game0, sharded):
    out = {}
    for name, kw, attrs, capacity in CASES:
        a, out[name] = _rounds(n_games, game0, kw, attrs, capacity, sharded)
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
    name, kw, attrs, capacity = CASES[1]
    _, want = _rounds(GAMES, 0, kw, attrs, capacity, False)
    _, got = _rounds(GAMES, 0, kw, attrs, capacity, True)
    _assert_case(got, want, "world of one")
    rounds = got["exchange"]["rounds"]
    assert [r["round"] for r in rounds] == [0, 1, 2] and all(r["path"] == "sparse" and r["bytes"] == 0 and r["entries"][0] > 100 for r in rounds)
    assert (got["exchange"]["added"], got["exchange"]["refused"]) == (0, 0)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    ranks.init_ranks("gloo", rank, world)
    try:
        n_games, game0 = ranks.shard_of(GAMES)
        out[rank] = dict(_all_cases(n_games, game0, True), shard=(n_games, game0))
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_device_equal_one_process():
    """One spawn of two fresh processes (three with this one) for all four cases: each rank's weights -- and E, A, the job-wide stats(),
    finished_summary() and tc_summary() where the case has them -- equal one process's on 13 games exactly, the ranks equal each
    other, and the summary names the path: sparse in the first three cases, dense with room for 3 entries.  evaluate(n_games=11) and
    evaluate_search on the two ranks give the single process's summary and histogram word for word."""
    import torch.multiprocessing as mp
    want = _all_cases(GAMES, 0, False)
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [out[0], out[1]]
    assert [g["shard"] for g in got] == [(7, 0), (6, 7)]
    for name, *_ in CASES:
        for rank in range(2):
            _assert_case(got[rank][name], want[name], (name, rank))
            rounds = got[rank][name]["exchange"]["rounds"]
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
