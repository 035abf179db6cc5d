"""The tabular Q-learner without a GPU: the host mirror (tests/qtable_host.py) against the reference replay it generalises, the
conditions under which the GPU tests' cases reach the paths they are for, the sensitivity of the shared table's checks to one lost
update, and the refusals of pulse_qtable_select / _update / _rollout_step (all of them return before any HIP call)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import qtable_host as qh
from tests import tfe_host


# ------------------------------------------------------------------ the mirror against the reference replay
@pytest.mark.parametrize("n,B,steps", [(4, 48, 60), (3, 40, 40)])
def test_unbounded_mirror_equals_the_reference_replay(n, B, steps):
    """Without a capacity the mirror is the replay of test_batched_q_learning_matches_reference_semantics_per_board (one dict per
    board, the oracle's two helpers -- pinned to the reference by tests/test_reference_pins.py): same actions at every step, same
    boards, same tables bit for bit."""
    lib = orc.lib()
    host = qh.QLearningHost(B, n, None, **qh.CFG)
    boards, score = np.zeros((B, n, n), dtype=np.int32), np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, 77)
    tables = [dict() for _ in range(B)]

    def q_of(g, key):
        return tables[g].setdefault(key, np.zeros(4, dtype=np.float64))

    for s in range(steps):
        actions, keys = np.zeros(B, dtype=np.int64), [None] * B
        for g in range(B):
            w = orc.philox4x32(991, g, s)
            p = float(((int(w[0]) << 21) ^ (int(w[1]) >> 11)) * (1.0 / 9007199254740992.0))
            keys[g] = tfe_host.pack_boards(boards[g:g + 1])[0].item()
            actions[g] = lib.oracle_select_action_epsilon_greedy(q_of(g, keys[g]).ctypes.data_as(C.c_void_p), 4, C.c_double(0.1), C.c_double(p),
                                                                 C.c_uint32(int(w[2])))
        assert np.array_equal(host.step(s), actions), s
        orc.tfe_step(boards, score, actions, rewards, dones, n, 77, s + 1)
        assert np.array_equal(host.boards, boards) and np.array_equal(host.dones, dones) and np.array_equal(host.score, score), s
        for g in range(B):
            cur, nxt = q_of(g, keys[g]), q_of(g, tfe_host.pack_boards(boards[g:g + 1])[0].item())
            lib.oracle_update_q_entry(cur.ctypes.data_as(C.c_void_p), int(actions[g]), nxt.ctypes.data_as(C.c_void_p), 4, C.c_double(0.1),
                                      C.c_double(float(rewards[g])), C.c_double(0.99), int(dones[g]))
    for g in range(B):
        assert set(host.tables[g]) == set(tables[g]), g
        assert all(np.array_equal(host.tables[g][k].view(np.uint64), v.view(np.uint64)) for k, v in tables[g].items()), g
    got = host.summary()
    assert got["no_room_s"] == got["no_room_next"] == got["full_regions"] == 0 and got["nonzero_rows"] > B


def test_the_key_is_the_lossy_one_of_the_device():
    """4 bits of min(log2 tile, 15), cell 0 lowest: 1 and negatives read as empty, 3 as 2, 65,536 and 2^20 as 32,768 -- and the two
    host forms of it (one board here, many boards in tests/tfe_host.py) agree on every board of the unusual case."""
    key = qh.pack_board(np.array([[1, 3, 6, -2], [32768, 65536, 2 ** 20, 12], [5, 2, 4, 0], [16384, 8, 0, 2048]]))
    assert [(key >> (4 * i)) & 15 for i in range(16)] == [0, 1, 2, 0, 15, 15, 15, 3, 2, 1, 2, 0, 14, 3, 0, 11]
    boards = qh.unusual_boards()
    assert [qh.pack_board(b) for b in boards] == tfe_host.pack_boards(boards).tolist()


# ------------------------------------------------------------------ what the GPU tests' cases reach (conditions, not measurements)
def test_full_regions_are_reached_at_sixteen_slots():
    for name in ("3x3-full", "3x3-full-id1000"):
        got = qh.run_case(name)[0].summary()
        print(name, got)
        assert got["full_regions"] >= 150 and got["no_room_s"] >= 4000 and got["no_room_next"] >= 100, (name, got)
        assert got["terminal"] >= 200 and got["boards_done"] >= 100, (name, got)
        assert got["terminal_after_done"] >= 100, (name, got)                       # boards that go on stepping once they are over


def test_games_end_and_no_region_fills_at_256_slots():
    for name in ("3x3-room", "3x3-flipped"):
        got = qh.run_case(name)[0].summary()
        print(name, got)
        assert got["full_regions"] == 0 and got["no_room_s"] == 0 and got["no_room_next"] == 0, (name, got)
        assert got["boards_done"] >= 40 and got["terminal"] >= 1000 and got["nonzero_rows"] >= 1500, (name, got)
    # the flip changes the games: the carried entries of a fused run are stale afterwards, not by chance still right
    a, b = qh.run_case("3x3-room")[1], qh.run_case("3x3-flipped")[1]
    assert np.array_equal(a["boards"][:qh.FLIP_AFTER + 1], b["boards"][:qh.FLIP_AFTER + 1])
    assert (a["boards"][qh.FLIP_AFTER + 1] != b["boards"][qh.FLIP_AFTER + 1]).any(axis=(1, 2)).sum() >= 50


def _packable(boards):
    return ((boards >= 0) & (boards & (boards - 1) == 0) & (boards != 1) & (boards <= 16384)).all(axis=(-1, -2))


def test_unusual_case_sends_the_wavefronts_it_names_through_the_cell_form():
    """Per wavefront of 64 boards, at every step: 0 and 2 hold boards the packed form can (and so do 4, 6, 7); 1 holds exactly one it
    cannot; 3 only such; 5 is ordinary at step 0, where MERGER's move to the left makes two 32,768 tiles, and holds that one board
    the packed form cannot from then on.  No region comes near its 64 slots."""
    host, rec = qh.run_case("4x4-unusual")
    start = qh.unusual_boards()
    assert set(np.abs(start[192:256]).reshape(64, -1).max(axis=1).tolist()) >= {32768, 65536, 2 ** 20}
    for t, boards in enumerate([start] + list(rec["boards"][:-1])):                  # the boards step t starts from
        odd = (~_packable(boards)).reshape(8, 64)
        assert odd.sum(axis=1).tolist() == [0, 1, 0, 64, 0, int(t > 0), 0, 0], t
        assert odd[1, qh.LONE - 64] and (t == 0 or odd[5, qh.MERGER - 320]), t
    assert rec["actions"][0, qh.MERGER] == 0 and rec["boards"][0, qh.MERGER, 0].tolist() == [32768, 32768, 0, 0]
    assert rec["scores"][0, qh.MERGER] == 2 * 32768 + 4 + 8 + 16384
    got = host.summary()
    assert got["full_regions"] == 0 and max(len(t) for t in host.tables) <= 25 and got["terminal"] >= 100 and got["nonzero_rows"] >= 1000


# ------------------------------------------------------------------ the shared table's checks can fail
def _least_shift(B, alpha, rounds=3):
    """min over the rounds and the four cells of |value with k updates - value with k - 1| / tolerance, per round"""
    q, least = np.zeros(4), []
    for rnd in range(rounds):
        counts = np.bincount(qh.random_actions(qh.SHARED_SEED, 0, B, rnd), minlength=4)
        assert counts.min() > B // 8
        ratios = []
        for a, k in enumerate(counts.tolist()):
            t = a + 1.0
            want, lost = qh.combined(q[a], t, k, alpha), qh.combined(q[a], t, k - 1, alpha)
            ratios.append(abs(want - lost) / qh.combined_tolerance(k, t, q[a]))
            q[a] = want
        least.append(min(ratios))
    return least


@pytest.mark.parametrize("B,alpha", qh.SHARED_SENSITIVE, ids=["700", "1300", "66000-alpha-2^-16"])
def test_one_lost_update_moves_a_cell_by_ten_thousand_tolerances(B, alpha):
    """The figures of tests/test_qtable_gpu.py's contended cells: with k - 1 for k updates in any of the three rounds the expected
    value moves by more than 10^4 times the tolerance, for every action's cell -- (1 - alpha)^k stays above 0.4 over the three rounds."""
    least = _least_shift(B, alpha)
    print(B, alpha, "one lost update / tolerance >=", least)
    assert min(least) > 1e4


def test_sixty_six_thousand_boards_need_a_smaller_alpha_to_see_a_lost_update():
    """alpha = 2^-10 with 66,000 boards: a cell takes k = 16,500 updates per round and (1 - alpha)^k = 1e-7, so one lost update moves
    the first round's value by some ten tolerances and the later rounds' by nothing that float64 can hold -- which is why the GPU test
    runs that size with alpha = 2^-16 as well, (1 - alpha)^k = 0.78."""
    least = _least_shift(66000, 2.0 ** -10)
    print("66000 boards, alpha 2^-10: one lost update / tolerance >=", least)
    assert 1.0 < least[0] < 1e4 and least[1] < 1.0 and least[2] < 1.0
    assert (66000, 2.0 ** -16) in qh.SHARED_SENSITIVE


def test_one_lost_update_moves_the_mean_of_unequal_targets_by_ten_thousand_tolerances():
    """all B = 1,300 updates of one cell combined, targets 1 + (g mod 7): the mean rule over two rounds"""
    alpha, q0 = 2.0 ** -10, 0.0
    mean = float(np.sum(1 + np.arange(1300) % 7)) / 1300
    for rnd in range(2):
        want = qh.combined(q0, mean, 1300, alpha)
        ratio = abs(want - qh.combined(q0, mean, 1299, alpha)) / qh.combined_tolerance(1300, 7.0, q0)
        print("round", rnd, "one lost update / tolerance =", ratio)
        assert ratio > 1e4
        q0 = want


def test_random_actions_are_the_oracles_draws():
    got = qh.random_actions(1, 1000, 300, 2)
    assert got.tolist() == [(int(orc.philox4x32(1, 1000 + g, 2)[2]) * 4) >> 32 for g in range(300)]


# ------------------------------------------------------------------ refusals
def _aligned_words():
    raw = (C.c_char * 4096)()
    return raw, (C.addressof(raw) + 63) & ~63


def test_qtable_entry_points_refuse_bad_arguments_without_a_gpu():
    """check_table, the null checks and the scratch's checks (csrc/qtable.hip: deferred_of) all come before the first HIP call; the
    pointers are host words that no refusal reads.  No call here is a valid one."""
    from pulselib_amd import _native
    lib = _native.lib()
    keep, ptr = _aligned_words()
    B, n = 256, 4

    def table(entries=ptr, capacity=256 * 64, region_slots=64):
        return _native.QTable(entries, capacity, region_slots)

    def scratch(n=256, acc_slots=512, **null):
        fields = {k: (None if k in null else ptr) for k in ("count", "cells", "targets", "owner", "acc_key", "acc_cnt", "acc_sum")}
        return _native.QTableScratch(*(fields[k] for k in ("count", "cells", "targets", "owner", "acc_key", "acc_cnt", "acc_sum")), n, acc_slots)

    def select(q, boards=ptr, n_boards=B, side=n, actions=ptr, slots=ptr):
        return lib.pulse_qtable_select(C.byref(q) if q is not None else None, boards, n_boards, side, 0.1, 1, 0, 0, actions, slots, None)

    def update(q, sc=None, slots=ptr, actions=ptr, rewards=ptr, nxt=ptr, term=ptr, n_boards=B, side=n):
        return lib.pulse_qtable_update(C.byref(q) if q is not None else None, C.byref(sc) if sc is not None else None, 0, slots, actions, rewards, nxt,
                                       term, n_boards, side, 0.1, 0.99, None)

    def rollout(q, sc=None, boards=ptr, score=ptr, n_boards=B, side=n, env_step=1, actions=ptr, rewards=ptr, dones=ptr, slots=ptr):
        return lib.pulse_qtable_rollout_step(C.byref(q) if q is not None else None, C.byref(sc) if sc is not None else None, 0, boards, score, n_boards,
                                             side, 0.1, 0.1, 0.99, 1, 0, 2, env_step, 0, actions, rewards, dones, slots, None)

    def refused(rc, message):
        assert rc == -1 and message in lib.pulse_last_error(), (rc, lib.pulse_last_error())

    # the table, through every entry point
    for call in (select, update, rollout):
        refused(call(None), b"PulseQTable: null table")
        refused(call(table(entries=None)), b"PulseQTable: null table")
        refused(call(table(entries=ptr + 8)), b"64-byte aligned")
        refused(call(table(entries=ptr + 32)), b"64-byte aligned")
        for side in (2, 5):
            refused(call(table(), side=side), b"board side must be 3 or 4")
        refused(call(table(region_slots=48)), b"must be a power of two")
        refused(call(table(capacity=1000, region_slots=0)), b"must be a power of two")
        refused(call(table(capacity=0, region_slots=0)), b"must be a power of two")
        refused(call(table(capacity=256 * 64 - 64)), b"capacity < n_boards * region_slots")
        refused(call(table(capacity=1 << 20, region_slots=1 << 13)), b"capacity < n_boards * region_slots")
    # a null argument, each in turn
    for call, names in ((select, ("boards", "actions", "slots")), (update, ("slots", "actions", "rewards", "nxt", "term")),
                        (rollout, ("boards", "score", "actions", "rewards", "dones", "slots"))):
        for name in names:
            for side in (3, 4):
                refused(call(table(), side=side, **{name: None}), b"pulse_qtable_" + {select: b"select", update: b"update", rollout: b"rollout_step"}[call]
                        + b": null argument")
    refused(rollout(table(), env_step=0), b"env_step must be >= 1")
    with pytest.raises(ValueError, match="env_step must be >= 1"):
        _native.check(rollout(table(), env_step=0), "pulse_qtable_rollout_step")
    # a shared table's scratch
    shared = table(capacity=1 << 12, region_slots=0)
    for call in (select, update, rollout):
        refused(call(shared, n_boards=-1), b"null argument")
    for call in (update, rollout):
        refused(call(shared), b"a shared table needs its PulseQTableScratch")
        for name in ("count", "cells", "targets", "owner", "acc_key", "acc_cnt", "acc_sum"):
            refused(call(shared, scratch(**{name: True})), b"a shared table needs its PulseQTableScratch")
        refused(call(shared, scratch(n=255)), b"need n >= n_boards")
        refused(call(shared, scratch(n=0)), b"need n >= n_boards")
        refused(call(shared, scratch(n=512, acc_slots=256)), b"acc_slots a power of two >= 2 n_boards")
        refused(call(shared, scratch(n=512, acc_slots=768)), b"acc_slots a power of two >= 2 n_boards")
        refused(call(shared, scratch(n=300, acc_slots=1024)), b"n must be a multiple of 256")
        refused(call(shared, scratch(n=257, acc_slots=1024), n_boards=257), b"n must be a multiple of 256")
        refused(call(shared, scratch(n=1048576 + 256, acc_slots=1 << 22), n_boards=1048577), b"at most 1,048,576 boards")
    assert keep is not None
