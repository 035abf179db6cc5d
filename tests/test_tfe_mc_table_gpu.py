"""The 2048 Monte-Carlo table operations on the device (csrc/tfe_mc.hip: pulse_tfe_mc_table_merge) against the
host's statement (merge_tables_on_host, fold_table_on_host) in exact integers: adding two agents' tables, growing, the all-or-nothing
drop, the fold, dense sources, save / load / continue, the refusals and the script's options.

Shapes: those of tests/test_tfe_mc_sym_gpu.py -- 300 games (two workgroups of the game kernels, the second partial) at n = 2 and n = 3 with
max_steps = 64, 70 games at n = 4 with max_steps = 48, seed 10 n + 1, board_id0 7.  Rehearsed on the host (tests/test_tfe_mc_table_cpu.py
asserts round 0): 183 / 7,959 / 3,314 plain and 41 / 6,344 / 3,238 canonical states after one round, 243 / 20,926 / 9,846 plain after
three, so capacity 2^16 holds n = 3 and n = 4 without a drop and 2^12 holds n = 2.  Every table, dense array and per-game buffer a
launch is handed sits between guard words: the class's allocator of tables is replaced by one that guards (the fixture below)."""
import copy
import re

import numpy as np
import pytest

from tests.tfe_gpu_support import guard, guarded, guards_intact

pytestmark = pytest.mark.gpu

#         n, games, max_steps
SHAPES = [(2, 300, 64), (3, 300, 64), (4, 70, 48)]
CAPACITY = {2: 1 << 12, 3: 1 << 16, 4: 1 << 16}
SPLIT = {300: 153, 70: 38}
BUFFERS = ("keys", "steps", "lengths", "total_score", "episode_reward", "counters", "_eval", "_merge")


@pytest.fixture(autouse=True)
def guarded_tables(monkeypatch):
    """every table and dense array of every agent made here -- by the tests, by grow / to_symmetric / load and by the script -- is
    allocated between guard words and listed in the agent's `_guards`"""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU

    def new_table(self, rows):
        inner, flat, g = guarded(torch.zeros((rows, 16), dtype=torch.int64, device=self.device))
        assert inner.data_ptr() % 128 == 0
        self.__dict__.setdefault("_guards", []).append((f"table of {rows}", flat, g))
        return inner
    monkeypatch.setattr(OnPolicyFirstVisitMCTFEGPU, "_new_table", new_table)


def _guard(a):
    """the per-game buffers and counters of an agent re-seated between guard words (contents kept)"""
    return guard(a, BUFFERS, fill=None)


def _agent(shape, symmetric=False, capacity=None, n_games=None, board_id0=7, **kw):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    n, games, max_steps = shape
    kw.setdefault("max_steps", max_steps)
    return _guard(OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), games if n_games is None else n_games, board_size=n,
                                             capacity=CAPACITY[n] if capacity is None else capacity, seed=10 * n + 1, board_id0=board_id0,
                                             symmetric=symmetric, **kw))


def _raw(a):
    return a.entries.cpu().numpy().copy()


def _same_last_round(a, b):
    """the two agents' last roll-outs: keys and steps over the moves played, lengths and scores"""
    la, lb = a.lengths.cpu().numpy(), b.lengths.cpu().numpy()
    assert np.array_equal(la, lb) and la.max() > 0
    on = np.arange(a.max_steps)[:, None] < la[None, :]
    assert np.array_equal(a.keys.cpu().numpy()[on], b.keys.cpu().numpy()[on])
    assert np.array_equal(a.steps.cpu().numpy()[on], b.steps.cpu().numpy()[on])
    assert np.array_equal(a.total_score.cpu().numpy(), b.total_score.cpu().numpy())


def _dense(a, table, keys=None):
    keys = sorted(table) if keys is None else keys
    return a.dense_entries(np.array(keys, dtype=np.uint64), np.array([table[k][0] for k in keys], dtype=np.int64).reshape(-1, 4),
                           np.array([table[k][1] for k in keys], dtype=np.int64).reshape(-1, 4))


# ------------------------------------------------------------------ 1. the tables of two agents add up
@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_merge_of_two_agents_is_the_whole_batch(shape, symmetric):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import merge_tables_on_host
    first = SPLIT[shape[1]]
    x = _agent(shape, symmetric).learn_batch()
    y = _agent(shape, symmetric, n_games=first).learn_batch()
    z = _agent(shape, symmetric, n_games=shape[1] - first, board_id0=7 + first).learn_batch()
    ty, tz, z_raw = y.table(), z.table(), _raw(z)
    assert x.stats()["dropped"] == y.stats()["dropped"] == z.stats()["dropped"] == 0
    assert y.merge_from(z) is y
    got, st = y.table(), y.merge_stats()
    print(shape, symmetric, "states", len(ty), "+", len(tz), "->", len(got), st)
    assert got == x.table()
    assert got == merge_tables_on_host(copy.deepcopy(ty), tz)
    assert st == dict(live=len(tz), placed=len(tz), dropped=0)
    assert len(got) < len(ty) + len(tz)                                     # entries met
    assert np.array_equal(_raw(z), z_raw)                                   # the source: only read
    assert y.merge_stats(clear=True) == st and y.merge_stats() == dict(live=0, placed=0, dropped=0)
    guards_intact(x, y, z)


# ------------------------------------------------------------------ 2. growing keeps the map and the games to come
@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_grow_keeps_the_map_and_the_future(shape, symmetric):
    n = shape[0]
    small, large = (1 << 12, 1 << 14) if n == 2 else (1 << 16, 1 << 17)
    a, b = _agent(shape, symmetric, small), _agent(shape, symmetric, large)
    for agent in (a, b):
        agent.learn_batch().learn_batch()
    before, stats, old = a.table(), a.stats(), a.entries
    assert a.grow(large) is a
    assert a.capacity == large and tuple(a.entries.shape) == (large, 16) and a.entries.data_ptr() != old.data_ptr()
    assert a.table() == before == b.table() and a.occupancy() == len(before)
    assert a.round == 2 and a.stats() == stats and a.merge_stats() == dict(live=0, placed=0, dropped=0)
    a.learn_batch()
    b.learn_batch()
    _same_last_round(a, b)
    assert a.table() == b.table() and len(a.table()) > len(before)
    assert a.stats() == b.stats() and a.stats()["dropped"] == 0
    a.grow(large // 2)                                                      # shrinking: the same rule
    assert a.capacity == large // 2 and a.table() == b.table()
    with pytest.raises(ValueError, match="power of two"):
        a.grow(3000)
    guards_intact(a, b)


# ------------------------------------------------------------------ 3. no room: counted, never half-learnt
def test_no_room_is_counted_and_nothing_is_half_added():
    shape = SHAPES[1]
    src = _agent(shape).learn_batch()
    table = src.table()
    assert len(table) == 7959 and src.stats()["dropped"] == 0               # (rehearsed)
    dst = _agent(shape, capacity=1 << 12)
    st = dst.merge_from(src).merge_stats()
    got = dst.table()
    print("into 2^12 slots:", st, "stored", len(got))
    assert st["live"] == 7959 and st["placed"] + st["dropped"] == st["live"]
    assert st["dropped"] >= st["live"] - 4096 and st["placed"] == dst.occupancy() == len(got)
    assert got == {k: table[k] for k in got}                                # every stored key holds exactly its source's eight integers
    entries, raw = src.entries, _raw(src)
    with pytest.raises(RuntimeError, match="found no room"):
        src.grow(1 << 12)
    assert src.entries is entries and src.capacity == 1 << 16 and np.array_equal(_raw(src), raw) and src.table() == table
    with pytest.raises(RuntimeError, match="found no room"):
        src.to_symmetric(capacity=1 << 12)
    guards_intact(src, dst)


# ------------------------------------------------------------------ 4. the fold on the device
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fold_on_the_device(shape):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    n = shape[0]
    plain, sym = _agent(shape).learn_batch(), _agent(shape, True).learn_batch()
    plain_raw = _raw(plain)
    folded = _guard(plain.to_symmetric())
    want = mc.fold_table_on_host(plain.table(), n)
    assert folded.table() == want == sym.table()                            # round 0 plays the same games in both frames
    assert folded.symmetric and folded.round == 1 and folded.capacity == plain.capacity and folded.n_games == plain.n_games
    assert (folded.seed, folded.board_id0, folded.env_seed, folded.agent_seed, folded.tie_seed, folded.frac_bits, folded.max_steps) == \
        (plain.seed, plain.board_id0, plain.env_seed, plain.agent_seed, plain.tie_seed, plain.frac_bits, plain.max_steps)
    assert folded.merge_stats() == dict(live=len(plain.table()), placed=len(plain.table()), dropped=0)
    assert np.array_equal(_raw(plain), plain_raw)
    sym.learn_batch()                                                       # the folded agent goes on as the symmetric one does
    folded.learn_batch()
    _same_last_round(folded, sym)
    assert folded.table() == sym.table()
    plain.learn_batch().learn_batch()                                       # three rounds: the policies have diverged, the fold is still the fold
    t3 = plain.table()
    assert plain.stats()["dropped"] == 0
    assert plain.to_symmetric(capacity=2 * plain.capacity).table() == mc.fold_table_on_host(t3, n)
    before = sym.table()                                                    # a plain table into a NON-EMPTY symmetric one
    sym.merge_stats(clear=True)
    got = sym.merge_from(plain).table()
    assert got == mc.merge_tables_on_host(copy.deepcopy(before), t3, n, canonical=True)
    assert sym.merge_stats() == dict(live=len(t3), placed=len(t3), dropped=0)
    with pytest.raises(ValueError, match="already"):
        sym.to_symmetric()
    guards_intact(plain, sym, folded)


# ------------------------------------------------------------------ 5. dense sources
def test_dense_sources():
    import torch
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    shape = SHAPES[1]
    src = _agent(shape).learn_batch()
    table = src.table()
    keys = sorted(table)
    assert len(keys) == 7959 and len(keys) % 256                            # 31 workgroups of the merge kernel and 23 lanes of a 32nd
    dense = _dense(src, table)
    assert tuple(dense.shape) == (7959, 16) and dense.data_ptr() % 128 == 0
    dst = _agent(shape)
    assert dst.merge_from(dense).table() == table
    assert dst.merge_stats(clear=True) == dict(live=7959, placed=7959, dropped=0)
    raw = _raw(dst)
    hollow = src._new_table(300)                                            # every key 0: nothing is live, whatever the other words hold
    hollow[:, 1:] = 5
    dst.merge_from(hollow)
    assert dst.merge_stats(clear=True) == dict(live=0, placed=0, dropped=0) and np.array_equal(_raw(dst), raw)
    dst.merge_from(dense)                                                   # a second time: every value doubles
    assert dst.table() == {k: ([2 * v for v in c], [2 * v for v in s]) for k, (c, s) in table.items()}
    one = _agent(shape)                                                     # a single row
    one.merge_from(_dense(src, table, keys[4000:4001]))
    assert one.table() == {keys[4000]: table[keys[4000]]} and one.merge_stats() == dict(live=1, placed=1, dropped=0)
    twice = _agent(shape)                                                   # the same keys twice in ONE launch: the adds meet
    twice.merge_from(_dense(src, table, keys[:700] + keys[:700]))
    assert twice.table() == {k: ([2 * v for v in table[k][0]], [2 * v for v in table[k][1]]) for k in keys[:700]}
    assert twice.merge_stats() == dict(live=1400, placed=1400, dropped=0)
    sym = _agent(shape, True)                                               # a dense plain source folded on the way
    sym.merge_from(dense, canonical=True)
    assert sym.table() == mc.fold_table_on_host(table, 3)
    with pytest.raises(ValueError, match="symmetric destination"):
        dst.merge_from(dense, canonical=True)
    for bad in (dense[:, :8], dense.to(torch.int32), dense[:0], dense.cpu()):
        with pytest.raises(ValueError):
            dst.merge_from(bad)
    guards_intact(src, dst, one, twice, sym)


# ------------------------------------------------------------------ 6. save, load, continue
@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_save_load_continue(shape, symmetric, tmp_path):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import read_checkpoint
    a = _agent(shape, symmetric).learn_batch().learn_batch()
    table = a.table()
    path, again = tmp_path / "run.npz", tmp_path / "again.npz"
    a.save(path)
    f = read_checkpoint(path, n=shape[0])
    assert f["keys"].tolist() == sorted(table) and len(table) > 40
    b = _guard(OnPolicyFirstVisitMCTFEGPU.load(path, torch.device("cuda:0"), capacity=2 * a.capacity))
    assert b.capacity == 2 * a.capacity and b.table() == table and b.merge_stats() == dict(live=len(table), placed=len(table), dropped=0)
    for name in ("round", "seed", "board_id0", "env_seed", "agent_seed", "tie_seed", "frac_bits", "n", "n_games", "max_steps", "gamma", "epsilon", "symmetric"):
        assert getattr(b, name) == getattr(a, name), name
    assert b.round == 2
    b.save(again)                                                           # other slots, the same arrays; and the same file from the same agent
    a.save(tmp_path / "third.npz")
    g, h = read_checkpoint(again), read_checkpoint(tmp_path / "third.npz")
    for name in ("keys", "cnt", "sum"):
        assert f[name].tobytes() == g[name].tobytes() == h[name].tobytes(), name
    assert {k: v for k, v in f.items() if k not in ("keys", "cnt", "sum")} == {k: v for k, v in g.items() if k not in ("keys", "cnt", "sum")}
    c = OnPolicyFirstVisitMCTFEGPU.load(path, torch.device("cuda:0"))       # the default capacity: the smallest power of two >= 4 m and >= 2^12
    assert c.capacity == max(1 << 12, 1 << (4 * len(table) - 1).bit_length()) and c.table() == table
    a.learn_batch()
    b.learn_batch()
    _same_last_round(a, b)
    assert a.table() == b.table() and a.round == b.round == 3 and b.stats()["dropped"] == 0
    guards_intact(a, b, c)


# ------------------------------------------------------------------ 7. what the Python layer refuses
def test_refusals_in_python():
    shape = SHAPES[0]
    a = _agent(shape)
    for other, what in ((_agent(SHAPES[1], capacity=1 << 12), "n differs"), (_agent(shape, gamma=0.8), "gamma differs"),
                        (_agent(shape, max_steps=4), "frac_bits differs"), (_agent(shape, True), "canonical states"), (a, "into itself")):
        with pytest.raises(ValueError, match=what):
            a.merge_from(other)
    with pytest.raises(ValueError, match="follows from"):
        _agent(shape, True).merge_from(a, canonical=True)
    assert a.merge_stats() == dict(live=0, placed=0, dropped=0) and a.occupancy() == 0


# ------------------------------------------------------------------ 8. the script
def test_script_grows_saves_and_resumes(tmp_path):
    import torch
    from pulselib_amd.scripts.tfe_opfvmc import run
    dev = torch.device("cuda:0")
    kw = dict(tables=300, board=3, max_steps=64, seed=31)
    lines = []
    agent = run(dev, 3, capacity=1 << 12, grow_at=0.5, out=lines.append, **kw)
    for line in lines:
        print(line)
    assert len(lines) == 3
    dropped = [int(re.search(r"dropped (\d+)", line).group(1)) for line in lines]
    seen = [tuple(map(int, re.search(r"occupancy (\d+) of (\d+)", line).groups())) for line in lines]
    assert dropped[0] > 0 and "grown to" in lines[0] and seen[0][1] == 1 << 12        # 7,900 states of round 0 do not fit 2^12 slots
    assert dropped[1] == dropped[2] == dropped[0]                           # ... and after the first growth nothing is dropped
    slots = 1 << 12
    for line, (occupancy, of) in zip(lines, seen):                          # the line shows the table the round ran on, then what it grew to
        assert of == slots and occupancy <= of
        grown = re.search(r"grown to (\d+)", line)
        slots = int(grown.group(1)) if grown else slots
        assert occupancy < 0.5 * slots
    assert agent.capacity == slots >= 1 << 15 and agent.occupancy() == len(agent.table()) == seen[-1][0]
    guards_intact(agent)
    plain_lines = []
    whole = run(dev, 3, capacity=1 << 16, out=plain_lines.append, **kw)   # without --grow-at the line is the one it was
    assert len(plain_lines) == 3 and not any("occupancy" in line or "grown" in line for line in plain_lines)
    assert whole.stats()["dropped"] == 0
    path = tmp_path / "run.npz"
    head = run(dev, 2, capacity=1 << 16, out=lines.append, save=path, **kw)
    tail = run(dev, 1, capacity=1 << 16, out=lines.append, resume=path, **kw)
    assert head.round == 2 and tail.round == 3 and lines[-1].startswith("Round 2: episodes 900,")
    assert tail.table() == whole.table() and tail.stats()["dropped"] == 0
    auto = run(dev, 1, out=lines.append, resume=path, **kw)                # no capacity given: load()'s own, from the saved rows
    saved = len(head.table())
    assert auto.capacity == max(1 << 12, 1 << (4 * saved - 1).bit_length()) and auto.table() == whole.table()
    with pytest.raises(ValueError, match="continues another run"):
        run(dev, 1, capacity=1 << 16, out=lines.append, resume=path, **{**kw, "tables": 200})
    guards_intact(whole, head, tail, auto)
