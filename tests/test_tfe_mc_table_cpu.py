"""The host half of the 2048 Monte-Carlo table operations (agents/tfe_on_policy_mc_gpu.py, csrc/tfe_mc.hip:
pulse_tfe_mc_table_merge): merge_tables_on_host on host-played games, the entry point's argument checks and struct layout, and the
checkpoint file's writer and reader.  Nothing here launches a kernel.

Shapes: those of tests/test_tfe_mc_sym_gpu.py -- (n, games, max_steps) = (2, 300, 64), (3, 300, 64), (4, 70, 48), seed 10 n + 1,
board_id0 7 -- round 0, played by tests/tfe_host.rollout_on_host and learnt by learn_on_host."""
import ctypes as C
import copy
import re
from pathlib import Path

import numpy as np
import pytest

from tests.native_args import assert_refusals, opts

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(2, 300, 64), (3, 300, 64), (4, 70, 48)]
SPLIT = {300: 153, 70: 38}
BOARD_ID0 = 7


def _learnt(n, games, max_steps, board_id0, canonical=False):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    seed = 10 * n + 1
    o = rollout_on_host(games, n, max_steps, 0.1, {}, seed, seed ^ mc.AGENT_KEY, seed ^ mc.TIE_KEY, board_id0, 0, canonical=canonical)
    return mc.learn_on_host(o["keys"], o["steps"], o["lengths"], 0.9, mc.frac_bits_for(0.9, max_steps), {})


@pytest.fixture(scope="module", params=SHAPES, ids=str)
def tables(request):
    """round 0 of a shape: the whole batch, its two parts (the second on the boards after the first's), and the batch in the canonical frame"""
    n, games, max_steps = request.param
    first = SPLIT[games]
    return dict(n=n, whole=_learnt(n, games, max_steps, BOARD_ID0), y=_learnt(n, first, max_steps, BOARD_ID0),
                z=_learnt(n, games - first, max_steps, BOARD_ID0 + first), canon=_learnt(n, games, max_steps, BOARD_ID0, canonical=True))


def test_merge_of_the_two_parts_is_the_whole(tables):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import merge_tables_on_host
    y, z = copy.deepcopy(tables["y"]), copy.deepcopy(tables["z"])
    got = merge_tables_on_host(y, z)
    assert got is y and got == tables["whole"]
    assert z == tables["z"]                                                 # the source is not changed ...
    got[next(iter(z))][0][0] += 1
    assert z == tables["z"]                                                 # ... and shares no list with the result
    assert set(tables["y"]) & set(tables["z"]) and len(tables["whole"]) < len(tables["y"]) + len(tables["z"])     # entries met


def test_merge_identity_and_commutation(tables):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import merge_tables_on_host
    y, z = tables["y"], tables["z"]
    assert merge_tables_on_host({}, y) == y
    assert merge_tables_on_host(copy.deepcopy(y), {}) == y
    assert merge_tables_on_host(copy.deepcopy(y), z) == merge_tables_on_host(copy.deepcopy(z), y)
    for i in (0, 1):                                                        # nothing is lost
        total = sum(sum(e[i]) for e in y.values()) + sum(sum(e[i]) for e in z.values())
        assert sum(sum(e[i]) for e in tables["whole"].values()) == total


def test_canonical_merge_is_the_fold(tables):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    n, whole = tables["n"], tables["whole"]
    folded = mc.fold_table_on_host(whole, n)
    assert mc.merge_tables_on_host({}, whole, n, canonical=True) == folded == tables["canon"]
    assert mc.merge_tables_on_host({}, folded, n, canonical=True) == folded          # a canonical table folds to itself
    assert len(folded) < len(whole)
    # the two parts folded one after the other into one table: the fold of the whole
    got = mc.merge_tables_on_host(mc.merge_tables_on_host({}, tables["y"], n, canonical=True), tables["z"], n, canonical=True)
    assert got == folded
    # the destination's own keys stay as they are: a plain entry that is not canonical is not moved by a later canonical merge
    key = next(k for k in whole if mc.canon_key_on_host(k, n)[0] != k)
    got = mc.merge_tables_on_host({key: ([1, 2, 3, 4], [5, 6, 7, 8])}, {}, n, canonical=True)
    assert got == {key: ([1, 2, 3, 4], [5, 6, 7, 8])}
    with pytest.raises(ValueError, match="board side"):
        mc.merge_tables_on_host({}, whole, canonical=True)


def test_rehearsed_state_counts(tables):
    """the numbers the device tests' capacities rest on: round 0 stores 183 / 7,959 / 3,314 plain and 41 / 6,344 / 3,238 canonical states"""
    want = {2: (183, 41), 3: (7959, 6344), 4: (3314, 3238)}[tables["n"]]
    assert (len(tables["whole"]), len(tables["canon"])) == want


# ------------------------------------------------------------------ the entry point's argument checks (as tests/test_tfe_mc_sym_cpu.py)
# never dereferenced: every case fails its check first
BASE = dict(src=0x100000, src_entries=16, dst=0x200000, dst_capacity=1 << 10, n=3, canonical=0, stats=0x700000)
CASES = [(dict(src=None), b"src is null"), (dict(dst=None), b"dst is null"), (dict(src=0x100040), b"src must be 128-byte aligned"),
         (dict(dst=0x200008), b"dst must be 128-byte aligned"), (dict(src_entries=0), b"src_entries must be positive"),
         (dict(src=0x10000000000, src_entries=1 << 32), b"src_entries must be below 2^32"),
         (dict(dst_capacity=0), b"dst_capacity must be a power of two"), (dict(dst_capacity=1000), b"dst_capacity must be a power of two"),
         (dict(dst=0x100000), b"src and dst overlap"),                                              # the same range
         (dict(dst=0x100780), b"src and dst overlap"),                                              # dst begins in src's last entry
         (dict(src=0x200000 + 128 * 1023), b"src and dst overlap"),                                 # src begins in dst's last entry
         (dict(src=0x1FF880, src_entries=17), b"src and dst overlap"),                              # src's last entry is dst's first
         (dict(canonical=2), b"canonical must be 0 or 1"), (dict(canonical=-1), b"canonical must be 0 or 1"),
         (dict(n=1), b"board side n must be 2..4"), (dict(n=5), b"board side n must be 2..4"),
         (dict(n=5, canonical=1), b"board side n must be 2..4"), (dict(stats=None), b"stats is null"),
         (dict(stats=0x700004), b"stats must be 8-byte aligned"), (dict(reserved0=1), b"reserved0 must be 0")]


def test_argument_checks_without_gpu():
    from pulselib_amd import _native
    assert_refusals(_native.lib(), "pulse_tfe_mc_table_merge", lambda **kw: opts(_native.TfeMCMerge, **{**BASE, **kw}), CASES)


def test_header_agrees_with_the_binding():
    from pulselib_amd import _native
    text = (ROOT / "include" / "pulse_env.h").read_text()
    assert C.sizeof(_native.TfeMCMerge) == 56
    offsets = {f: getattr(_native.TfeMCMerge, f).offset for f, _ in _native.TfeMCMerge._fields_}
    assert offsets == dict(src=0, src_entries=8, dst=16, dst_capacity=24, n=32, canonical=36, stats=40, reserved0=48)
    body = re.search(r"typedef struct PulseTfeMCMerge \{(.*?)\} PulseTfeMCMerge;", text, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    size = {"const void*": 8, "void*": 8, "uint64_t": 8, "int32_t": 4, "int64_t*": 8, "int64_t": 8}
    at, names = 0, []
    for d in decls:                                                         # the header's own types give the same offsets (natural alignment)
        ctype, fields = re.match(r"((?:const )?\w+\*?)\s+(.*)", d).groups()
        for f in re.findall(r"\w+", fields):
            at = -(-at // size[ctype]) * size[ctype]
            assert offsets[f] == at, f
            at += size[ctype]
            names.append(f)
    assert at == 56 and names == [f for f, _ in _native.TfeMCMerge._fields_]
    assert re.search(r"int pulse_tfe_mc_table_merge\(const PulseTfeMCMerge\* o, void\* stream\);", text)
    assert _native.SYMBOLS["pulse_tfe_mc_table_merge"] == (C.c_int, [C.c_void_p, C.c_void_p])


# ------------------------------------------------------------------ the checkpoint file
SCALARS = dict(n=3, gamma=0.9, epsilon=0.1, frac_bits=22, max_steps=64, seed=2 ** 64 - 3, board_id0=7, round=2, symmetric=1, n_games=300)


def _rows():
    keys = np.array([0x211, 0x12, 0x100000000, 0x3], dtype=np.uint64)      # not sorted
    cnt = np.arange(16, dtype=np.int64).reshape(4, 4)
    total = (np.arange(16, dtype=np.int64).reshape(4, 4) + 1) * (1 << 40)
    return keys, cnt, total


def test_checkpoint_round_trip(tmp_path):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    keys, cnt, total = _rows()
    path = tmp_path / "table.ckpt"                                          # written as named: no suffix is appended
    mc.write_checkpoint(path, keys, cnt, total, **SCALARS)
    assert path.exists() and sorted(p.name for p in tmp_path.iterdir()) == ["table.ckpt"]
    f = mc.read_checkpoint(path, n=3)
    order = np.argsort(keys)
    assert f["keys"].dtype == np.uint64 and f["keys"].tolist() == sorted(keys.tolist())
    assert np.array_equal(f["cnt"], cnt[order]) and np.array_equal(f["sum"], total[order]) and f["cnt"].dtype == f["sum"].dtype == np.int64
    assert {k: f[k] for k in SCALARS} == {**SCALARS, "symmetric": True} and type(f["seed"]) is int and type(f["symmetric"]) is bool
    with np.load(path, allow_pickle=False) as z:                            # plain arrays: every member loads without pickle
        assert sorted(z.files) == sorted(["version", "keys", "cnt", "sum"] + list(SCALARS))
        assert all(z[k].dtype != object for k in z.files) and int(z["version"]) == mc.CHECKPOINT_VERSION == 1
    other = tmp_path / "again.npz"                                          # the same table in another slot order: the same arrays
    perm = np.array([2, 0, 3, 1])
    mc.write_checkpoint(other, keys[perm], cnt[perm], total[perm], **SCALARS)
    g = mc.read_checkpoint(other)
    assert all(np.array_equal(f[k], g[k]) for k in ("keys", "cnt", "sum"))
    empty = tmp_path / "empty.npz"
    mc.write_checkpoint(empty, np.zeros(0, np.uint64), np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), **SCALARS)
    assert len(mc.read_checkpoint(empty)["keys"]) == 0 and mc.read_checkpoint(empty)["cnt"].shape == (0, 4)


def test_checkpoint_refusals(tmp_path):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    keys, cnt, total = _rows()
    path = tmp_path / "table.npz"
    mc.write_checkpoint(path, keys, cnt, total, **SCALARS)
    with pytest.raises(ValueError, match="board side 3, expected 4"):
        mc.read_checkpoint(path, n=4)
    with np.load(path, allow_pickle=False) as z:
        good = {k: z[k] for k in z.files}

    def rewritten(**change):
        bad = tmp_path / "bad.npz"
        with open(bad, "wb") as fh:
            np.savez(fh, **{**good, **change})
        return bad
    with pytest.raises(ValueError, match="format version 2"):
        mc.read_checkpoint(rewritten(version=np.array(2, dtype=np.int64)))
    with pytest.raises(ValueError, match="fit the 2 x 2 cells"):           # keys of a 3 x 3 board under n = 2
        mc.read_checkpoint(rewritten(n=np.array(2, dtype=np.int64)))
    with pytest.raises(ValueError, match="board side 5"):
        mc.read_checkpoint(rewritten(n=np.array(5, dtype=np.int64)))
    with pytest.raises(ValueError, match="strictly ascending"):
        mc.read_checkpoint(rewritten(keys=good["keys"][::-1].copy()))
    with pytest.raises(ValueError, match="strictly ascending"):            # key 0 is the free slot
        mc.read_checkpoint(rewritten(keys=np.array([0, 3, 4, 5], dtype=np.uint64)))
    with pytest.raises(ValueError, match="int64\\[m, 4\\]"):
        mc.read_checkpoint(rewritten(cnt=good["cnt"][:3]))
    with pytest.raises(ValueError, match="int64\\[m, 4\\]"):
        mc.read_checkpoint(rewritten(sum=good["sum"].astype(np.float64)))
    missing = tmp_path / "missing.npz"
    with open(missing, "wb") as fh:
        np.savez(fh, **{k: v for k, v in good.items() if k != "round"})
    with pytest.raises(ValueError, match="round"):
        mc.read_checkpoint(missing)
    pickled = tmp_path / "pickled.npz"                                      # an object array needs a pickle: the reader does not allow one
    with open(pickled, "wb") as fh:
        np.savez(fh, **{**good, "keys": np.array([{"a": 1}], dtype=object)})
    with pytest.raises(ValueError):
        mc.read_checkpoint(pickled)
    with pytest.raises(ValueError, match="one row per entry"):
        mc.write_checkpoint(tmp_path / "x.npz", keys, cnt[:3], total, **SCALARS)
    with pytest.raises(ValueError, match="exactly the scalars"):
        mc.write_checkpoint(tmp_path / "x.npz", keys, cnt, total, **{k: v for k, v in SCALARS.items() if k != "seed"})
