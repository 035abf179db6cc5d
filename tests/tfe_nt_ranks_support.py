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
