"""The host half of the 2048 Monte-Carlo symmetries and evaluation launch (agents/tfe_on_policy_mc_gpu.py,
csrc/tfe_mc.hip): the eight transforms and the action map against the oracle's move, canonical keys, the folded table, the run-mask
first-visit rule on canonical (state, action) pairs against the dict rule, and the two new entry points' argument checks and struct
layouts.  Nothing here launches a kernel."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests.native_args import assert_refusals, opts

ROOT = Path(__file__).resolve().parent.parent
SIDES = (2, 3, 4)


def _boards(n, count, seed):
    """random boards of every fill: empty cells with probability 0 .. 0.6 (at least one tile), tiles 2 .. 2^k with few distinct values,
    so that rows merge; some boards are full"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        logs = rng.integers(1, 2 + i % 5, size=(n, n))
        logs[rng.random((n, n)) < (i % 4) * 0.2] = 0
        if not logs.any():
            logs[0, 0] = 1
        out.append(np.where(logs > 0, 1 << logs, 0).astype(np.int32))
    return out


def _image(board, src):
    return board.ravel()[src].reshape(board.shape)


@pytest.mark.parametrize("n", SIDES)
def test_transforms_are_the_eight_symmetries(n):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import transforms_on_host
    T = transforms_on_host(n)
    assert T.shape == (8, n * n)
    for src in T:
        assert sorted(src.tolist()) == list(range(n * n))                  # a bijection of the cells
    assert len({tuple(src.tolist()) for src in T}) == 8 and T[0].tolist() == list(range(n * n))
    board = np.arange(n * n).reshape(n, n)
    for k in range(4):                                                      # T_k: k of the reference's rotations (TFE.py:38-44: out[n-1-j][i] = in[i][j])
        assert np.array_equal(_image(board, T[k]), np.rot90(board, k))
        assert np.array_equal(_image(board, T[4 + k]), np.rot90(board.T, k))
    images = {tuple(src.tolist()) for src in T}
    for a in T:                                                             # closed under composition: a group of order 8
        for b in T:
            assert tuple(a[b].tolist()) in images


@pytest.mark.parametrize("n", SIDES)
def test_action_map_commutes_with_the_oracles_move(n):
    """T_j(move(B, a)) == move(T_j(B), ACTION_MAP[j][a]) with the same merge score, for 200 boards, every j and every a; the move is
    the oracle's step with its spawn taken out (tests/tfe_host.move_on_host)."""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import ACTION_MAP, ACTION_UNMAP, transforms_on_host
    from tests.tfe_host import move_on_host
    T = transforms_on_host(n)
    assert all(sorted(row) == [0, 1, 2, 3] for row in ACTION_MAP) and len(ACTION_MAP) == 8
    assert all(ACTION_UNMAP[j][ACTION_MAP[j][a]] == a for j in range(8) for a in range(4))
    changed = merged = lone = 0
    for board in _boards(n, 200, 7 + n):
        for a in range(4):
            moved, score, spawned = move_on_host(board, a)
            changed += not np.array_equal(moved, board)
            merged += score > 0
            lone += spawned
            for j in range(8):
                got, got_score, got_spawned = move_on_host(_image(board, T[j]), ACTION_MAP[j][a])
                assert np.array_equal(got, _image(moved, T[j])) and got_score == score and got_spawned == spawned, (board, j, a)
    assert changed > 300 and merged > 100 and (lone > 0 or n == 4)
    # no other table passes: with a wrong action for a board that the move changes asymmetrically the images differ
    board = np.array([[2, 2], [4, 0]], dtype=np.int32) if n == 2 else _boards(n, 8, 1)[5]
    for j in range(8):
        for a in range(4):
            right = _image(move_on_host(board, a)[0], T[j])
            assert [b for b in range(4) if np.array_equal(move_on_host(_image(board, T[j]), b)[0], right)].count(ACTION_MAP[j][a]) == 1


def test_device_constants_are_the_action_map():
    """csrc/tfe_mc.hip holds the two tables as two bits per (j, a) in one 64-bit constant each"""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import ACTION_MAP, ACTION_UNMAP
    text = (ROOT / "pulselib_amd" / "csrc" / "tfe_mc.hip").read_text()
    m = re.search(r"kActionMap = (0x[0-9a-f]+)ull, kActionUnmap = (0x[0-9a-f]+)ull;", text)
    for word, table in zip(m.groups(), (ACTION_MAP, ACTION_UNMAP)):
        assert [[(int(word, 16) >> (8 * j + 2 * a)) & 3 for a in range(4)] for j in range(8)] == [list(r) for r in table]


@pytest.mark.parametrize("n", SIDES)
def test_canon_is_constant_over_the_images_and_greedy_is_equivalent(n):
    """canon_on_host of a board's eight images is one key, the smallest of the eight, with the smallest j that reaches it; and the
    greedy action of that key's entry, mapped back to each image's frame, leads the images to images of one board with one score."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import canon_many, move_on_host
    T = mc.transforms_on_host(n)
    rng = np.random.default_rng(n)
    symmetric = 0
    for board in _boards(n, 200, 70 + n):
        images = [_image(board, src) for src in T]
        keys = [mc.pack_board(b) for b in images]
        key_c, j = mc.canon_on_host(board)
        assert key_c == min(keys) and j == keys.index(key_c) and keys[0] == mc.pack_board(board)
        assert mc.canon_key_on_host(keys[0], n) == (key_c, j)
        symmetric += len(set(keys)) < 8
        many = canon_many(np.stack(images))
        assert many[0].tolist() == [key_c] * 8                              # constant over the images
        assert many[1].tolist() == [mc.canon_on_host(b)[1] for b in images]
        for b, jb in zip(images, many[1].tolist()):                         # T_j* of a board IS the canonical board
            assert mc.pack_board(_image(b, T[jb])) == key_c
        entry = (rng.integers(0, 3, 4).tolist(), rng.integers(0, 40, 4).tolist())        # few distinct q: ties are common
        a_c = mc.greedy_on_host(entry, key_c, 99, 5)
        ends = set()
        for b, jb in zip(images, many[1].tolist()):
            moved, score, spawned = move_on_host(b, mc.ACTION_UNMAP[jb][a_c])
            ends.add((mc.canon_on_host(moved)[0], score, spawned))
        assert len(ends) == 1
    assert symmetric > 0                                                    # some boards are their own image: j* is the smallest then


class _Agent:
    """OnPolicyFirstVisitMCTFEGPU.greedy without a device: the method reads table(), n, symmetric, tie_seed, round"""
    def __init__(self, table, n, symmetric):
        self._table, self.n, self.symmetric, self.tie_seed, self.round = table, n, symmetric, 5, 2

    def table(self):
        return self._table


@pytest.mark.parametrize("n", (2, 3))
def test_greedy_takes_raw_keys(n):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    T = mc.transforms_on_host(n)
    board = _boards(n, 8, 3)[6]
    key_c, _ = mc.canon_on_host(board)
    table = {key_c: ([1, 1, 1, 1], [5, 9, 2, 7])}                          # q: action 1 of the canonical frame
    for src in T:
        image = _image(board, src)
        key, (_, j) = mc.pack_board(image), mc.canon_on_host(image)
        (a,) = mc.OnPolicyFirstVisitMCTFEGPU.greedy(_Agent(table, n, True), [key])
        assert mc.ACTION_MAP[j][a] == 1
        want = [1] if key == key_c else [None]
        assert mc.OnPolicyFirstVisitMCTFEGPU.greedy(_Agent(table, n, False), [key]) == want
    assert mc.OnPolicyFirstVisitMCTFEGPU.greedy(_Agent({}, n, True), [mc.pack_board(board)]) == [None]


@pytest.mark.parametrize("n,n_games", [(2, 600), (3, 200)])
def test_run_mask_on_canonical_pairs_is_the_dict_rule(n, n_games):
    """Equal canonical keys: equal tile sums: one run of one unchanged board: one j* (DESIGN.md section 12.1).  Host-played games in
    the canonical frame, round 0 on an empty table and round 1 on the table learnt from it; at n = 2 repeats are common."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    seed, table, repeats = 31 + n, {}, 0
    for r in range(2):
        o = rollout_on_host(n_games, n, 256, 0.1, table, seed, seed ^ mc.AGENT_KEY, seed ^ mc.TIE_KEY, 50 + r * n_games, r, canonical=True)
        assert o["truncated"] == 0 and (r == 0) == (o["present"] == 0)
        a, _, f = mc.unpack_steps(o["steps"])
        for g, L in enumerate(o["lengths"].tolist()):
            keys, actions = o["keys"][:L, g], a[:L, g]
            want = mc.first_visit_flags_on_host(keys, actions)
            assert np.array_equal(mc.run_mask_flags_on_host(keys, actions), want)
            assert np.array_equal(f[:L, g], want)                           # the roll-out's own bit 7
            assert all(mc.canon_key_on_host(k, n) == (k, 0) for k in keys[:3].tolist())
            repeats += int((~want).sum())
        mc.learn_on_host(o["keys"], o["steps"], o["lengths"], 0.9, mc.frac_bits_for(0.9, 256), table)
    assert repeats >= 100, repeats


@pytest.mark.parametrize("n", (2, 3))
def test_canonical_rollout_on_an_empty_table_plays_the_plain_games(n):
    """no entry: the board moves by y >> 30 in either frame; the recorded pairs are the plain ones, canonicalised"""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    args = (40, n, 128, 0.1, {}, 8, 8 ^ mc.AGENT_KEY, 8 ^ mc.TIE_KEY, 3, 0)
    plain, canon = rollout_on_host(*args), rollout_on_host(*args, canonical=True)
    for name in ("lengths", "total_score", "episode_reward", "moved", "final_boards"):
        assert np.array_equal(canon[name], plain[name]), name
    a_c, r_c, _ = mc.unpack_steps(canon["steps"])
    a, r, _ = mc.unpack_steps(plain["steps"])
    for g, L in enumerate(plain["lengths"].tolist()):
        for t in range(L):
            key_c, j = mc.canon_key_on_host(int(plain["keys"][t, g]), n)
            assert (int(canon["keys"][t, g]), int(a_c[t, g]), int(r_c[t, g])) == (key_c, mc.ACTION_MAP[j][a[t, g]], int(r[t, g]))


@pytest.mark.parametrize("n", (2, 3))
def test_fold_table(n):
    """folding is idempotent, every key of a folded table is its own canonical key, nothing is lost, and the fold of the table learnt
    from plain games on an empty table is the table learnt from the same games recorded in the canonical frame"""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    args = (120, n, 128, 0.1, {}, 9, 9 ^ mc.AGENT_KEY, 9 ^ mc.TIE_KEY, 0, 0)
    fb = mc.frac_bits_for(0.9, 128)
    plain, canon = rollout_on_host(*args), rollout_on_host(*args, canonical=True)
    table = mc.learn_on_host(plain["keys"], plain["steps"], plain["lengths"], 0.9, fb, {})
    folded = mc.fold_table_on_host(table, n)
    assert folded == mc.learn_on_host(canon["keys"], canon["steps"], canon["lengths"], 0.9, fb, {})
    assert mc.fold_table_on_host(folded, n) == folded and len(folded) < len(table)
    assert all(mc.canon_key_on_host(k, n) == (k, 0) for k in folded)
    for i in (0, 1):
        assert sum(sum(e[i]) for e in folded.values()) == sum(sum(e[i]) for e in table.values())
    assert table == mc.learn_on_host(plain["keys"], plain["steps"], plain["lengths"], 0.9, fb, {})         # the argument was not changed


def test_eval_summary_on_host():
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import EVAL_BINS, EVAL_SUMMARY, eval_summary_on_host
    scores = [4, 8, 8, 100]
    words = [4, 30, sum(scores), sum(s * s for s in scores), 100, 1, 12, 9] + [0] * 3 + [1, 3] + [0] * 11
    out = eval_summary_on_host(words)
    assert len(EVAL_SUMMARY) == 8 and EVAL_BINS == 16 and [out[k] for k in EVAL_SUMMARY] == words[:8] and out["max_tile_hist"] == words[8:]
    assert out["mean_score"] == 30.0 and math.isclose(out["std_score"], float(np.std(scores, ddof=1)), rel_tol=1e-12)
    assert out["mean_length"] == 7.5 and out["coverage"] == 0.4 and out["max_score"] == 100 and out["truncated"] == 1
    assert eval_summary_on_host([0] * 24)["std_score"] == 0.0


# ------------------------------------------------------------------ the entry points' argument checks (as tests/test_tfe_mc_cpu.py)
# never dereferenced: every case fails its check first
BASE = dict(entries=0x100000, capacity=1 << 10, n_games=64, n=3, max_steps=128, frac_bits=22, gamma=0.9, epsilon=0.1,
            keys=0x200000, steps=0x300000, lengths=0x400000, total_score=0x500000, episode_reward=0x600000, stats=0x700000,
            summary=0x800000, max_tile_hist=0x900000, canonical=1)
TABLE = [(dict(entries=None), b"entries is null"), (dict(entries=0x100040), b"128-byte aligned"), (dict(capacity=0), b"power of two"),
         (dict(capacity=1000), b"power of two"), (dict(n=1), b"board side must be 2..4"), (dict(n=5), b"board side must be 2..4"),
         (dict(n_games=0), b"n_games must be positive"), (dict(max_steps=0), b"max_steps must be in 1..65535"),
         (dict(max_steps=65536), b"max_steps must be in 1..65535"), (dict(epsilon=-0.01), b"epsilon must be in [0, 1]"),
         (dict(epsilon=math.nan), b"epsilon must be in [0, 1]")]
ROLLOUT = [(dict(gamma=1.01), b"gamma must be in [0, 1]"), (dict(frac_bits=23), b"frac_bits"), (dict(frac_bits=-1), b"frac_bits"),
           (dict(keys=None), b"keys is null"), (dict(steps=None), b"steps is null"), (dict(lengths=None), b"lengths is null"),
           (dict(stats=None), b"stats is null"), (dict(keys=0x200004), b"8-byte aligned"), (dict(lengths=0x400002), b"4-byte aligned"),
           (dict(reserved0=1), b"reserved0 must be 0"), (dict(total_score=None), b"total_score is null"),
           (dict(episode_reward=None), b"episode_reward is null"), (dict(total_score=0x500004), b"total_score must be 8-byte aligned"),
           (dict(episode_reward=0x600002), b"episode_reward must be 4-byte aligned")]
EVAL = [(dict(frac_bits=31), b"frac_bits must be in 0..30"), (dict(frac_bits=-1), b"frac_bits must be in 0..30"),
        (dict(canonical=2), b"canonical must be 0 or 1"), (dict(canonical=-1), b"canonical must be 0 or 1"),
        (dict(summary=None), b"summary is null"), (dict(max_tile_hist=None), b"max_tile_hist is null"),
        (dict(summary=0x800004), b"8-byte aligned"), (dict(max_tile_hist=0x900004), b"8-byte aligned"),
        (dict(total_score=0x500004), b"total_score must be 8-byte aligned"), (dict(lengths=0x400002), b"lengths must be 4-byte aligned"),
        (dict(reserved0=1), b"reserved0 / reserved1 must be 0"), (dict(reserved1=1), b"reserved0 / reserved1 must be 0")]


def test_argument_checks_without_gpu():
    from pulselib_amd import _native
    lib = _native.lib()
    for name, struct, cases in (("pulse_tfe_mc_rollout_canon", _native.TfeMCRollout, TABLE + ROLLOUT), ("pulse_tfe_mc_evaluate", _native.TfeMCEval, TABLE + EVAL)):
        assert_refusals(lib, name, lambda **kw: opts(struct, **{**BASE, **kw}), cases)


def test_header_agrees_with_the_binding():
    from pulselib_amd import _native
    text = (ROOT / "include" / "pulse_env.h").read_text()
    assert C.sizeof(_native.TfeMCRollout) == 144 and C.sizeof(_native.TfeMCEval) == 128
    offsets = {f: getattr(_native.TfeMCEval, f).offset for f, _ in _native.TfeMCEval._fields_}
    assert offsets == dict(entries=0, capacity=8, n_games=16, n=20, max_steps=24, frac_bits=28, epsilon=32, env_seed=40, agent_seed=48,
                           tie_seed=56, board_id0=64, round=72, canonical=80, reserved0=84, summary=88, max_tile_hist=96, total_score=104,
                           lengths=112, reserved1=120)
    body = re.search(r"typedef struct PulseTfeMCEval \{(.*?)\} PulseTfeMCEval;", text, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    names = [n for d in decls for n in re.findall(r"(\w+)\s*(?:,|$)", d)]
    assert names == [f for f, _ in _native.TfeMCEval._fields_]
    size = {"const void*": 8, "uint64_t": 8, "int32_t": 4, "double": 8, "int64_t*": 8, "int32_t*": 8, "int64_t": 8}
    at = 0
    for d in decls:                                                         # the header's own types give the same offsets (natural alignment)
        ctype, fields = re.match(r"((?:const )?\w+\*?)\s+(.*)", d).groups()
        for f in re.findall(r"\w+", fields):
            at = -(-at // size[ctype]) * size[ctype]
            assert offsets[f] == at, f
            at += size[ctype]
    assert at == 128
    assert re.search(r"int pulse_tfe_mc_rollout_canon\(const PulseTfeMCRollout\* o, void\* stream\);", text)
    assert re.search(r"int pulse_tfe_mc_evaluate\(const PulseTfeMCEval\* o, void\* stream\);", text)


def test_symmetric_argument_and_cpu_device():
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    with pytest.raises(RuntimeError, match="No CPU fallback"):
        OnPolicyFirstVisitMCTFEGPU(torch.device("cpu"), 64, symmetric=True)
