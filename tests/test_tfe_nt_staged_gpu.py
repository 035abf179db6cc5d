"""The 2048 n-tuple network's weight sets by tile stage on the device (csrc/tfe_ntuple_staged.hip:
pulse_tfe_nt_rollout_staged, pulse_tfe_nt_learn_staged, pulse_tfe_nt_evaluate_staged, pulse_tfe_nt_search_staged, and the apply launches
once per stage) against the host's statement of them: the mirrors of the package handed tuples that carry the stage tiles
(tests/tfe_nt_staged_support.py), under the host game loops of the sibling files.  Every comparison is exact: integers word for word,
float64 and float32 as bit patterns.  Every buffer a launch is handed sits between guard words, and the rows of keys / values / steps /
backed at and beyond a game's length must keep what they held.

Shape: the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), 257 games of at most 256 moves (one full workgroup and one of one lane one ply
deep; 32 workgroups of eight groups and one group under the search), epsilon .25, gamma 1, seed 457, with and without symmetry.  Stages
from tiles 8 and 32 (nibbles 3 and 5), so every game crosses both boundaries in its first few dozen moves; the weights are a seeded
normal array of scale 4 with a slice of its own per stage, divided by 64 (exact) one ply deep so that play is led by the rewards and
games are cut (tests/test_tfe_nt_restart_gpu.py).  Every test of a staged launch asserts first, on the host's side, that every stage was
reached -- keys in it, and for the learners adds in its slice -- so a run in which nothing reached a stage cannot pass quietly."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guarded, guards_intact, read
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_staged_support import STAGE_TILES, UNREACHED, adds_per_stage, boards, staged, staged_weights, stages_struct
from tests.tfe_nt_support import (BOARD_ID0, BUFFERS, GAMES, MAX_STEPS, PER_MOVE, SEED, TUPLES, bits, learner_agent, learner_round, nt, plain_learner,
                                  search_outputs, weights)

pytestmark = pytest.mark.gpu

MODES = {"one_ply": (0, False), "search": (1, False), "backed": (1, True)}  # (layers, backed)
DIVISOR = {0: 64, 1: 1}                                                     # layers: what divides the seeded weights
EPSILON, ROUND = .25, 0
START_PATTERN, BACKED_PATTERN = 0x3C3C3C3C3C3C3C3C, -4321.125              # what `start` and `backed` hold before the first launch
W = 16 ** 4 + 16 ** 6
S = len(STAGE_TILES) + 1


def _seeds():
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return SEED, SEED ^ AGENT_KEY, SEED ^ TIE_KEY


def _upload(t, array):
    import torch
    array = np.array(array)                                                 # (a copy: torch takes no read-only array)
    t.copy_(torch.from_numpy(array.view(np.int64) if array.dtype == np.uint64 else array).reshape(t.shape))


def _agent(layers=0, symmetric=True, tiles=STAGE_TILES, backed=False, w=None, **kw):
    """the agent of the shape between guard words, with a `start` of zeros (and a `backed`) of its own between guard words, and the
    weights of the shape -- a slice per stage -- or `w`"""
    import torch
    a = learner_agent(symmetric=symmetric, stage_tiles=tiles, **kw)
    a._restart_state()
    names = ("start", "restart_stats")
    if backed:
        a.backed, names = torch.zeros_like(a.values), names + ("backed",)
    a = guard(a, names, backed=BACKED_PATTERN)
    _upload(a.weights_dev, staged_weights(TUPLES, len(tiles) + 1, DIVISOR[layers]) if w is None else w)
    return a


def _start_of(a):
    return a.start.cpu().numpy().view(np.uint64)


def _read(a):
    out = read(a, PER_MOVE)
    return dict(out, backed=bits(a.backed.cpu().numpy())) if a.backed is not None else out


def _launched(a, launch):
    """`launch` on the agent; the read-back carries what the per-move rows held before it and the counters' differences"""
    before, st = _read(a), a.stats()
    launch()
    after = a.stats()
    return dict(_read(a), **{k + "_before": v for k, v in before.items() if k in PER_MOVE + ("backed",)}, **{k: after[k] - st[k] for k in ("moves", "truncated")})


# ------------------------------------------------------------------ the games, word for word
@functools.lru_cache(maxsize=None)
def _host_games(layers, symmetric):
    """the host's games of the shape from reset on the staged weights (at one layer with the backed values: recording them does not
    change play), once per session"""
    w = staged_weights(TUPLES, S, DIVISOR[layers])
    zeros = np.zeros(GAMES, dtype=np.uint64)
    want = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, 1.0, w, staged(), symmetric, *_seeds(), BOARD_ID0, ROUND, depth=layers, backed=bool(layers), start=zeros)
    played = np.arange(MAX_STEPS)[:, None] < want["lengths"][None, :]
    per_stage = np.bincount(nt().stage_of_keys_on_host(want["keys"][played], STAGE_TILES), minlength=S)
    print("layers", layers, "symmetric", symmetric, "ended", want["ended"], "cut", want["truncated"], "afterstates per stage", per_stage.tolist())
    assert (per_stage > 0).all() and want["ended"] >= 1 and want["truncated"] >= 1 and not want["start_left"].any()
    plain = nt_games_on_host(GAMES, 32, EPSILON, 1.0, w[:W], TUPLES, symmetric, *_seeds(), BOARD_ID0, ROUND, depth=layers, start=zeros)
    assert not np.array_equal(plain["keys"][:32], want["keys"][:32])         # the stages change play: slice 0 alone plays other games
    return want


def _assert_games(a, got, want, where, backed):
    assert_rollout(got, want, where, PER_MOVE)
    played = np.arange(MAX_STEPS)[:, None] < want["lengths"][None, :]
    assert (~played).any() and (got["keys_before"] == np.uint64(PATTERNS["keys"])).all(), where          # so the rows beyond a game keep the pattern
    if backed:
        assert np.array_equal(got["backed"][played], bits(want["backed"])[played]), where
        assert np.array_equal(got["backed"][~played], got["backed_before"][~played]), where
        assert (got["backed_before"] == bits(np.float64(BACKED_PATTERN))).all(), where
    assert got["moves"] == int(want["lengths"].sum()) and got["truncated"] == want["truncated"], where
    assert not _start_of(a).any(), where
    guards_intact(a)


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_staged_games_are_the_hosts(mode, symmetric):
    """keys, values as float64 bit patterns, step bytes, lengths, scores and counters; `backed` at one layer"""
    layers, backed = MODES[mode]
    want = _host_games(layers, symmetric)
    a = _agent(layers, symmetric, backed=backed)
    got = _launched(a, lambda: a.rollout_staged_launch(layers, backed=backed))
    _assert_games(a, got, want, (mode, symmetric), backed)
    # the public method: the agent's attributes lead to the same launch
    b = _agent(layers, symmetric, backed=backed)
    b.rollout_layers, b.backed_targets = layers, backed
    _assert_games(b, _launched(b, b.rollout), want, (mode, symmetric, "rollout()"), backed)


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
@pytest.mark.parametrize("layers", [0, 1])
def test_the_staged_evaluations_are_the_hosts(layers, symmetric):
    """the 24 words and the per-game arrays: with equal seeds, boards, round and epsilon the evaluation plays the roll-out's games"""
    from pulselib_amd.agents.tfe_ntuple_td_gpu import EVAL_SUMMARY
    from tests.tfe_host import eval_words
    want = _host_games(layers, symmetric)
    a = _agent(layers, symmetric)
    ev = (a.evaluate_search if layers else a.evaluate)(epsilon=EPSILON, board_id0=BOARD_ID0, per_game=True)
    assert np.array_equal(ev["lengths"], want["lengths"]) and np.array_equal(ev["total_score"], want["total_score"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["greedy"], want["capped"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words and ev["games"] == GAMES
    guards_intact(a)


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
def test_the_staged_search_is_the_mirror_bit_for_bit(symmetric):
    import torch
    n, keys = nt(), boards()
    a = _agent(1, symmetric)
    a.round = 3                                                            # (the coins of another round than the games')
    w = staged_weights(TUPLES, S, 1)
    want = n.search_nt_on_host(keys, w, staged(), symmetric, a.gamma, a.tie_seed, a.round)
    stage = n.stage_of_keys_on_host(want["after"].reshape(-1), STAGE_TILES).reshape(-1, 4)
    assert set(stage.ravel().tolist()) == {0, 1, 2} and int((stage.min(axis=1) != stage.max(axis=1)).sum()) >= 2       # moves of one board in two stages
    plain = n.search_nt_on_host(keys, w[:W], TUPLES, symmetric, a.gamma, a.tie_seed, a.round)
    assert not np.array_equal(plain["q"], want["q"])
    dev = torch.device("cuda:0")
    dev_boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    q, action, cand, guards = search_outputs(len(keys), dev)
    a.search_launch(dev_boards, q, action, cand)
    assert np.array_equal(cand.cpu().numpy(), want["candidates"]) and np.array_equal(action.cpu().numpy().astype(np.int64), want["action"])
    assert np.array_equal(bits(q.cpu().numpy()), bits(want["q"]))
    guards_intact(a, [("boards", gb, nb)] + guards)
    out = a.search(keys)
    assert np.array_equal(bits(out["q"]), bits(want["q"])) and np.array_equal(out["action"], want["action"]) and np.array_equal(out["candidates"], want["candidates"])


# ------------------------------------------------------------------ the learners
# (lam, backed, tc): the scatter with the one-step difference formed in the launch (td0*) or given by a walk, without and with acc_abs
FORMS = {"td0": (0.0, False, False), "td0_tc": (0.0, False, True), "lambda": (0.5, False, False), "backed": (0.5, True, False), "backed_tc": (0.5, True, True)}


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
@pytest.mark.parametrize("form", list(FORMS))
def test_a_staged_learner_adds_what_the_host_adds(form, symmetric):
    """all S * W accumulator cells (and acc_abs with tc) and the counters, on the records of the device's own staged roll-out; the backed
    learners read a `backed` of seeded values in place of a search's (the learner reads it as numbers).  The five forms with and
    without symmetry launch each of the eight scatter kernels at least once."""
    n, (lam, backed, tc) = nt(), FORMS[form]
    a = _agent(0, symmetric, backed=backed, extra_buffers=("acc_abs",), tc=tc)
    a.rollout()
    got = read(a, PER_MOVE)
    L, values = got["lengths"].astype(np.int64), got["values"].view(np.float64)
    records = (got["keys"], values, got["steps"], L, a.tuples, symmetric, 1.0)
    host_acc, host_abs = np.zeros((S * W, 2), dtype=np.int64), (np.zeros(S * W, dtype=np.int64) if tc else None)
    if backed:
        seeded = np.random.default_rng(23).standard_normal(values.shape) * 8
        _upload(a.backed, seeded)
        host = n.learn_backed_nt_on_host(got["keys"], values, seeded, got["steps"], L, a.tuples, symmetric, 1.0, lam, host_acc, host_abs)
    elif tc:
        host = n.learn_tc_nt_on_host(*records, lam, host_acc, host_abs)
        assert a.deltas is None                                             # TD(0) with tc: no walk, the difference is formed in the scatter
    elif lam:
        host = n.learn_lambda_nt_on_host(*records, lam, host_acc)
    else:
        host = n.learn_nt_on_host(*records, host_acc)
    per_stage = adds_per_stage(host_acc, S)
    print(form, "adds per stage", per_stage, {k: host[k] for k in ("learnt", "skipped", "clamped")})
    assert all(x > 0 for x in per_stage) and host["skipped"] >= 1
    before = a.stats()
    a.learn_staged_launch(lam, backed=backed, tc=tc)
    st = a.stats()
    assert {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")} == {k: host[k] for k in ("learnt", "skipped", "clamped")}
    assert np.array_equal(a.acc.cpu().numpy(), host_acc)
    if tc:
        assert np.array_equal(a.acc_abs.cpu().numpy(), host_abs) and host_abs.any()
    if lam:
        played = np.arange(MAX_STEPS)[:, None] < L[None, :]
        assert np.array_equal(bits(a.deltas.cpu().numpy())[played], bits(host["deltas"])[played])
    after = read(a, PER_MOVE)
    assert all(np.array_equal(after[k], got[k]) for k in got)              # the records are only read
    guards_intact(a)
    # learn(): the agent's attributes lead to the same launch
    a.acc.zero_()
    a.lam, a.backed_targets = lam, backed
    a.learn()
    assert np.array_equal(a.acc.cpu().numpy(), host_acc)
    assert (a.deltas is None) == (form in ("td0", "td0_tc"))


def test_three_staged_rounds_are_the_hosts():
    """lambda .5 with tc: per round acc and acc_abs over all S * W cells, the counters, the weights as float32 bit patterns after the
    apply launches of the three stages and what they added to tc_stats (learner_round, the host's learner and apply on tuples that
    carry the stages), at the end E and A; then learn_batch() three times on a twin agent leaves the same weights and records."""
    import torch
    kw = dict(lam=0.5, tc=True, stage_tiles=STAGE_TILES)
    a = learner_agent(extra_buffers=("deltas", "acc_abs", "E", "A", "tc_stats"), **kw)
    b = plain_learner(**kw)
    assert a.weights_dev.shape == (S * W,) and a.acc.shape == (S * W, 2) and a.E.shape == a.A.shape == a.acc_abs.shape == (S * W,) and a.n_weights == W
    coherence = (np.zeros(S * W), np.zeros(S * W))
    learnt = lambda a, h: dict(per_stage=adds_per_stage(h.host_acc, S), abs_equal=np.array_equal(h.acc_abs, h.host_abs), abs_any=bool(h.host_abs.any()))
    applied = lambda a, h: dict(tc_stats=a.tc_stats.cpu().tolist(), host_tc=h.host_tc)     # tc_stats adds up over the stages' launches and the rounds
    recs = [learner_round(a, after_learn=learnt, after_apply=applied, coherence=coherence) for _ in range(3)]
    print([{k: rec[k] for k in ("ended", "cut", "moves", "per_stage", "host", "stats", "moved", "tc_stats", "host_tc")} for rec in recs])
    moved = rho = 0
    for rec in recs:
        assert all(x > 0 for x in rec["per_stage"]), rec["per_stage"]
        assert rec["abs_equal"] and rec["abs_any"], rec
        moved, rho = moved + rec["host_tc"][0], rho + rec["host_tc"][1]
        assert rec["tc_stats"] == [moved, rho, 0, 0] and rec["host_tc"][0] == rec["moved"] and 0 < rec["host_tc"][1] <= rec["moved"] << 32, rec
        assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["stats"] == {k: rec["host"][k] for k in rec["stats"]}, rec
        assert rec["ended"] >= 1 and rec["cut"] >= 1 and rec["moved"] > 0, rec
    E, A = a.coherence()
    assert np.array_equal(bits(E), bits(coherence[0])) and np.array_equal(bits(A), bits(coherence[1]))
    w = a.weights().reshape(S, W)
    assert all(w[s].any() for s in range(S)) and not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2])
    guards_intact(a)
    for _ in range(3):
        b.learn_batch()
    assert a.round == b.round == 3 and b.start is not None and not b.start.any().item()
    for k in ("weights_dev", "E", "A", "tc_stats", "lengths", "total_score", "episode_reward", "counters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------ equal slices: the one-stage network
def _bytes_equal(a, b, names):
    import torch
    for k in names:
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k


@pytest.mark.parametrize("mode", list(MODES))
def test_on_equal_slices_the_staged_launches_are_their_siblings(mode):
    """rollout_from, evaluate and evaluate_search, search, and the learners' acc summed over the slices; then n_stages = 1 on the same
    structs: the parent's outputs byte for byte"""
    import torch
    from pulselib_amd import _native
    (layers, backed), one = MODES[mode], weights("seeded") / np.float32(DIVISOR[MODES[mode][0]])
    a = _agent(layers, True, backed=backed, w=np.tile(one, S))
    b = _agent(layers, True, tiles=(), backed=backed, w=one)
    c = _agent(layers, True, tiles=(), backed=backed, w=one)               # the parent's struct through the staged entry points at n_stages = 1
    assert b.stage_tiles == () and b.weights_dev.shape == (W,) and type(b.tuples) is tuple
    one_stage = stages_struct(())
    a.rollout_staged_launch(layers, backed=backed)
    b.rollout_from_launch(layers, backed=backed)
    c._launch("pulse_tfe_nt_rollout_staged", c._rollout_struct(), C.byref(one_stage), layers, c.backed.data_ptr() if backed else None, c.start.data_ptr())
    records = ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters", "start") + (("backed",) if backed else ())
    _bytes_equal(a, b, records)
    _bytes_equal(c, b, records)
    played = np.arange(MAX_STEPS)[:, None] < b.lengths.cpu().numpy()[None, :]
    per_stage = np.bincount(nt().stage_of_keys_on_host(b.keys.cpu().numpy().view(np.uint64)[played], STAGE_TILES), minlength=S)
    assert (per_stage > 0).all() and int(b.lengths.min().item()) < MAX_STEPS == int(b.lengths.max().item())
    # the learner of the mode
    lam = 0.5 if layers else 0.0
    a.learn_staged_launch(lam, backed=backed)
    o = c._moves(_native.TfeNtLearnBacked())
    o.lam = lam
    if layers:
        b.learn_backed_launch(lam) if backed else b.learn_lambda_launch(lam)
        c.deltas = torch.zeros_like(c.values)
        o.deltas, o.backed = c.deltas.data_ptr(), (c.backed.data_ptr() if backed else None)
    else:
        b.learn()
    c._launch("pulse_tfe_nt_learn_staged", o, C.byref(one_stage))
    slices = a.acc.reshape(S, W, 2)
    assert torch.equal(slices.sum(dim=0), b.acc) and all(bool(slices[s, :, 1].any().item()) for s in range(S)) and torch.equal(c.acc, b.acc)
    _bytes_equal(a, b, ("counters",) + (("deltas",) if layers else ()))
    _bytes_equal(c, b, ("counters",) + (("deltas",) if layers else ()))
    # the evaluation at the mode's depth
    ev = lambda x: (x.evaluate_search if layers else x.evaluate)(epsilon=EPSILON, per_game=True)
    ea, eb = ev(a), ev(b)
    e = c._draws(c._eval_struct(), c.eval_board_id0())
    e.n_games, e.max_steps, e.epsilon = GAMES, MAX_STEPS, EPSILON
    c.eval_counters(clear=True)
    e.summary, e.max_tile_hist = c._eval.data_ptr(), c._eval[8:].data_ptr()
    c._launch("pulse_tfe_nt_evaluate_staged", e, C.byref(one_stage), layers)
    for k in ea:
        assert np.array_equal(ea[k], eb[k]), k
    assert c.eval_counters() == {k: v for k, v in eb.items() if k not in ("total_score", "lengths")}
    if layers:
        keys = boards()
        sa, sb = a.search(keys), b.search(keys)
        q = torch.zeros((len(keys), 4), dtype=torch.float64, device=c.device)
        action, cand = torch.zeros(len(keys), dtype=torch.int8, device=c.device), torch.zeros(len(keys), dtype=torch.uint8, device=c.device)
        dev_boards = torch.from_numpy(keys.view(np.int64).copy()).to(c.device)
        c._launch("pulse_tfe_nt_search_staged", c._search_struct(dev_boards, q, action, cand), C.byref(one_stage))
        for k, t in (("q", q), ("action", action), ("candidates", cand)):
            assert np.array_equal(bits(sa[k]) if k == "q" else sa[k], bits(sb[k]) if k == "q" else sb[k]), k
            assert np.array_equal(t.cpu().numpy().reshape(sb[k].shape).view(np.uint8), sb[k].view(np.uint8)), k
    guards_intact(a, b, c)


# ------------------------------------------------------------------ a stage nobody reaches, and a stage added half-way
def test_a_stage_no_game_reaches_is_left_untouched():
    """stages from tiles 8 and 16,384: three rounds move the first two slices and leave the third slice's weights and accumulators as
    they were, to the last word"""
    import torch
    a = _agent(0, True, tiles=(8, UNREACHED), extra_buffers=("acc_abs", "E", "A", "tc_stats", "deltas"), lam=0.5, tc=True)
    pattern = (np.random.default_rng(31).standard_normal(W) * 4).astype(np.float32)
    _upload(a.weights_dev[2 * W:], pattern)
    a.acc[2 * W:] = 0x1234                                                  # nothing adds here, and its apply launch finds cnt > 0 ...
    a.acc[2 * W:, 1] = 0                                                    # ... nowhere: cnt = 0
    for _ in range(3):
        a.learn_batch()
    played = np.arange(MAX_STEPS)[:, None] < a.lengths.cpu().numpy()[None, :]
    reached = nt().stage_of_keys_on_host(a.keys.cpu().numpy().view(np.uint64)[played], (8, UNREACHED))
    assert set(reached.tolist()) == {0, 1} and a.round == 3                 # no game of the last round reached the tile (nor of the others: the slice below)
    w = a.weights().reshape(3, W)
    assert np.array_equal(w[2].view(np.uint32), pattern.view(np.uint32))
    acc = a.acc.reshape(3, W, 2)
    assert bool((acc[2, :, 0] == 0x1234).all().item()) and not acc[2, :, 1].any().item() and not acc[:2].any().item()
    assert not a.acc_abs[2 * W:].any().item() and not a.E[2 * W:].any().item() and not a.A[2 * W:].any().item()
    assert a.E[:W].any().item() and a.E[W:2 * W].any().item()
    start = staged_weights(TUPLES, 3, DIVISOR[0]).reshape(3, W)
    assert not np.array_equal(w[0], start[0]) and not np.array_equal(w[1], start[1])
    guards_intact(a)


def test_add_stage_in_the_middle_of_a_run_changes_no_evaluation():
    """two rounds with stages from tile 8 under lambda .5 and tc, add_stage(32), and the evaluations one ply deep and under the search
    are what they were before it: every counter and every game; the next round then learns in three slices"""
    import torch
    a = plain_learner(lam=0.5, tc=True, stage_tiles=(8,))
    for _ in range(2):
        a.learn_batch()
    before = [a.evaluate(per_game=True), a.evaluate_search(n_games=33, per_game=True)]
    w, (E, A) = a.weights().reshape(2, W), [x.reshape(2, W) for x in a.coherence()]
    assert w[0].any() and w[1].any()
    a.add_stage(32)
    assert a.stage_tiles == (8, 32) and a.tuples.stage_tiles == (8, 32) and a.weights_dev.shape == (3 * W,) and a.acc.shape == (3 * W, 2)
    grown = a.weights().reshape(3, W)
    assert np.array_equal(grown[0].view(np.uint32), w[0].view(np.uint32)) and all(np.array_equal(grown[s].view(np.uint32), w[1].view(np.uint32)) for s in (1, 2))
    gE, gA = [x.reshape(3, W) for x in a.coherence()]
    assert np.array_equal(bits(gE[2]), bits(E[1])) and np.array_equal(bits(gA[2]), bits(A[1])) and np.array_equal(bits(gE[0]), bits(E[0]))
    assert not a.acc.any().item() and not a.acc_abs.any().item()
    after = [a.evaluate(per_game=True), a.evaluate_search(n_games=33, per_game=True)]
    for x, y in zip(before, after):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    with pytest.raises(ValueError, match="begins at tile 32 already"):
        a.add_stage(32)
    a.learn_batch()
    moved = a.weights().reshape(3, W)
    assert not np.array_equal(moved[1], moved[2]) and a.round == 3
    # an agent without stages is promoted the same way
    b = plain_learner()
    b.learn_batch()
    ev = b.evaluate(per_game=True)
    b.add_stage(64)
    assert b.stage_tiles == (64,) and b.n_stages == 2 and all(np.array_equal(ev[k], v) for k, v in b.evaluate(per_game=True).items())
    b.learn_batch()


# ------------------------------------------------------------------ restarts
def test_a_restarted_staged_round_is_the_hosts():
    """one round from reset, its pick, and the round from `start`: the games from the picked boards with V read by stage, the `start` the
    launch leaves, and acc over all S * W cells"""
    n = nt()
    a = _agent(0, True, lam=0.5, extra_buffers=("deltas",))
    a.restart_fraction, a.restart_min_length = 0.5, 128
    _upload(a.start, np.full(GAMES, START_PATTERN, dtype=np.uint64))        # restarts are on: the first round plays from what `start` holds
    a.start.zero_()
    a.learn_batch()
    got = read(a, PER_MOVE)
    left, picked = n.restart_pick_on_host(got["keys"], got["lengths"], MAX_STEPS, a.env_seed, a.round_board_id0(0), 0.5, 128)
    print("picked", picked, "of", GAMES)
    assert 8 <= picked[0] <= GAMES - 8 and np.array_equal(_start_of(a), left) and a.round == 1
    policy = a.weights()
    got = _launched(a, a.rollout)
    want = nt_games_on_host(GAMES, MAX_STEPS, EPSILON, 1.0, policy, a.tuples, True, *_seeds(), a.round_board_id0(), a.round, start=left)
    kept = want["start_left"]
    assert_rollout(got, want, "round 1", PER_MOVE)
    assert np.array_equal(_start_of(a), kept) and np.array_equal(kept, left) and got["moves"] == int(want["lengths"].sum())
    first = n.stage_of_keys_on_host(want["keys"][0], STAGE_TILES)
    assert (first[left != 0] > 0).all() and (first[left == 0] == 0).any()   # restarted games begin in a later stage
    host_acc = np.zeros((S * W, 2), dtype=np.int64)
    host = n.learn_lambda_nt_on_host(got["keys"], got["values"].view(np.float64), got["steps"], got["lengths"].astype(np.int64), a.tuples, True, 1.0, 0.5, host_acc)
    assert all(x > 0 for x in adds_per_stage(host_acc, S)) and host["learnt"] > 0
    a.learn()
    assert np.array_equal(a.acc.cpu().numpy(), host_acc)
    guards_intact(a)
