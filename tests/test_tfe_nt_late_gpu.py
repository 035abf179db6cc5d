"""The 2048 n-tuple network's three newest units on the device, at the limits and on late boards: weight sets
by tile stage (section 13.9; csrc/tfe_ntuple_staged.hip), games continued across rounds (section 13.10; csrc/tfe_ntuple_continue.hip)
and the search whose depth the empty cells choose (section 13.11; csrc/tfe_ntuple_search.hip), against the host's statement of
them.  Every comparison is exact: integers word for word, float64 and float32 as bit patterns.  Every buffer a launch is handed sits
between guard words, and the rows of keys / values / steps / backed at and beyond a game's length must keep what they held.  The
premises a case rests on -- stages reached, games capped, dead and cut, boards deep and shallow -- are the HOST's counts, asserted
where tests/tfe_nt_late_support.py makes the host's games; tests/test_tfe_nt_late_cpu.py asserts the same floors without a GPU and
prints the counts quoted below.

What the sibling files of the three units never ran, and this one does: PULSE_TFE_NT_MAX_STAGES = 4 stages; thresholds at the nibbles
1, 14 and 15; boards in the top stage because they hold the 32,768 tile; 1,188,368 weights per stage, no multiple of 256, so every
stage's apply launch begins inside a workgroup's stride; stage offsets up to 3 * 33,685,504; the pick's capped, dead-at-max_steps and
capped-at-max_steps games, max_steps = 2 and a `start` of late boards; the adaptive search at "eight" and "one6", with 8 images and
with 1, on boards with nibble 15 and few empty cells.

Regime (tests/tfe_nt_late_support.py): late_start(65, 3), 96 moves, epsilon .25, gamma 1, seed 457 (459 for "eight" with 8 images under
the search, where 457 cuts 7 games), round 0 on the boards 3000..; weights staged_weights(tuples, 4, divisor), / 64 one ply deep.
Rehearsed on the host, afterstates per stage, then games capped / dead / cut at move 96 without the cap (moves):
  eight, 8 images: one ply 61 / 1,564 / 323 / 25, 25 / 25 / 15 (1,973); search and backed 109 / 1,531 / 311 / 25, 25 / 30 / 11 (1,976)
  eight, 1 image: one ply 64 / 1,597 / 312 / 26, 26 / 23 / 16 (1,999); search and backed 98 / 1,553 / 367 / 28, 28 / 23 / 14 (2,046)
  one6, 1 image, one ply: 65 / 1,588 / 308 / 28, 28 / 23 / 14 (1,989)
  eight, 8 images, one ply under the tiles (2, 256, 16384): 0 / 1,480 / 106 / 357, 26 / 26 / 13 (1,943)"""
import time

import numpy as np
import pytest

from tests import tfe_nt_late_support as late
from tests.test_tfe_nt_adaptive_gpu import SEARCH, _launch_boards
from tests.test_tfe_nt_continue_gpu import _assert_state, _with_continue
from tests.test_tfe_nt_restart_gpu import _assert_games, _launched, _set_start, _start_of, _with_restart
from tests.tfe_gpu_support import PER_GAME, assert_rollout, guard, guarded, guards_intact, read
from tests.tfe_nt_staged_support import adds_per_stage
from tests.tfe_nt_support import BOARD_ID0, PER_MOVE, SEED, SHAPES, bits, late_start, learner_agent, nt, search_agent, search_outputs

pytestmark = pytest.mark.gpu

SETTINGS = {"td0": dict(lam=0.0), "lambda.5-tc": dict(lam=0.5, tc=True)}
TC_STATE = ("deltas", "acc_abs", "E", "A", "tc_stats")
LEARN_CASES = [case + ("td0",) for case in late.ROLLOUT_CASES] + [("eight", True, mode, "lambda.5-tc") for mode in late.MODES]
SEARCH_CASES = [("eight", True), ("eight", False), ("one6", True), ("one6", False)]
IMAGES = {True: "8_images", False: "1_image"}


def _upload(t, array):
    import torch
    array = np.array(array)                                                 # (a copy: torch takes no read-only array)
    t.copy_(torch.from_numpy(array.view(np.int64) if array.dtype == np.uint64 else array).reshape(t.shape))


def _agent(shape, symmetric, layers, tiles=late.LATE_TILES, games=late.GAMES, max_steps=late.MAX_STEPS, seed=SEED, backed=False, **kw):
    """the agent of a case on four stages, every buffer between guard words -- `deltas` too where the backed learner would allocate it
    -- with the shape's weights, a slice per stage"""
    import torch
    a = learner_agent(games, tuples=SHAPES[shape], symmetric=symmetric, stage_tiles=tiles, max_steps=max_steps, seed=seed, epsilon=late.EPSILON, **kw)
    if backed and a.deltas is None:
        a.deltas = torch.zeros_like(a.values)
    a = guard(a, tuple(k for k in TC_STATE if getattr(a, k) is not None))
    assert a.n_stages == late.S and a.weights_dev.shape == (late.S * a.n_weights,) and a.acc.shape == (late.S * a.n_weights, 2)
    _upload(a.weights_dev, late.late_weights(shape, layers))
    return a


# ------------------------------------------------------------------ 1. four stages on late boards: the games, the learners, the apply launches
def _play(a, g, layers, backed, where):
    """pulse_tfe_nt_rollout_staged from late_start(65, 3): every record, the counters, `backed`, the `start` left and the rows beyond"""
    _set_start(a, late_start(late.GAMES, 3))
    got = _launched(a, lambda: a.rollout_staged_launch(layers, backed=backed))
    _assert_games(a, got, g.want, g.left, where, backed)
    return got


def _learn_and_apply(a, g, backed, where, state=None):
    """One learn and the apply launches of the four stages on the device's own records, the terminal bit set in every second capped
    game's last byte (with_dead_caps: the only way a move is learnt in stage 3): all 4 W cells of acc, with tc acc_abs, E, A and
    tc_stats, deltas where there are any, the counters, the weights as bit patterns; the records and `start` as they were.  state: what
    the host's acc, acc_abs, E and A hold before the launch (zero, or the device's patterns).  Returns the host's adds per stage."""
    n = nt()
    steps, marked = late.with_dead_caps(a.steps.cpu().numpy(), g)
    _upload(a.steps, steps)
    rec, policy, before = read(a, PER_MOVE), a.weights(), a.stats()
    a.backed_targets = backed
    a.learn()
    acc, st = a.acc.cpu().numpy(), a.stats()
    state = state or {}
    host_acc = state.get("acc", np.zeros_like(acc)).copy()
    host_abs = state.get("acc_abs", np.zeros(len(acc), dtype=np.int64)).copy() if a.tc else None
    records = (rec["keys"], rec["values"].view(np.float64), rec["steps"], g.L, a.tuples, a.symmetric, a.gamma)
    if backed:
        learn = lambda acc, ab: n.learn_backed_nt_on_host(*records[:2], a.backed.cpu().numpy(), *records[2:], a.lam, acc, ab)
    elif a.tc:
        learn = lambda acc, ab: n.learn_tc_nt_on_host(*records, a.lam, acc, ab)
    else:
        learn = lambda acc, ab: n.learn_nt_on_host(*records, acc)
    host = learn(host_acc, host_abs)
    per_stage = adds_per_stage(host_acc, late.S)                            # (a pattern in `state` has cnt = 0)
    stats = {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")}
    print(where, "adds per stage", per_stage, "capped games learnt", len(marked), "learn", stats)
    skipped = int((rec["steps"][g.L - 1, np.arange(a.n_games)] >> 7 == 0).sum())
    assert len(marked) >= 4 and host["skipped"] == skipped >= late.FLOOR["cut"] + 4 and host["learnt"] + host["skipped"] == g.counts["moves"], where
    assert stats == {k: host[k] for k in stats} and np.array_equal(acc, host_acc), where
    if a.tc:
        assert np.array_equal(a.acc_abs.cpu().numpy(), host_abs) and host_abs.any(), where
    if a.deltas is not None:
        assert np.array_equal(bits(a.deltas.cpu().numpy())[g.played], bits(host["deltas"])[g.played]), where
    a.apply()
    host_w = policy.copy()
    if a.tc:
        E, A = state.get("E", np.zeros(len(acc))).copy(), state.get("A", np.zeros(len(acc))).copy()
        moved = n.apply_tc_nt_on_host(host_w, host_acc, host_abs, E, A, a.alpha / a.n_features)
        got_E, got_A = a.coherence()
        assert np.array_equal(bits(got_E), bits(E)) and np.array_equal(bits(got_A), bits(A)) and tuple(a.tc_stats.cpu().tolist()) == moved + (0, 0), where
        assert np.array_equal(a.acc_abs.cpu().numpy(), host_abs) and moved[0] > 0, where
    else:
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0, where
    weights = a.weights()
    assert np.array_equal(weights.view(np.uint32), host_w.view(np.uint32)) and np.array_equal(a.acc.cpu().numpy(), host_acc), where
    W = a.n_weights
    moved_per_stage = [int((weights[s * W:(s + 1) * W].view(np.uint32) != policy[s * W:(s + 1) * W].view(np.uint32)).sum()) for s in range(late.S)]
    assert all((m > 0) == (x > 0) for m, x in zip(moved_per_stage, per_stage)), (where, moved_per_stage, per_stage)
    after = read(a, PER_MOVE)
    assert all(np.array_equal(after[k], rec[k]) for k in PER_MOVE + PER_GAME) and np.array_equal(_start_of(a), g.left), where     # only read
    guards_intact(a)
    return per_stage


@pytest.mark.parametrize("shape,symmetric,mode,learner", LEARN_CASES, ids=["-".join((s, IMAGES[y], m, l)) for s, y, m, l in LEARN_CASES])
def test_four_stages_on_late_boards_are_the_hosts(shape, symmetric, mode, learner):
    """pulse_tfe_nt_rollout_staged from late_start(65, 3) under LATE_TILES, then pulse_tfe_nt_learn_staged -- TD(0), with "lambda.5-tc"
    the walk and acc_abs, in the backed mode the backed walk -- and the apply launches, once per stage.  On the host first (the module's
    docstring has the counts): every stage holds at least 20 recorded afterstates, at least 8 games are capped, 8 dead and 8 cut
    without the cap, and stage 3 holds the capping moves alone, their bytes without a terminal bit -- so the roll-out's own records add
    nothing to the top slice, and every second of those bytes gets the bit before the learner runs.  Adds per stage then, TD(0), one
    ply: eight with 8 images 3,904 / 99,136 / 20,672 / 832, with 1 image 512 / 12,648 / 2,496 / 104, one6 65 / 1,574 / 308 / 14."""
    (layers, backed) = late.MODES[mode]
    where = (shape, symmetric, mode, learner)
    g = late.late_games(shape, symmetric, layers)
    a = _with_restart(_agent(shape, symmetric, layers, seed=g.seed, backed=backed, **SETTINGS[learner]), backed)
    _play(a, g, layers, backed, where)
    values = a.values.cpu().numpy()
    top = g.played & (g.stage == 3)
    assert np.unique(values[top]).size >= late.FLOOR["capped"] // 2 and values[top].all(), where      # V of the capping moves: read in the top slice
    per_stage = _learn_and_apply(a, g, backed, where)
    assert all(x > 0 for x in per_stage), (where, per_stage)


def test_under_a_threshold_at_nibble_one_stage_zero_is_left_untouched():
    """The tiles (2, 256, 16384): every board with a tile is in stage 1 or above.  "eight" with 8 images, one ply, lambda .5 with tc:
    the games, then the learn and the four apply launches with slice 0 of the weights, of acc (sums with cnt 0), of acc_abs, of E and of
    A holding patterns -- all 4 W cells of each are the host's, and slice 0 is bit for bit what it held."""
    tiles, where = late.LOW_TILES, "low tiles"
    g = late.late_games("eight", True, 0, tiles)
    a = _with_restart(_agent("eight", True, 0, tiles=tiles, **SETTINGS["lambda.5-tc"]))
    W, rng = a.n_weights, np.random.default_rng(31)
    state = dict(acc=np.zeros((late.S * W, 2), dtype=np.int64), acc_abs=np.zeros(late.S * W, dtype=np.int64), E=np.zeros(late.S * W), A=np.zeros(late.S * W))
    state["acc"][:W, 0], state["acc_abs"][:W] = 0x1234, 0x4321               # nothing adds here, and the apply launch finds cnt = 0
    state["E"][:W], state["A"][:W] = rng.standard_normal(W), np.abs(rng.standard_normal(W)) + 1.0
    for k, v in state.items():
        _upload(getattr(a, k), v)
    w0 = a.weights()[:W].copy()
    _play(a, g, 0, False, where)
    per_stage = _learn_and_apply(a, g, False, where, state)
    assert per_stage[0] == 0 and all(x > 0 for x in per_stage[1:]), per_stage
    E, A = a.coherence()
    assert np.array_equal(a.weights()[:W].view(np.uint32), w0.view(np.uint32)) and np.array_equal(a.acc[:W].cpu().numpy(), state["acc"][:W])
    assert np.array_equal(a.acc_abs[:W].cpu().numpy(), state["acc_abs"][:W]) and np.array_equal(bits(E[:W]), bits(state["E"][:W]))
    assert np.array_equal(bits(A[:W]), bits(state["A"][:W])) and E[W:].any() and not a.acc[W:].any().item()
    guards_intact(a)


@pytest.mark.parametrize("tiles", [late.LATE_TILES, late.LOW_TILES], ids=["late_tiles", "low_tiles"])
@pytest.mark.parametrize("shape,symmetric", SEARCH_CASES, ids=["-".join((s, IMAGES[y])) for s, y in SEARCH_CASES])
def test_the_staged_search_on_late_boards_is_the_mirror(shape, symmetric, tiles):
    """pulse_tfe_nt_search_staged on the 123 boards of late_boards() -- the crafted boards, the 49 boards of late_start(65, 3) and the
    afterstates 12 moves into the games -- on the seeded slices: q as bit patterns, actions, candidates.  On the host first: under
    LATE_TILES the boards and their afterstates are in all four stages and 24 boards have candidate afterstates in two stages (the floor
    is 8); under (2, 256, 16384) the stages are 1 to 3 and 6 boards have such a pair (the floor is 4: tests/tfe_nt_late_support.py)."""
    import torch
    want, split = late.staged_search(shape, symmetric, tiles)
    keys = late.late_boards()
    a = _agent(shape, symmetric, 1, tiles=tiles, games=7, max_steps=16)
    a.round = late.SEARCH_ROUND
    assert a.tie_seed == late.seeds(SEED)[2]
    dev = torch.device("cuda:0")
    boards, gb, nb = guarded(torch.from_numpy(keys.view(np.int64).copy()).to(dev))
    q, action, cand, guards = search_outputs(len(keys), dev)
    a.search_launch(boards, q, action, cand)
    assert np.array_equal(cand.cpu().numpy(), want["candidates"]) and np.array_equal(action.cpu().numpy().astype(np.int64), want["action"])
    assert np.array_equal(bits(q.cpu().numpy()), bits(want["q"])) and np.array_equal(boards.cpu().numpy().view(np.uint64), keys)
    guards_intact(a, [("boards", gb, nb)] + guards)
    out = a.search(keys)
    assert np.array_equal(bits(out["q"]), bits(want["q"])) and np.array_equal(out["action"], want["action"]) and np.array_equal(out["candidates"], want["candidates"])


def test_one_round_of_the_default_network_on_four_stages_equals_the_host():
    """The largest offsets: the shipping network times four stages is 134,742,016 weights, 539 MB, and an acc of 2.16 GB; stage 3 begins
    at weight 101,056,512.  One TD(0) round of the 65 late games, symmetric, one ply: the games, then acc at every cell the host visits
    and the counts of cells with adds and of non-zero words over all of acc (formed on the device: no dense pass on the host, whose acc
    is touched at the visited cells alone), then the four apply launches: the weights at the visited cells as bit patterns, the count
    of weights that changed, acc zero.  Cost: the seeded weights are drawn on the host once (134,742,016 normals: up to 5 s of one
    core) and uploaded, and the guarded acc is 2.16 GB of device memory; on an MI355X the case took 1.5 s in all (one run).
    Rehearsed on the host: afterstates per stage 63 / 1,537 / 291 / 25, games capped / dead / cut 25 / 28 / 12 in 1,916 moves; the
    learner visits 112 / 13,012 / 4,719 / 385 cells of the four slices, the largest at index 134,662,336."""
    import torch
    start_time = time.perf_counter()
    n = nt()
    g = late.late_games("default", True, 0)
    a = _with_restart(_agent("default", True, 0))
    W = a.n_weights
    assert W == 33685504 and a.total_weights == 134742016 and a.n_features == 32
    _play(a, g, 0, False, "default")
    steps, marked = late.with_dead_caps(a.steps.cpu().numpy(), g)
    _upload(a.steps, steps)
    rec, before, w0 = read(a, PER_MOVE), a.stats(), a.weights_dev.clone()
    a.learn()
    host_acc = np.zeros((late.S * W, 2), dtype=np.int64)                    # (zero pages until touched)
    host = n.learn_nt_on_host(rec["keys"], rec["values"].view(np.float64), rec["steps"], g.L, a.tuples, True, 1.0, host_acc)
    learnt = g.played.copy()
    learnt[g.L - 1, np.arange(late.GAMES)] = rec["steps"][g.L - 1, np.arange(late.GAMES)] >> 7 != 0
    visited = np.unique(n.feature_indices_on_host(rec["keys"][learnt], a.tuples, True))
    per_stage = np.bincount(visited // W, minlength=late.S).tolist()
    print("default on four stages: cells visited per stage", per_stage, "largest index", int(visited.max()), host)
    assert all(x > 0 for x in per_stage) and int(visited.max()) >= 3 * W + 16 ** 4 and len(marked) >= 4 and host["learnt"] == int(learnt.sum())
    st, at = a.stats(), torch.from_numpy(visited).to(a.device)
    assert {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")} == host
    sub = host_acc[visited]
    assert np.array_equal(a.acc[at].cpu().numpy(), sub) and (sub[:, 1] > 0).all()
    assert int(torch.count_nonzero(a.acc[:, 1]).item()) == len(visited) and int(torch.count_nonzero(a.acc).item()) == int(np.count_nonzero(sub))
    assert int(a.acc[:, 1].sum().item()) == a.n_features * host["learnt"]
    a.apply()
    sub_w = w0[at].cpu().numpy()
    old = sub_w.copy()
    assert n.apply_nt_on_host(sub_w, sub, a.alpha / a.n_features) == len(visited)
    assert np.array_equal(a.weights_dev[at].cpu().numpy().view(np.uint32), sub_w.view(np.uint32)) and not a.acc.any().item()
    changed = int(torch.count_nonzero(a.weights_dev.view(torch.int32) != w0.view(torch.int32)).item())
    assert changed == int((sub_w.view(np.uint32) != old.view(np.uint32)).sum()) > 0
    guards_intact(a)
    print("default on four stages: wall s", time.perf_counter() - start_time)


def test_a_four_stage_checkpoint_continues_bit_for_bit(tmp_path):
    """"eight" on four stages with lambda .5 and tc: one late round, save, load -- format version 5, stage_tiles of three, E and A --
    and two more rounds on either agent leave the same weights, E, A and records."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    from pulselib_amd.agents.tfe_ntuple_td_gpu import CHECKPOINT_VERSION_STAGED
    kw = dict(tuples=SHAPES["eight"], epsilon=late.EPSILON, max_steps=late.MAX_STEPS, seed=SEED, board_id0=BOARD_ID0, lam=0.5, tc=True)
    a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), late.GAMES, stage_tiles=late.LATE_TILES, **kw)
    _upload(a.weights_dev, late.late_weights("eight", 0))
    a._restart_state()
    _set_start(a, late_start(late.GAMES, 3))
    a.rollout_staged_launch(0)
    a.learn().apply()
    a.round += 1
    assert all(a.E[s * a.n_weights:(s + 1) * a.n_weights].any().item() for s in range(3)) and int(a.lengths.min().item()) < late.MAX_STEPS
    path = tmp_path / "late.npz"
    a.save(path)
    with np.load(path) as f:
        assert int(f["version"]) == CHECKPOINT_VERSION_STAGED == 5 and f["stage_tiles"].tolist() == list(late.LATE_TILES) and len(f["tc_index"]) > 0
    b = NTupleTDAfterstateTFEGPU.load(path, a.device)
    assert b.stage_tiles == late.LATE_TILES and b.n_stages == 4 and b.tc and b.lam == 0.5 and b.round == 1 and b.start is None
    for k in ("weights_dev", "E", "A"):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k
    for _ in range(2):
        a.learn_batch()
        b.learn_batch()
    assert a.round == b.round == 3 and not a.start.any().item()
    for k in ("weights_dev", "E", "A", "lengths", "total_score", "episode_reward"):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k
    played = (torch.arange(a.max_steps, device=a.device)[:, None] < a.lengths[None, :])
    for k in PER_MOVE:
        assert torch.equal(getattr(a, k)[played], getattr(b, k)[played]), k
    assert not torch.equal(a.weights_dev, torch.from_numpy(np.array(late.late_weights("eight", 0))).to(a.device))


# ------------------------------------------------------------------ 2. the pick of continued games at its three-way branch
@pytest.mark.parametrize("case", list(late.CONTINUE_CASES))
def test_five_continued_rounds_from_late_boards_are_the_hosts(case):
    """pulse_tfe_nt_continue_pick after pulse_tfe_nt_rollout_staged, five rounds from a `start` of late_start(games, 3) on "eight" with
    LATE_TILES under fixed weights, round r on the boards 3000 + games * r: per round the games from the `start` the pick before left,
    then `start`, both carries, the 24 words of `finished` and the guard words; the records are left as read.  Rounds 0 and 4 also run
    pulse_tfe_nt_learn_staged with tc at lambda .5 (in the backed case the backed walk): acc and acc_abs over 4 W cells, the cut and
    the capped games' last moves skipped.  On the host first (tests/test_tfe_nt_late_cpu.py prints them), games capped / capped at
    move max_steps / dead at move max_steps / finished after having been continued, and the games continued per round:
      max_steps 2 (seed 561): 95 / 17 / 7 / 20, 176 252 253 255 248      max_steps 7: 103 / 1 / 15 / 82, 152 224 229 243 250
      max_steps 16: 101 / 0 / 7 / 42, 102 224 251 256 255                 max_steps 16, 65 games, search and backed: 26 / 0 / 1 / 14, 27 56 62 65 63
    The floors of the 257-game cases: 50 capped, 3 capped at move 2, 5 dead at move 7, 20 resumed, 100 continued in every round."""
    n = nt()
    games, K, layers, seed = late.CONTINUE_CASES[case]
    backed = bool(layers)
    rounds, counts = late.continued_rounds(case)
    a = _with_continue(_agent("eight", True, layers, games=games, max_steps=K, seed=seed, backed=backed, **SETTINGS["lambda.5-tc"]), backed)
    a.continue_games, a.backed_targets = True, backed
    _set_start(a, late_start(games, 3))
    assert not a.finished.any().item() and not a.carry_score.any().item() and not a.carry_moves.any().item()
    for r, rd in enumerate(rounds):
        where = (case, "round", r)
        assert np.array_equal(_start_of(a), rd.start) and a.round == r, where
        got = _launched(a, lambda: a.rollout_staged_launch(layers, backed=backed))
        assert_rollout(got, rd.games, where, PER_MOVE)
        if backed:
            played = np.arange(K)[:, None] < rd.games["lengths"][None, :]
            assert np.array_equal(got["backed"][played], bits(rd.games["backed"])[played]) and np.array_equal(got["backed"][~played], got["backed_before"][~played]), where
        assert got["moves"] == int(rd.games["lengths"].sum()) and np.array_equal(_start_of(a), rd.start), where     # every board of `start` is usable, or 0
        rec = read(a, PER_MOVE)
        if r in (0, len(rounds) - 1):
            L, before = rec["lengths"].astype(np.int64), a.stats()
            a.learn()
            acc, ab, st = a.acc.cpu().numpy(), a.acc_abs.cpu().numpy(), a.stats()
            host_acc, host_abs = np.zeros_like(acc), np.zeros_like(ab)
            records = (rec["keys"], rec["values"].view(np.float64), rec["steps"], L, a.tuples, True, 1.0)
            if backed:
                host = n.learn_backed_nt_on_host(*records[:2], a.backed.cpu().numpy(), *records[2:], a.lam, host_acc, host_abs)
            else:
                host = n.learn_tc_nt_on_host(*records, a.lam, host_acc, host_abs)
            last = rec["steps"][L - 1, np.arange(games)]
            print(where, "learn", {k: host[k] for k in ("learnt", "skipped", "clamped")}, "capped", int(rd.capped.sum()), "adds per stage", adds_per_stage(host_acc, late.S))
            assert host["skipped"] == int((last >> 7 == 0).sum()) >= int(rd.cut.sum()) >= 8 and (r or int((rd.capped & (last >> 7 == 0)).sum()) >= 8), where
            assert {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")} == {k: host[k] for k in ("learnt", "skipped", "clamped")}, where
            assert np.array_equal(acc, host_acc) and np.array_equal(ab, host_abs) and host_abs.any(), where
            assert np.array_equal(bits(a.deltas.cpu().numpy())[np.arange(K)[:, None] < L[None, :]], bits(host["deltas"])[np.arange(K)[:, None] < L[None, :]]), where
            a.acc.zero_()
            a.acc_abs.zero_()
        a.continue_pick_launch()
        _assert_state(a, rd.carried, where)
        after = read(a, PER_MOVE)
        assert all(np.array_equal(after[k], rec[k]) for k in rec), where  # the records are only read
        a.round += 1
    assert a.finished_summary(clear=False) == n.finished_summary_on_host(rounds[-1].carried.finished)
    assert a.finished.cpu().tolist()[7] == counts["capped"] and a.finished.cpu().tolist()[6] == counts["resumed"]
    guards_intact(a)


# ------------------------------------------------------------------ 3. the adaptive search at the limit shapes, on late boards
@pytest.mark.parametrize("shape,symmetric", SEARCH_CASES, ids=["-".join((s, IMAGES[y])) for s, y in SEARCH_CASES])
def test_the_adaptive_search_on_late_boards_is_the_mirror(shape, symmetric):
    """pulse_tfe_nt_search_adaptive on the 123 boards of late_boards() under the seeded weights of the shape (one stage), E = 0, 2 and 4
    against the mirror, E = 16 device against device with pulse_tfe_nt_search_deep at two layers; the agent's search(keys, layers=2,
    deep_empty_max=E) gives the same rows, and `depth_stats`, which the board launch is not handed, stays as it was.  On the host first,
    at every shape: at E = 4 33 boards are deep and 90 shallow, the shallow rows are the one-layer search's bit for bit, 31 deep rows
    differ from it in q and 6 to 12 in the action; at E = 2 23 boards are deep, at E = 0 the 3 full ones; the boards have every count of
    empty cells from 0 to 12."""
    import torch
    counts = late.adaptive_premises(shape, symmetric)
    keys = late.late_boards()
    a = search_agent(7, 16, SEED, "seeded", symmetric, tuples=SHAPES[shape])
    a.depth_stats = torch.full((2,), 0x0123, dtype=torch.int64, device=a.device)
    a = guard(a, ("depth_stats",), fill=None)
    a.round = late.SEARCH_ROUND
    assert a.tie_seed == late.seeds(SEED)[2] and a.stage_tiles == ()
    rows = {}
    for E in (0, 2, 4):
        want = late.adaptive_search(shape, symmetric, E)
        q, action, cand = rows[E] = _launch_boards(a, keys, SEARCH, E)
        assert np.array_equal(cand, want["candidates"]) and np.array_equal(action, want["action"]) and np.array_equal(q.view(np.uint64), want["q"].view(np.uint64)), E
        out = a.search(keys, layers=2, deep_empty_max=E)
        assert np.array_equal(out["q"].view(np.uint64), want["q"].view(np.uint64)) and np.array_equal(out["action"], want["action"]), E
        assert np.array_equal(out["candidates"], want["candidates"]), E
    q16, action16, cand16 = _launch_boards(a, keys, SEARCH, 16)
    q2, action2, cand2 = _launch_boards(a, keys, "pulse_tfe_nt_search_deep", 2)
    assert np.array_equal(q16.view(np.uint64), q2.view(np.uint64)) and np.array_equal(action16, action2) and np.array_equal(cand16, cand2)
    deep = late.adaptive_search(shape, symmetric, 4)["deep"]
    assert np.array_equal(rows[4][0][deep].view(np.uint64), q2[deep].view(np.uint64)) and (rows[4][0][~deep] != q2[~deep]).any() and (rows[0][0] != rows[2][0]).any()
    assert a.depth_stats.cpu().tolist() == [0x0123, 0x0123] and counts["deep"] >= late.ADAPTIVE_FLOOR["deep"]
    guards_intact(a)
