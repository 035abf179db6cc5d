"""The 2048 n-tuple network's restarted roll-outs on the device (csrc/tfe_ntuple_restart.hip:
pulse_tfe_nt_rollout_from, pulse_tfe_nt_restart_pick) against the host's statement of them (restart_pick_on_host; tests/tfe_nt_host.py:
the oracle's environment begun on the usable boards of `start`).  Every comparison but the last is exact: integers word for word,
float64 and float32 as bit patterns.  Every buffer a launch is handed sits between guard words, and the rows of keys / values / steps /
backed at and beyond a game's length must keep what they held.

Shapes: one ply 257 games of at most 256 moves (one full workgroup and one of one lane), seed 457; one layer section 13.5's 17 games of
at most 192 moves (two workgroups of eight groups and one group), seed 2312.  The tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), gamma 1.
One layer: the seeded weights of scale 4 at epsilon .25.  One ply: on those every game from a board half-way through another is over
long before move 256, so the weights are the same array divided by 64 (exact) and epsilon is .05: play is led by the rewards, V
breaks their ties, and games are cut.  The `start` of a roll-out case mixes boards the host's pick took from a recorded round,
zeros, a dead board, a board with a 32,768 tile and a crafted live board; every case asserts on the host's games, first, that at least
one game ends and at least one is cut."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guards_intact, read
from tests.tfe_nt_host import nt_games_on_host, usable_on_host
from tests.tfe_nt_support import (BOARD_ID0, BUFFERS, CRAFTED, GAMES, MAX_STEPS, PER_MOVE, SEED, TUPLES, bits, learner_agent, learner_round, nt, plain_learner,
                                  search_agent, weights)
from tests.tfe_search_host import key_of

pytestmark = pytest.mark.gpu

SHAPE = {0: (GAMES, MAX_STEPS, SEED), 1: (17, 192, 2312)}                   # layers: (games, max_steps, seed)
MODES = {"one_ply": (0, False), "search": (1, False), "backed": (1, True)}  # (layers, backed)
EPSILON, DIVISOR, ROUND = {0: .05, 1: .25}, {0: 64, 1: 1}, 0                 # layers: the roll-out cases' epsilon, and what divides the seeded weights
START_PATTERN, BACKED_PATTERN = 0x3C3C3C3C3C3C3C3C, -4321.125              # what `start` and `backed` hold before the first launch
DEAD, CAPPED, LIVE = 1, 4, 5                                               # the games of a mixed `start` that get the three boards made by hand
ROUND_MIN_LENGTH = 128


def _seeds(seed):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    return seed, seed ^ AGENT_KEY, seed ^ TIE_KEY


def _with_restart(a, backed=False):
    """the agent with a `start` and `restart_stats` (and a `backed`) of its own between guard words: `start` and `backed` hold patterns"""
    import torch
    a._restart_state()
    names = ("start", "restart_stats")
    if backed:
        a.backed, names = torch.zeros_like(a.values), names + ("backed",)
    return guard(a, names, start=START_PATTERN, backed=BACKED_PATTERN)


@functools.lru_cache(maxsize=None)
def _weights(layers):
    w = weights("seeded") / np.float32(DIVISOR[layers])
    w.setflags(write=False)
    return w


def _agent(layers, symmetric, backed):
    import torch
    games, max_steps, seed = SHAPE[layers]
    a = _with_restart(search_agent(games, max_steps, seed, "seeded", symmetric, epsilon=EPSILON[layers]), backed)
    a.weights_dev.copy_(torch.from_numpy(_weights(layers).copy()))
    return a


def _start_of(a):
    return a.start.cpu().numpy().view(np.uint64)


def _set_start(a, start):
    import torch
    a.start.copy_(torch.from_numpy(np.ascontiguousarray(start, dtype=np.uint64).view(np.int64).copy()))


# ------------------------------------------------------------------ the pick
def test_the_pick_takes_the_hosts_boards():
    """257 games (two workgroups, one lane in the second) of at most 256 moves at epsilon .25 from zero weights, recorded by the device's
    own pulse_tfe_nt_rollout; min_length = the median length, so that about half the games are too short"""
    n, a = nt(), _with_restart(learner_agent())
    a.rollout()
    got = read(a, PER_MOVE)
    L = got["lengths"].astype(np.int64)
    min_length = int(np.median(L))
    want, picked = n.restart_pick_on_host(got["keys"], L, MAX_STEPS, a.env_seed, a.round_board_id0(), 0.5, min_length)
    print("picked", picked, "of", GAMES, "at min_length", min_length)
    assert 8 <= picked[0] <= GAMES - 8 and int((want == 0).sum()) == GAMES - picked[0]     # some games are picked and some are not
    assert (_start_of(a) == np.uint64(START_PATTERN)).all() and a.restart_stats.cpu().tolist() == [0, 0]
    a.restart_pick_launch(0.5, min_length)
    assert np.array_equal(_start_of(a), want) and a.restart_stats.cpu().tolist() == list(picked)
    assert usable_on_host(want[want != 0]).all()
    later, more = n.restart_pick_on_host(got["keys"], L, MAX_STEPS, a.env_seed, a.round_board_id0(), 0.75, 2)
    assert more[0] > picked[0] and more[1] > picked[1]
    a.restart_pick_launch(0.75, 2)                                          # a second pick writes every entry again and ADDS to picked
    assert np.array_equal(_start_of(a), later) and a.restart_stats.cpu().tolist() == [picked[0] + more[0], picked[1] + more[1]]
    assert a.restart_summary() == dict(picked=picked[0] + more[0], mean_depth=(picked[1] + more[1]) / (picked[0] + more[0]), started=more[0])
    assert a.restart_stats.cpu().tolist() == [0, 0]
    after = read(a, PER_MOVE)
    assert all(np.array_equal(after[k], got[k]) for k in got)              # the records are only read
    guards_intact(a)


# ------------------------------------------------------------------ the games from given boards, word for word
@functools.lru_cache(maxsize=None)
def _mixed_start(layers):
    """boards the host's pick takes from a host round of the shape (zero weights, one ply), every third of them zeroed, and three made by
    hand: a dead board, a board with a 32,768 tile and a live one"""
    games, max_steps, seed = SHAPE[layers]
    rec = nt_games_on_host(games, max_steps, .25, 1.0, weights("zero"), TUPLES, True, *_seeds(seed), BOARD_ID0, ROUND)
    start, picked = nt().restart_pick_on_host(rec["keys"], rec["lengths"], max_steps, seed, BOARD_ID0, 0.5, 2)
    assert picked[0] == games
    start[::3] = 0
    start[DEAD], start[CAPPED], start[LIVE] = key_of(CRAFTED["dead"]), key_of(CRAFTED["tile_32768"]), key_of(CRAFTED["one_merge"])
    start.setflags(write=False)
    return start


@functools.lru_cache(maxsize=None)
def _host_games(layers, symmetric):
    """the host's games from the mixed start, with the backed values at one layer (recording them does not change play:
    tests/test_tfe_nt_backed_cpu.py), and the `start` the launch is to leave"""
    games, max_steps, seed = SHAPE[layers]
    start = _mixed_start(layers)
    want = nt_games_on_host(games, max_steps, EPSILON[layers], 1.0, _weights(layers), TUPLES, symmetric, *_seeds(seed), BOARD_ID0, ROUND,
                            depth=layers, backed=bool(layers), start=start)
    left = want["start_left"]
    assert want["ended"] >= 1 and want["truncated"] >= 1 and want["ended"] + want["truncated"] == games, (layers, symmetric, want["ended"])
    kept = left != 0
    assert not kept[[DEAD, CAPPED]].any() and kept[LIVE] and not kept[::3].any() and int(kept.sum()) == games - len(start[::3]) - 2
    assert np.array_equal(left[kept], start[kept])
    return want, left


def _read(a):
    out = read(a, PER_MOVE)
    return dict(out, backed=bits(a.backed.cpu().numpy())) if a.backed is not None else out


def _launched(a, launch):
    """`launch` on the agent; the read-back carries what the per-move rows held before it and the counters' differences"""
    before, st = _read(a), a.stats()
    launch()
    after = a.stats()
    return dict(_read(a), **{k + "_before": v for k, v in before.items() if k in PER_MOVE + ("backed",)}, **{k: after[k] - st[k] for k in ("moves", "truncated")})


def _assert_games(a, got, want, left, where, backed):
    assert_rollout(got, want, where, PER_MOVE)
    played = np.arange(got["keys"].shape[0])[:, None] < want["lengths"][None, :]
    assert (~played).any() and (got["keys_before"] == np.uint64(PATTERNS["keys"])).all(), where        # so the rows beyond a game keep the pattern
    if backed:
        assert np.array_equal(got["backed"][played], bits(want["backed"])[played]), where
        assert np.array_equal(got["backed"][~played], got["backed_before"][~played]), where
        assert (got["backed_before"] == bits(np.float64(BACKED_PATTERN))).all(), where
    assert got["moves"] == int(want["lengths"].sum()) and got["truncated"] == want["truncated"], where
    assert np.array_equal(_start_of(a), left), where
    guards_intact(a)


@pytest.mark.parametrize("symmetric", [True, False], ids=["symmetric", "one_image"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_games_from_given_boards_are_the_hosts(mode, symmetric):
    layers, backed = MODES[mode]
    want, left = _host_games(layers, symmetric)
    a = _agent(layers, symmetric, backed)
    _set_start(a, _mixed_start(layers))
    got = _launched(a, lambda: a.rollout_from_launch(layers, backed=backed))
    _assert_games(a, got, want, left, (mode, symmetric), backed)
    first = want["keys"][0]
    plain = _plain_first_keys(layers, symmetric)
    assert (first[left != 0] != plain[left != 0]).any() and np.array_equal(first[left == 0], plain[left == 0])     # who began where


@functools.lru_cache(maxsize=None)
def _plain_first_keys(layers, symmetric):
    """the first afterstates of the same launch from reset: one move of every game on the host"""
    games, _, seed = SHAPE[layers]
    want = nt_games_on_host(games, 1, EPSILON[layers], 1.0, _weights(layers), TUPLES, symmetric, *_seeds(seed), BOARD_ID0, ROUND, depth=layers,
                            start=np.zeros(games, dtype=np.uint64))
    return want["keys"][0]


@pytest.mark.parametrize("mode", list(MODES))
def test_with_a_start_of_zeros_the_launch_is_its_sibling(mode):
    """pulse_tfe_nt_rollout, pulse_tfe_nt_rollout_search and pulse_tfe_nt_rollout_backed on the same struct: every output, byte for byte"""
    import torch
    (layers, backed), max_steps = MODES[mode], SHAPE[MODES[mode][0]][1]
    a, b = _agent(layers, True, backed), _agent(layers, True, backed)
    a.start.zero_()
    a.rollout_from_launch(layers, backed=backed)
    if backed:
        b.rollout_backed_launch(1)
    elif layers:
        b.rollout_search_launch(1)
    else:
        b._launch("pulse_tfe_nt_rollout", b._rollout_struct())
    for k in ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters") + (("backed",) if backed else ()):
        assert torch.equal(getattr(a, k).view(torch.uint8), getattr(b, k).view(torch.uint8)), k
    assert not a.start.any().item() and (_start_of(b) == np.uint64(START_PATTERN)).all()
    assert int(a.lengths.min().item()) < max_steps == int(a.lengths.max().item()) and a.stats()["moves"] == int(a.lengths.sum().item()) > 0
    guards_intact(a, b)


# ------------------------------------------------------------------ rounds
def _restarted_round(a, left, coherence, where):
    """learner_round with the games held to the host's from `left`, the `start` the pick of the round before left (None: no pick yet),
    and, after the apply, the pick launch held to the host's.  Returns (the record, the next round's start)."""
    n, out = nt(), {}

    def games(a, h):
        given = np.zeros(a.n_games, dtype=np.uint64) if left is None else left
        want = nt_games_on_host(a.n_games, a.max_steps, a.epsilon, a.gamma, h.policy, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                                a.round_board_id0(), a.round, start=given)
        kept = want["start_left"]
        assert_rollout(h.got, want, where, PER_MOVE)
        assert np.array_equal(_start_of(a), kept) and np.array_equal(kept, given), where      # picked boards are usable: none is zeroed
        return dict(restarted=int(np.count_nonzero(kept)))

    def pick(a, h):
        a.restart_pick_launch()
        want, picked = n.restart_pick_on_host(h.got["keys"], h.L, a.max_steps, a.env_seed, a.round_board_id0(), a.restart_fraction, a.restart_min_length)
        assert np.array_equal(_start_of(a), want), where
        out["start"] = want
        return dict(picked=picked[0], depth=picked[1])
    rec = learner_round(a, after_learn=games, after_apply=pick, coherence=coherence)
    return rec, out["start"]


def _assert_twins(a, b, more=()):
    """two agents after the same rounds: the weights, the per-game arrays, the counters and `start` whole, the per-move rows up to each
    game's length (beyond it one holds its patterns and the other zeros)"""
    import torch
    for k in ("weights_dev", "lengths", "total_score", "episode_reward", "counters", "start"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    played = np.arange(a.max_steps)[:, None] < a.lengths.cpu().numpy()[None, :]
    for k in PER_MOVE + tuple(more):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint64 if x.itemsize == 8 else x.dtype)[played], y.view(np.uint64 if y.itemsize == 8 else y.dtype)[played]), k


@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=0.5, tc=True)], ids=["lambda0", "lambda.5-tc"])
def test_three_restarted_rounds_are_the_hosts(kw):
    """acc over all W, the counters and the weights as float32 bit patterns per round (learner_round), the games from the boards the
    round before picked and the pick itself; then learn_batch() three times on a twin agent leaves the same weights, records and start.
    Rehearsed on the host: 241 / 235 / 226 games end and 16 / 22 / 31 are cut, 187 / 138 / 159 are picked at lambda 0; with lambda .5 and tc
    241 / 245 / 229 end, 16 / 12 / 28 are cut, 187 / 120 / 163 are picked."""
    import torch
    a = _with_restart(learner_agent(extra_buffers=("deltas", "acc_abs", "E", "A", "tc_stats"), **kw))
    a.start.zero_()                                                         # (its own start, guarded: a first round from zeros is a round from reset)
    b = plain_learner(**kw)
    for agent in (a, b):
        agent.restart_fraction, agent.restart_min_length = 0.5, ROUND_MIN_LENGTH
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if a.tc else None
    left, recs = None, []
    for r in range(3):
        rec, left = _restarted_round(a, left, coherence, ("round", r))
        recs.append(rec)
        guards_intact(a)
    print([{k: rec[k] for k in ("ended", "cut", "moves", "restarted", "picked", "depth", "host", "stats")} for rec in recs])
    for rec in recs:
        assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"] and rec["stats"] == {k: rec["host"][k] for k in rec["stats"]}, rec
        assert rec["ended"] >= 1 and rec["cut"] >= 1 and 8 <= rec["picked"] <= GAMES - 8, rec
    assert recs[0]["restarted"] == 0 and [rec["restarted"] for rec in recs[1:]] == [rec["picked"] for rec in recs[:2]]
    if a.tc:
        E, A = a.coherence()
        assert np.array_equal(bits(E), bits(coherence[0])) and np.array_equal(bits(A), bits(coherence[1]))
    assert b.start is None
    for _ in range(3):
        b.learn_batch()
    assert a.round == b.round == 3 and b.restart_summary()["picked"] == sum(rec["picked"] for rec in recs)
    _assert_twins(a, b)


def test_three_restarted_rounds_under_search_with_backed_targets_are_the_hosts():
    """rollout_layers = 1, backed_targets, lambda .5: 17 games of at most 192 moves at epsilon .25, the first round from the seeded
    weights.  Per round the games and backed values from the boards the round before picked, acc, the counters, the weights as
    bit patterns and the pick; then learn_batch() three times on a twin agent."""
    import torch
    n, (games, max_steps, seed) = nt(), SHAPE[1]
    make = lambda: plain_learner(games, max_steps=max_steps, seed=seed, lam=0.5)
    a, b = make(), make()
    a = guard(a, BUFFERS + ("deltas",), **PATTERNS)
    a = _with_restart(a, backed=True)
    a.start.zero_()
    for agent in (a, b):
        agent.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
        agent.rollout_layers, agent.backed_targets, agent.restart_fraction, agent.restart_min_length = 1, True, 0.5, 32
    left, counts = np.zeros(games, dtype=np.uint64), []
    for r in range(3):
        policy = a.weights()
        got = _launched(a, a.rollout)
        want = nt_games_on_host(games, max_steps, a.epsilon, a.gamma, policy, a.tuples, a.symmetric, a.env_seed, a.agent_seed, a.tie_seed,
                                a.round_board_id0(), a.round, depth=1, backed=True, start=left)
        kept = want["start_left"]
        assert_rollout(got, want, ("round", r), PER_MOVE)
        L = got["lengths"].astype(np.int64)
        played = np.arange(max_steps)[:, None] < L[None, :]
        assert np.array_equal(got["backed"][played], bits(want["backed"])[played]) and np.array_equal(got["backed"][~played], got["backed_before"][~played])
        assert np.array_equal(_start_of(a), kept) and np.array_equal(kept, left)
        before = a.stats()
        a.learn()
        st, acc = a.stats(), a.acc.cpu().numpy()
        host_acc = np.zeros_like(acc)
        host = n.learn_backed_nt_on_host(got["keys"], got["values"].view(np.float64), got["backed"].view(np.float64), got["steps"], L, a.tuples, a.symmetric,
                                         a.gamma, a.lam, host_acc)
        assert np.array_equal(acc, host_acc) and {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")} == {
            k: host[k] for k in ("learnt", "skipped", "clamped")}
        assert host["skipped"] == want["truncated"] and host["learnt"] + host["skipped"] == int(L.sum()) == got["moves"]
        a.apply()
        host_w = policy.copy()
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0
        assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)) and not a.acc.any().item()
        a.restart_pick_launch()
        left, picked = n.restart_pick_on_host(got["keys"], L, max_steps, a.env_seed, a.round_board_id0(), 0.5, 32)
        assert np.array_equal(_start_of(a), left)
        counts.append((want["ended"], want["truncated"], picked))
        guards_intact(a)
        a.round += 1
    print("games ended / cut / (picked, depths) per round:", counts)
    assert all(ended >= 1 and picked[0] >= 1 for ended, _, picked in counts), counts
    for _ in range(3):
        b.learn_batch()
    _assert_twins(a, b, ("backed", "deltas"))


def test_without_the_attribute_three_rounds_are_todays():
    import torch
    from pulselib_amd import _native
    a, b = plain_learner(33), plain_learner(33)
    assert a.restart_fraction == 0.0 and a.start is None
    for _ in range(3):
        a.learn_batch()
        b._launch("pulse_tfe_nt_rollout", b._rollout_struct())._launch("pulse_tfe_nt_learn", b._moves(_native.TfeNtLearn())).apply()
        b.round += 1
    for k in ("weights_dev", "keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.round == 3 and a.weights().any() and a.start is None and a.restart_stats is None
    with pytest.raises(ValueError, match="holds no start"):
        a.restart_summary()


# ------------------------------------------------------------------ the score
def test_it_learns():
    """The default network, 4,096 games per round, max_steps 4,096, epsilon 0, seed 0, restart_fraction .5 (restart_min_length 64), two
    rounds from zero weights: the second round's games begin half-way through the first's.  Then 1,024 one-ply evaluation games from
    the default evaluation boards (from reset) on it and on zero weights, paired by board.  Asserted (the sibling tests' margin): the
    restarted agent beats zero weights by at least three standard errors of the paired difference.  The comparison with the
    unrestarted agent is DESIGN.md section 13.7's measurement, not a test.  On an MI355X (one run): zero weights 2,025.6 +- 29.0, restarted
    6,643.3 +- 93.6: +4,617.7 +- 98.3 (47 standard errors); round 2 restarted 4,090 of its 4,096 games from a mean depth of 88.9; nothing
    clamped.  Rehearsed on the host at 256 games per round: 5,044.1 +- 77.1, +3,018.6 +- 82.7 (36.5 standard errors)."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    dev = torch.device("cuda:0")
    a = NTupleTDAfterstateTFEGPU(dev, 4096, max_steps=4096, seed=0)
    a.restart_fraction = 0.5
    a.learn_batch()
    first = a.restart_summary()
    a.learn_batch()
    st = a.stats()
    assert a.round == 2 and st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not a.acc.any().item()
    assert first["picked"] == first["started"] > 0 and a.start is not None
    ev = a.evaluate(n_games=1024, per_game=True)
    zero = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=4096, seed=0).evaluate(n_games=1024, per_game=True)
    d = (ev["total_score"] - zero["total_score"]).astype(np.float64)
    gain, gain_se = d.mean(), d.std(ddof=1) / np.sqrt(d.size)
    se = lambda e: e["std_score"] / e["games"] ** .5
    print("1,024 one-ply games after two rounds of 4,096 with restart .5: zero weights", zero["mean_score"], "+-", se(zero), "restarted", ev["mean_score"], "+-",
          se(ev), "restarted minus zero", gain, "+-", gain_se, "round 2 restarted", first["picked"], "games from mean depth", first["mean_depth"], "moves", st["moves"],
          "clamped", st["clamped"])
    assert ev["games"] == zero["games"] == 1024
    assert gain >= 3.0 * gain_se, (ev["mean_score"], zero["mean_score"], gain_se)
