"""The 2048 n-tuple network's search-backed TD targets on the device (csrc/tfe_ntuple_backed.hip:
pulse_tfe_nt_rollout_backed, pulse_tfe_nt_learn_backed) against the host's statement of them (tests/tfe_nt_host.py: the oracle's
environment under search_nt_on_host, recording its `backed`; backed_deltas_on_host, learn_backed_nt_on_host).  Every comparison is
exact: integers word for word, float64 and float32 as bit patterns.  Every buffer a launch is handed sits between guard words, and the
rows of keys / values / steps / backed / deltas at and beyond a game's length must keep what they held.

Shapes: section 13.5's, the smallest that fill two workgroups unevenly.  One layer: 17 games of at most 192 moves = two workgroups of
eight groups and one group, seed 2312.  Two layers: 7 games of at most 160 moves, one workgroup each, seed 5.  The tuples (0, 1, 2, 3)
and (4, 5, 6, 8, 9, 10), weights zero or a seeded normal array of scale 4, gamma 1.  Every case asserts on the host's games, first,
that at least one game ends and at least one is cut.  The learner: two rounds of 33 games (four workgroups of groups and one group;
one wavefront of the walk with 31 lanes beyond the batch) of at most 256 moves at epsilon .25, the first on zero weights, the second
on the weights it left."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guards_intact, read
from tests.tfe_nt_support import BOARD_ID0, BUFFERS, PER_MOVE, TUPLES, bits, nt, plain_learner, search_agent, weights

pytestmark = pytest.mark.gpu

SHAPE = {1: (17, 192, 2312), 2: (7, 160, 5)}                               # layers: (games, max_steps, seed)
EPSILON, ROUND = .25, 0
ONE_LAYER = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("zero", 0.0, True), ("zero", EPSILON, True), ("seeded", EPSILON, False))
TWO_LAYERS = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("seeded", EPSILON, False))
ROUND_GAMES = 33
BACKED_PATTERN, DELTAS_PATTERN = -4321.125, 777.0625                       # what `backed` and `deltas` hold before the first launch
TC_BUFFERS = ("acc_abs", "E", "A", "tc_stats")


def _with_backed(a, deltas=False):
    """the agent with a `backed` (and `deltas`) of its own between guard words, holding the pattern"""
    import torch
    names = ("backed", "deltas") if deltas else ("backed",)
    for name in names:
        setattr(a, name, torch.zeros_like(a.values))
    return guard(a, names, backed=BACKED_PATTERN, deltas=DELTAS_PATTERN)


def _agent(layers, name, epsilon, symmetric=True, **kw):
    games, max_steps, seed = SHAPE[layers]
    return _with_backed(search_agent(games, max_steps, seed, name, symmetric, epsilon=epsilon, **kw))


@functools.lru_cache(maxsize=None)
def _host_games(layers, name, epsilon, symmetric=True):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_host import nt_games_on_host
    games, max_steps, seed = SHAPE[layers]
    want = nt_games_on_host(games, max_steps, epsilon, 1.0, weights(name), TUPLES, symmetric, seed, seed ^ AGENT_KEY, seed ^ TIE_KEY, BOARD_ID0, ROUND,
                            depth=layers, backed=True)
    assert want["ended"] >= 1 and want["truncated"] >= 1 and want["ended"] + want["truncated"] == games, (layers, name, epsilon, want["ended"])
    return want


def _read(a):
    return dict(read(a, PER_MOVE), backed=bits(a.backed.cpu().numpy()))


def _launched(a, launch):
    """`launch` on the agent; the read-back carries what the per-move rows held before it and the counters' differences"""
    before, st = _read(a), a.stats()
    launch()
    after = a.stats()
    return dict(_read(a), **{k + "_before": before[k] for k in PER_MOVE + ("backed",)}, **{k: after[k] - st[k] for k in ("moves", "truncated")})


def _assert_games(a, got, want, where):
    assert_rollout(got, want, where, PER_MOVE)
    played = np.arange(got["backed"].shape[0])[:, None] < want["lengths"][None, :]
    assert np.array_equal(got["backed"][played], bits(want["backed"])[played]), where
    assert np.array_equal(got["backed"][~played], got["backed_before"][~played]) and (~played).any(), where
    assert (got["backed_before"] == bits(np.float64(BACKED_PATTERN))).all(), where          # so those rows keep the pattern
    assert got["moves"] == int(want["lengths"].sum()) and got["truncated"] == want["truncated"], where
    guards_intact(a)


# ------------------------------------------------------------------ the games and the backed values, word for word
@pytest.mark.parametrize("name,epsilon,symmetric", ONE_LAYER)
def test_one_layer_records_the_hosts_games(name, epsilon, symmetric):
    want, a = _host_games(1, name, epsilon, symmetric), _agent(1, name, epsilon, symmetric)
    got = _launched(a, lambda: a.rollout_backed_launch(1))
    _assert_games(a, got, want, (name, epsilon, symmetric))
    assert np.isfinite(want["backed"]).all() and want["backed"].any()


@pytest.mark.parametrize("name,epsilon,symmetric", TWO_LAYERS)
def test_two_layers_record_the_hosts_games(name, epsilon, symmetric):
    want, a = _host_games(2, name, epsilon, symmetric), _agent(2, name, epsilon, symmetric)
    got = _launched(a, lambda: a.rollout_backed_launch(2))
    _assert_games(a, got, want, (name, epsilon, symmetric))


@pytest.mark.parametrize("layers", [1, 2])
def test_recording_one_more_word_does_not_change_play(layers):
    """the new launch against pulse_tfe_nt_rollout_search on the same struct: keys, values, steps and the per-game arrays"""
    a, b = _agent(layers, "seeded", EPSILON), _agent(layers, "seeded", EPSILON)
    got, plain = _launched(a, lambda: a.rollout_backed_launch(layers)), _launched(b, lambda: b.rollout_search_launch(layers))
    for k in PER_MOVE + ("lengths", "total_score", "episode_reward", "moves", "truncated"):
        assert np.array_equal(got[k], plain[k]), k
    assert np.array_equal(plain["backed"], plain["backed_before"]) and not np.array_equal(got["backed"], got["backed_before"])
    assert int(got["lengths"].min()) < SHAPE[layers][1] == int(got["lengths"].max())
    guards_intact(a, b)


# ------------------------------------------------------------------ the learner on the device's own records
def _learner(**kw):
    a = plain_learner(ROUND_GAMES, **kw)
    a = guard(a, BUFFERS + tuple(k for k in TC_BUFFERS if getattr(a, k) is not None), **PATTERNS)
    a.deltas = None
    a = _with_backed(a, deltas=True)
    a.rollout_layers, a.backed_targets = 1, True
    return a


def _round(a, coherence):
    """One round on the device -- the backed roll-out, learn(), apply() -- with the walk, the adds and the apply held to the host's on
    the device's own records.  Returns (games ended, games cut)."""
    n, policy = nt(), a.weights()
    deltas_before = bits(a.deltas.cpu().numpy())
    got = _launched(a, a.rollout)
    L = got["lengths"].astype(np.int64)
    played = np.arange(a.max_steps)[:, None] < L[None, :]
    last = got["steps"][L - 1, np.arange(a.n_games)]
    ended, cut = int((last >> 7 != 0).sum()), int((last >> 7 == 0).sum())
    before = a.stats()
    a.learn()
    st = a.stats()
    values, backed = got["values"].view(np.float64), got["backed"].view(np.float64)
    acc = a.acc.cpu().numpy()
    host_acc, host_abs = np.zeros_like(acc), np.zeros(a.n_weights, dtype=np.int64) if a.tc else None
    host = n.learn_backed_nt_on_host(got["keys"], values, backed, got["steps"], L, a.tuples, a.symmetric, a.gamma, a.lam, host_acc, host_abs)
    deltas = bits(a.deltas.cpu().numpy())
    assert np.array_equal(deltas[played], bits(host["deltas"])[played]) and np.array_equal(deltas[~played], deltas_before[~played])
    assert np.array_equal(acc, host_acc) and int(acc[:, 1].sum()) == a.n_features * host["learnt"]
    if a.tc:
        assert np.array_equal(a.acc_abs.cpu().numpy(), host_abs) and host_abs.any()
    assert {k: st[k] - before[k] for k in ("learnt", "skipped", "clamped")} == {k: host[k] for k in ("learnt", "skipped", "clamped")}
    assert host["skipped"] == cut and host["learnt"] + host["skipped"] == int(L.sum()) == got["moves"]
    a.apply()
    host_w = policy.copy()
    if a.tc:
        n.apply_tc_nt_on_host(host_w, host_acc, host_abs, *coherence, a.alpha / a.n_features)
        E, A = a.coherence()
        assert np.array_equal(bits(E), bits(coherence[0])) and np.array_equal(bits(A), bits(coherence[1]))
    else:
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0
    assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)) and not np.array_equal(host_w.view(np.uint32), policy.view(np.uint32))
    assert not a.acc.any().item() and not (a.tc and a.acc_abs.any().item())
    guards_intact(a)
    a.round += 1
    return ended, cut


@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=0.5), dict(lam=0.5, tc=True)], ids=["lambda0", "lambda.5", "tc"])
@pytest.mark.parametrize("start", ["zero", "seeded"])
def test_the_learner_learns_as_the_host_does(start, kw):
    """deltas, acc, acc_abs, the counters and the weights after the apply.  From zero weights two rounds, the second on the weights the
    first left (rehearsed on the host: 3 games end and 30 are cut, then 8 and 25); from the seeded weights section 13.5's round, of
    which 32 games end and 1 is cut."""
    import torch
    a = _learner(**kw)
    if start == "seeded":
        a.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
    assert (bits(a.deltas.cpu().numpy()) == bits(np.float64(DELTAS_PATTERN))).all()
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if a.tc else None
    counts = [_round(a, coherence) for _ in range(2 if start == "zero" else 1)]
    print("games ended / cut per round:", counts)
    assert all(ended >= 1 and cut >= 1 and ended + cut == ROUND_GAMES for ended, cut in counts), counts
    assert start == "zero" or counts == [(32, 1)], counts
    assert a.round == len(counts) and a.weights().any()


# ------------------------------------------------------------------ the agent
def test_the_attribute_takes_the_backed_launches():
    """backed_targets = True through learn_batch() against the direct launches; `backed` and `deltas` are allocated on first use"""
    import torch
    agents = [plain_learner(ROUND_GAMES, lam=0.0), plain_learner(ROUND_GAMES, lam=0.0)]
    for a in agents:
        a.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
        assert a.backed is None and a.deltas is None
    a, b = agents
    a.rollout_layers, a.backed_targets = 1, True
    a.learn_batch()
    b.rollout_backed_launch(1).learn_backed_launch(0.0).apply()
    assert a.round == 1 and b.round == 0 and a.backed.dtype == torch.float64 and a.backed.shape == a.values.shape == a.deltas.shape
    for k in ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters", "weights_dev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    T = int(a.lengths.max().item())
    played = np.arange(T)[:, None] < a.lengths.cpu().numpy()[None, :]
    assert a.trajectory_backed().shape == (T, ROUND_GAMES) and a.trajectory_deltas().shape == (T, ROUND_GAMES)
    assert np.array_equal(bits(a.trajectory_backed())[played], bits(b.trajectory_backed())[played])
    assert np.array_equal(bits(a.trajectory_deltas())[played], bits(b.trajectory_deltas())[played])
    assert not torch.equal(a.weights_dev, torch.from_numpy(weights("seeded").copy()).to(a.device)) and not a.acc.any().item()
    with pytest.raises(ValueError, match="backed_targets needs rollout_layers"):
        a.rollout(layers=0)


def test_without_the_attribute_a_round_under_search_is_todays():
    import torch
    agents = [plain_learner(ROUND_GAMES, lam=0.5), plain_learner(ROUND_GAMES, lam=0.5)]
    for a in agents:
        a.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
    a, b = agents
    a.rollout_layers = 1
    assert a.backed_targets is False
    a.learn_batch()
    b._launch("pulse_tfe_nt_rollout_search", b._rollout_struct(), 1).learn_lambda_launch(0.5).apply()
    for k in ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "counters", "weights_dev", "deltas"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.backed is None and b.backed is None and a.weights().any()
    with pytest.raises(ValueError, match="holds no backed"):
        a.trajectory_backed()
    with pytest.raises(ValueError, match="holds no backed"):
        a.learn_backed_launch(0.0)


# ------------------------------------------------------------------ the score
def test_it_learns():
    """The default network, 4,096 games per round, max_steps 4,096, epsilon 0, seed 0, rollout_layers = 1, backed_targets = True, two
    rounds.  Then 1,024 one-ply evaluation games from the default evaluation boards on it and on zero weights, paired by board.
    Asserted (section 13.5's assertion): the backed agent beats zero weights by at least three standard errors of the paired difference.
    Printed, not asserted: the same for an agent under rollout_layers = 1 alone.  On an MI355X (one run): zero weights 2,025.6 +- 29.0,
    backed targets 4,254.7 +- 61.6, the records' targets 2,821.3 +- 41.7: +2,229.1 +- 67.1 over zero weights (33 standard errors; the
    records' targets cleared the assertion at 16) and +1,433.4 +- 72.4 over the records' targets; nothing clamped.  DESIGN.md section
    13.6 has twelve rounds."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    dev = torch.device("cuda:0")
    agents = {}
    for backed in (True, False):
        a = NTupleTDAfterstateTFEGPU(dev, 4096, max_steps=4096, seed=0)
        a.rollout_layers, a.backed_targets = 1, backed
        for _ in range(2):
            a.learn_batch()
        agents[backed] = a
    st = agents[True].stats()
    assert agents[True].round == 2 and st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not agents[True].acc.any().item()
    ev = {backed: a.evaluate(n_games=1024, per_game=True) for backed, a in agents.items()}
    zero = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=4096, seed=0).evaluate(n_games=1024, per_game=True)

    def paired(x, y):
        d = (x["total_score"] - y["total_score"]).astype(np.float64)
        return d.mean(), d.std(ddof=1) / np.sqrt(d.size)
    se = lambda e: e["std_score"] / e["games"] ** .5
    gain, gain_se = paired(ev[True], zero)
    diff, diff_se = paired(ev[True], ev[False])
    print("1,024 one-ply games after two rounds of 4,096 under one-layer search: zero weights", zero["mean_score"], "+-", se(zero), "backed targets",
          ev[True]["mean_score"], "+-", se(ev[True]), "the records' targets", ev[False]["mean_score"], "+-", se(ev[False]), "backed minus zero", gain, "+-",
          gain_se, "backed minus the records' targets", diff, "+-", diff_se, "clamped", st["clamped"])
    assert ev[True]["games"] == zero["games"] == 1024
    assert gain >= 3.0 * gain_se, (ev[True]["mean_score"], zero["mean_score"], gain_se)
