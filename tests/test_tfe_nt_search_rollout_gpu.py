"""The 2048 n-tuple network's training roll-out under expectimax search on the device (DESIGN.md section 13.5;
csrc/tfe_ntuple_search_rollout.hip: pulse_tfe_nt_rollout_search) against the host's statement of it (tests/tfe_nt_host.py:
the oracle's environment under search_nt_on_host, recording value_on_host of the chosen afterstates).  Every comparison is exact:
integers word for word, float64 as bit patterns.  Every buffer a launch is handed sits between guard words, and the rows of keys /
values / steps at and beyond a game's length must keep what they held.

Shapes: those of the evaluations under the same policies.  One layer (tests/test_tfe_nt_search_gpu.py): 17 games of at most 192 moves
= two workgroups of eight groups and one group, seed 2312.  Two layers (tests/test_tfe_nt_search2_gpu.py): 7 games of at most 160
moves, one workgroup each, seed 5.  The tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), weights zero or a seeded normal array of scale 4,
gamma 1.  Those files chose the seeds on the host: every case but zero weights at epsilon 0 holds at least two games that end, no two
equally long, and at least two that are cut; test_the_hosts_games_end_and_are_cut asserts it on the games compared here.  A whole round
under search: 33 games = four full workgroups of groups and one group, at most 256 moves, the seeded weights, epsilon .25."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import assert_rollout, guards_intact, read
from tests.tfe_nt_support import BOARD_ID0, PER_MOVE, TUPLES, learner_round, plain_learner, search_agent, weights

pytestmark = pytest.mark.gpu

SHAPE = {1: (17, 192, 2312), 2: (7, 160, 5)}                               # layers: (games, max_steps, seed)
EPSILON, ROUND = .25, 0
ONE_LAYER = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("zero", 0.0, True), ("zero", EPSILON, True), ("seeded", EPSILON, False))
TWO_LAYERS = (("seeded", 0.0, True), ("seeded", EPSILON, True), ("seeded", EPSILON, False))
ROUND_GAMES = 33


def _agent(layers, name, epsilon, symmetric=True, **kw):
    games, max_steps, seed = SHAPE[layers]
    return search_agent(games, max_steps, seed, name, symmetric, epsilon=epsilon, **kw)


@functools.lru_cache(maxsize=None)
def _host_games(layers, name, epsilon, symmetric=True, gamma=1.0):
    from pulselib_amd.agents.tfe_common import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_host import nt_games_on_host
    games, max_steps, seed = SHAPE[layers or 1]
    args = (games, max_steps, epsilon, gamma, weights(name), TUPLES, symmetric, seed, seed ^ AGENT_KEY, seed ^ TIE_KEY, BOARD_ID0, ROUND)
    return nt_games_on_host(*args, depth=layers)


def _launched(a, launch):
    """`launch` on the agent; the read-back carries what the per-move rows held before it and the counters' differences"""
    before, st = read(a, PER_MOVE), a.stats()
    launch()
    after = a.stats()
    return dict(read(a, PER_MOVE), **{k + "_before": before[k] for k in PER_MOVE}, **{k: after[k] - st[k] for k in ("moves", "truncated")})


def _assert_games(a, got, want, where):
    assert_rollout(got, want, where, PER_MOVE)
    assert got["moves"] == int(want["lengths"].sum()) and got["truncated"] == want["truncated"], where
    guards_intact(a)


# ------------------------------------------------------------------ the games, word for word
def test_the_hosts_games_end_and_are_cut():
    """no GPU work: what the games below exercise (module docstring)"""
    for layers, cases in ((1, ONE_LAYER), (2, TWO_LAYERS)):
        for name, epsilon, symmetric in cases:
            want = _host_games(layers, name, epsilon, symmetric)
            L = want["lengths"]
            ended = L[L < SHAPE[layers][1]]
            assert want["truncated"] >= 2 and want["capped"] == 0 and want["ended"] + want["truncated"] == SHAPE[layers][0], (layers, name, epsilon)
            assert len(set(ended.tolist())) == len(ended), (layers, name, epsilon, sorted(L.tolist()))
            if (name, epsilon) != ("zero", 0.0):
                assert want["ended"] >= 2 and want["ended"] == len(ended), (layers, name, epsilon, want["ended"])
            played = np.arange(L.max())[:, None] < L[None, :]
            assert (name == "zero") != bool(want["values"][:L.max()][played].any())


@pytest.mark.parametrize("name,epsilon,symmetric", ONE_LAYER)
def test_one_layer_records_the_hosts_games(name, epsilon, symmetric):
    a, want = _agent(1, name, epsilon, symmetric), _host_games(1, name, epsilon, symmetric)
    got = _launched(a, lambda: a.rollout_search_launch(1))
    _assert_games(a, got, want, (name, epsilon, symmetric))


@pytest.mark.parametrize("name,epsilon,symmetric", TWO_LAYERS)
def test_two_layers_record_the_hosts_games(name, epsilon, symmetric):
    a, want = _agent(2, name, epsilon, symmetric), _host_games(2, name, epsilon, symmetric)
    got = _launched(a, lambda: a.rollout_search_launch(2))
    _assert_games(a, got, want, (name, epsilon, symmetric))


# ------------------------------------------------------------------ the attribute and the default
def test_the_attribute_takes_the_search_launch():
    a, b, want = _agent(1, "seeded", EPSILON), _agent(1, "seeded", EPSILON), _host_games(1, "seeded", EPSILON)
    assert a.rollout_layers == 0
    a.rollout_layers = 1
    got, direct = _launched(a, a.rollout), _launched(b, lambda: b.rollout_search_launch(1))
    for k in got:
        assert np.array_equal(got[k], direct[k]), k
    _assert_games(a, got, want, "attribute")
    again = _launched(b, lambda: b.rollout(layers=1))                       # ... and so does the argument, over the attribute's 0
    assert b.rollout_layers == 0 and all(np.array_equal(again[k], direct[k]) for k in PER_MOVE + ("lengths", "total_score", "episode_reward"))
    guards_intact(b)


def test_the_default_is_the_one_ply_rollout():
    a, want = _agent(1, "seeded", EPSILON), _host_games(0, "seeded", EPSILON)
    got = _launched(a, a.rollout)
    _assert_games(a, got, want, "default")
    search = _host_games(1, "seeded", EPSILON)
    assert not np.array_equal(want["lengths"], search["lengths"])           # (the two policies do play different games here)
    b = _agent(1, "seeded", EPSILON)
    b.rollout_layers = 2
    _assert_games(b, _launched(b, lambda: b.rollout(layers=0)), want, "layers=0 over the attribute")


def test_gamma_zero_is_the_one_ply_rollouts_records():
    a, want = _agent(1, "seeded", EPSILON, gamma=0.0), _host_games(0, "seeded", EPSILON, True, 0.0)
    got = _launched(a, lambda: a.rollout_search_launch(1))
    _assert_games(a, got, want, "gamma 0")
    assert want["values"].any() and want["ended"] >= 1


# ------------------------------------------------------------------ a whole round under search
@pytest.mark.parametrize("kw", [dict(lam=0.0), dict(lam=0.5), dict(tc=True)], ids=["td0", "lambda", "tc"])
def test_a_round_under_search_learns_as_the_host_does(kw):
    """the learn and the apply launch on the device's own search records against the host learners' (tfe_nt_support.learner_round)"""
    import torch
    a = plain_learner(ROUND_GAMES, **kw)
    a.weights_dev.copy_(torch.from_numpy(weights("seeded").copy()))
    a.rollout_layers = 1
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if a.tc else None
    rec = learner_round(a, coherence=coherence)
    assert rec["acc_equal"] and rec["weights_equal"] and rec["acc_zero"], kw
    assert rec["ended"] >= 1 and rec["cut"] >= 1 and rec["ended"] + rec["cut"] == ROUND_GAMES and rec["values_any"], (rec["ended"], rec["cut"])
    assert rec["stats"] == {k: rec["host"][k] for k in ("learnt", "skipped", "clamped")} and rec["host"]["skipped"] == rec["cut"]
    assert rec["host"]["learnt"] + rec["host"]["skipped"] == rec["moves"] and rec["acc_adds"] == a.n_features * rec["host"]["learnt"] and rec["moved"] > 0
    assert a.round == 1


# ------------------------------------------------------------------ the score
def test_it_learns():
    """The default network, 4,096 games per round, max_steps 4,096, epsilon 0, seed 0, two rounds: one agent plays its rounds under
    search one chance layer deep (rollout_layers = 1), one as before (0).  Then 1,024 one-ply evaluation games from the default
    evaluation boards on each and on zero weights, paired by board.  Asserted: the search-trained network beats zero weights by at
    least three standard errors of the paired difference.  Printed, not asserted: the paired difference between the two trained
    networks, the roll-outs' mean lengths and the two round times between HIP events.  On an MI355X (one run): zero weights
    2,025.6 +- 29.0, trained one-ply 6,640.7 +- 96.6, trained under search 2,821.3 +- 41.7: +795.7 +- 49.9 over zero weights (16
    standard errors) and -3,819.5 +- 105.1 against the one-ply-trained network -- after two rounds the network trained on the search's
    games plays WORSE one ply deep than the one trained on its own (DESIGN.md section 13.5 has twelve rounds: still worse).  Roll-out
    mean lengths 178 / 402 one-ply and 577 / 715 under search; rounds 31 / 73 ms and 155 / 191 ms."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    dev = torch.device("cuda:0")
    agents, lengths, seconds = {}, {}, {}
    for layers in (1, 0):
        a = NTupleTDAfterstateTFEGPU(dev, 4096, max_steps=4096, seed=0)
        a.rollout_layers = layers
        lengths[layers], seconds[layers] = [], []
        for _ in range(2):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            a.learn_batch()
            stop.record()
            stop.synchronize()
            seconds[layers].append(start.elapsed_time(stop) * 1e-3)
            lengths[layers].append(a.lengths.double().mean().item())
        agents[layers] = a
    st = agents[1].stats()
    assert agents[1].round == 2 and st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not agents[1].acc.any().item()
    ev = {layers: a.evaluate(n_games=1024, per_game=True) for layers, a in agents.items()}
    zero = NTupleTDAfterstateTFEGPU(dev, 1024, max_steps=4096, seed=0).evaluate(n_games=1024, per_game=True)

    def paired(x, y):
        d = (x["total_score"] - y["total_score"]).astype(np.float64)
        return d.mean(), d.std(ddof=1) / np.sqrt(d.size)
    se = lambda e: e["std_score"] / e["games"] ** .5
    gain, gain_se = paired(ev[1], zero)
    diff, diff_se = paired(ev[1], ev[0])
    print("1,024 one-ply games after two rounds of 4,096: zero weights", zero["mean_score"], "+-", se(zero), "trained one-ply", ev[0]["mean_score"], "+-",
          se(ev[0]), "trained under search", ev[1]["mean_score"], "+-", se(ev[1]), "search-trained minus zero", gain, "+-", gain_se,
          "search-trained minus one-ply-trained", diff, "+-", diff_se, "roll-out mean lengths per round: one-ply", lengths[0], "search", lengths[1],
          "round seconds: one-ply", seconds[0], "search", seconds[1])
    assert ev[1]["games"] == ev[0]["games"] == zero["games"] == 1024
    assert gain >= 3.0 * gain_se, (ev[1]["mean_score"], zero["mean_score"], gain_se)
