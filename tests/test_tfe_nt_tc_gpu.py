"""The 2048 n-tuple network's temporal-coherence step sizes on the device (csrc/tfe_ntuple_tc.hip:
pulse_tfe_nt_learn_tc, pulse_tfe_nt_apply_tc) against the host's statement of them (learn_tc_nt_on_host, apply_tc_nt_on_host) on the
device's own recorded games.  Every comparison is exact: the three accumulators, the counters and tc_stats as integers, the weights as
float32 bit patterns, E and A as float64 bit patterns.  Every buffer a launch is handed sits between guard words.

Shape: the learners' regime (tests/tfe_nt_support.py) -- 257 games (one full workgroup of the adds and one of one lane), max_steps 256, epsilon
.25, seed 457, board_id0 3000 -- on the tuples (0, 1, 2, 3) and (15,): 65,552 weights, so that most visited weights are visited in
every round and rho leaves 1.  Three rounds per setting, played once and shared; the host's E and A are carried by the host from zero,
the weights a round starts from are the device's."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import guards_intact
from tests.tfe_nt_support import GAMES, ROUNDS, STEP_SIZE, bits, learner_agent, learner_round, plain_learner, tc_worked, tc_worked_state

pytestmark = pytest.mark.gpu

TUPLES = ((0, 1, 2, 3), (15,))
SETTINGS = {"td0": dict(lam=0.0), "lambda": dict(lam=0.5), "td0-plain": dict(lam=0.0, symmetric=False), "lambda-plain": dict(lam=0.5, symmetric=False),
            "td0-gamma": dict(lam=0.0, gamma=0.9), "lambda-gamma": dict(lam=0.5, gamma=0.9)}
_plain = functools.partial(plain_learner, tuples=TUPLES, tc=True)
_agent = functools.partial(learner_agent, extra_buffers=("acc_abs", "E", "A", "tc_stats", "deltas"), tuples=TUPLES, tc=True)


def _round(a, host_E, host_A):
    """learner_round with this file's verdicts: the third accumulator, tc_stats' differences against the host's (moved, rho sum), and
    E and A against host_E / host_A, the host's own, advanced in place"""
    def after_learn(a, h):
        h.tc_before = a.tc_stats.cpu().numpy().copy()
        return dict(abs_equal=np.array_equal(h.acc_abs, h.host_abs), abs_any=bool(h.acc_abs.any()), abs_bounds=bool((h.acc_abs >= np.abs(h.acc[:, 0])).all()))

    def after_apply(a, h):
        E, A = a.coherence()
        return dict(host_tc=h.host_tc, tc=tuple((a.tc_stats.cpu().numpy() - h.tc_before).tolist()), E_equal=np.array_equal(bits(E), bits(host_E)),
                    A_equal=np.array_equal(bits(A), bits(host_A)), coherent=bool((np.abs(E) <= A).all()))
    return learner_round(a, after_learn, after_apply, coherence=(host_E, host_A))


@functools.lru_cache(maxsize=None)
def _rounds(setting):
    import torch
    kw = SETTINGS[setting]
    a = _agent(**kw)
    if len(kw) > 1:                                                        # the plain and the gamma settings start on weights that are not zero
        a.weights_dev.copy_(torch.from_numpy((np.random.default_rng(19).standard_normal(a.n_weights) * 3).astype(np.float32)))
    first = a.weights()
    E, A = np.zeros(a.n_weights), np.zeros(a.n_weights)
    out = [_round(a, E, A) for _ in range(ROUNDS)]
    guards_intact(a)
    return a, out, first


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_three_rounds_equal_the_host(setting):
    """acc, acc_abs and the counters before the apply launch; the weights, E, A and tc_stats after it; every round has ended games and,
    from zero weights, cut ones; once differences of both signs have met at a weight rho is below 1 somewhere (the round's sum of rho falls short of the
    count): from the second round on weights that are not zero, from the third on zero weights"""
    a, rounds, _ = _rounds(setting)
    for r, rec in enumerate(rounds):
        assert rec["ended"] >= 1 and rec["ended"] + rec["cut"] == GAMES, (r, rec["ended"], rec["cut"])
        assert rec["cut"] >= 1 or len(SETTINGS[setting]) > 1, r            # (from zero weights; on the random ones a round may end every game)
        assert rec["acc_equal"] and rec["abs_equal"] and rec["abs_any"] and rec["abs_bounds"] and rec["stats"] == rec["host"], (r, rec["stats"], rec["host"])
        assert rec["stats"]["skipped"] == rec["cut"] and rec["stats"]["learnt"] > 1000, r
        assert rec["weights_equal"] and rec["E_equal"] and rec["A_equal"] and rec["acc_zero"] and rec["coherent"], r
        assert rec["tc"] == rec["host_tc"] + (0, 0) and rec["tc"][0] == rec["visited"] > 50, (r, rec["tc"], rec["host_tc"])
        assert (r > 0 or len(SETTINGS[setting]) > 1) == rec["values_any"], r
    assert rounds[0]["tc"][1] == rounds[0]["tc"][0] << 32                  # zero E and A: rho = 1.0 at every weight
    # on zero weights every V of round 0 is 0 and no difference is negative (a reward, or 0 - 0): E = A and rho is still 1.0 in round 1
    for r in (1, 2):
        if r == 1 and len(SETTINGS[setting]) == 1:
            assert rounds[r]["tc"][1] == rounds[r]["tc"][0] << 32
        else:
            assert 0 < rounds[r]["tc"][1] < rounds[r]["tc"][0] << 32, r


@pytest.mark.parametrize("setting", ["td0", "lambda"])
def test_device_against_device(setting):
    """the first round of a tc agent leaves the weights of the agent without tc on the same seed; on the games the third round
    recorded pulse_tfe_nt_learn_tc leaves the acc and the counters of pulse_tfe_nt_learn / pulse_tfe_nt_learn_lambda; tc_summary reads
    and zeroes tc_stats; clear() zeroes the new state"""
    a, rounds, _ = _rounds(setting)
    b = _plain(tc=False, **SETTINGS[setting])
    assert b.acc_abs is None and b.E is None and b.A is None and b.tc_stats is None      # tc = False allocates nothing more
    assert (b.deltas is None) == (setting == "td0")
    b.learn_batch()
    c = _plain(**SETTINGS[setting]).learn_batch()
    assert np.array_equal(b.weights().view(np.uint32), c.weights().view(np.uint32)) and b.weights().any()
    assert c.tc_summary() == dict(moved=rounds[0]["tc"][0], mean_rho=1.0) and c.tc_summary() == dict(moved=0, mean_rho=1.0)
    assert not a.acc.any().item() and not a.acc_abs.any().item()
    out = []
    for tc in (True, False):
        a.tc, before = tc, a.stats()
        a.learn()
        out.append((a.acc.cpu().numpy(), {k: v - before[k] for k, v in a.stats().items()}))
        a.acc.zero_()
    a.tc, abs_written = True, a.acc_abs.any().item()                       # only the tc launch wrote it
    a.acc_abs.zero_()
    assert abs_written and np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][1]["learnt"] > 0 and out[0][0][:, 1].any()
    total = sum(rec["tc"][1] for rec in rounds) / sum(rec["tc"][0] for rec in rounds) * 2.0 ** -32
    s = a.tc_summary()
    assert s["moved"] == sum(rec["tc"][0] for rec in rounds) and s["mean_rho"] == total and 0.0 < total < 1.0 and not a.tc_stats.any().item()
    guards_intact(a)
    c.learn_batch().rollout()
    c.learn()
    assert c.E.any().item() and c.A.any().item() and c.acc_abs.any().item() and c.tc_stats.any().item()
    c.clear()
    assert not any(getattr(c, k).any().item() for k in ("weights_dev", "acc", "acc_abs", "E", "A", "tc_stats", "counters")) and c.round == 0


def test_launches_allocate_on_first_use():
    """learn_tc_launch and apply_tc_launch on an agent built without tc: the state appears, zeroed, and deltas only with lam > 0"""
    a = _plain(64, tc=False, max_steps=64)
    a.rollout()
    a.learn_tc_launch(0.0)
    assert a.deltas is None and a.acc_abs is not None and a.acc_abs.any().item() and not a.E.any().item()
    a.apply_tc_launch()
    s = a.tc_summary()
    assert s["moved"] > 0 and s["mean_rho"] == 1.0 and not a.acc.any().item() and not a.acc_abs.any().item() and a.E.any().item()
    a.learn_tc_launch(0.5)
    assert a.deltas is not None and a.acc_abs.any().item()
    b = _plain(64, tc=False, max_steps=64)
    with pytest.raises(ValueError, match="no temporal-coherence launch"):
        b.coherence()
    with pytest.raises(ValueError, match="no temporal-coherence launch"):
        b.tc_summary()


def test_hand_made_buffers():
    """the two hand-worked rounds (tests/tfe_nt_support.py: tc_worked) copied into an agent of 3 games and 3 moves: the clamp, the cut game's skipped move,
    a game of length 0, a turned sign (rho = 11 / 32,787), a weight seen in round 1 only and one whose A is still 0"""
    import torch
    a = _agent(3, tuples=((0, 3),), max_steps=3, gamma=1.0, epsilon=0.0)
    assert a.alpha / a.n_features == STEP_SIZE
    learnt = dict(learnt=0, skipped=0, clamped=0)
    for r, ((keys, values, steps, lengths), want) in enumerate(zip(tc_worked(), tc_worked_state())):
        want_acc, want_ab, want_st, want_w, want_E, want_A, want_tc = want
        a.keys.copy_(torch.from_numpy(keys.view(np.int64)))
        a.values.copy_(torch.from_numpy(values))
        a.steps.copy_(torch.from_numpy(steps))
        a.lengths.copy_(torch.tensor(lengths, dtype=torch.int32))
        a.learn()
        learnt = {k: learnt[k] + want_st[k] for k in learnt}
        assert {k: a.stats()[k] for k in learnt} == learnt, r
        assert np.array_equal(a.acc.cpu().numpy(), want_acc) and np.array_equal(a.acc_abs.cpu().numpy(), want_ab), r
        a.apply()
        assert tuple(a.tc_stats.cpu().tolist()) == want_tc + (0, 0), r
        a.tc_stats.zero_()
        E, A = a.coherence()
        assert np.array_equal(a.weights().view(np.uint32), want_w.view(np.uint32)), r
        assert np.array_equal(bits(E), bits(want_E)) and np.array_equal(bits(A), bits(want_A)), r
        assert not a.acc.any().item() and not a.acc_abs.any().item(), r
    guards_intact(a)


def test_untouched_weights_keep_their_state():
    """E, A and the weights pre-filled with patterns: a weight with cnt == 0 keeps all three bit for bit; a visited one follows the
    host on the patterns (rho = 3.5 / 7.25)"""
    import torch
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a = _agent(lam=0.5)
    a.weights_dev.fill_(-1.5)
    a.E.fill_(-3.5)
    a.A.fill_(7.25)
    a.rollout()
    a.learn()
    acc, acc_abs = a.acc.cpu().numpy(), a.acc_abs.cpu().numpy()
    w, E, A = np.full(a.n_weights, -1.5, dtype=np.float32), np.full(a.n_weights, -3.5), np.full(a.n_weights, 7.25)
    rest = acc[:, 1] == 0
    a.apply()
    moved, rho_sum = nt.apply_tc_nt_on_host(w, acc, acc_abs, E, A, a.alpha / a.n_features)
    assert 100 < moved == a.n_weights - int(rest.sum()) and int(rest.sum()) > 1000
    got_E, got_A = a.coherence()
    assert (bits(got_E)[rest] == bits([-3.5])[0]).all() and (bits(got_A)[rest] == bits([7.25])[0]).all()
    assert (a.weights().view(np.uint32)[rest] == np.float32(-1.5).view(np.uint32)).all()
    assert np.array_equal(bits(got_E), bits(E)) and np.array_equal(bits(got_A), bits(A)) and np.array_equal(a.weights().view(np.uint32), w.view(np.uint32))
    assert tuple(a.tc_stats.cpu().tolist()) == (moved, rho_sum, 0, 0) and rho_sum == moved * int(np.rint(np.ldexp(3.5 / 7.25, 32)))
    guards_intact(a)


def test_save_and_load_continue_the_run(tmp_path):
    """saved after two rounds, loaded and run one more round: the weights, E and A of the uninterrupted agent after three, bit for bit"""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
    a, _, _ = _rounds("lambda")
    b = _plain(lam=0.5)
    b.learn_batch().learn_batch().save(tmp_path / "net.npz")
    f = nt.read_checkpoint(tmp_path / "net.npz")
    assert f["tc"] is True and f["lam"] == 0.5 and len(f["tc_index"]) > 100 and (np.diff(f["tc_index"]) > 0).all()
    c = NTupleTDAfterstateTFEGPU.load(tmp_path / "net.npz", torch.device("cuda:0"))
    assert c.tc and c.lam == 0.5 and c.round == 2 and c.acc_abs is not None and not c.tc_stats.any().item()
    c.learn_batch()
    assert c.round == a.round == 3 and np.array_equal(c.weights().view(np.uint32), a.weights().view(np.uint32))
    for x, y in zip(c.coherence(), a.coherence()):
        assert np.array_equal(bits(x), bits(y)) and x.any()
    plain = _plain(tc=False)
    plain.learn_batch().save(tmp_path / "plain.npz")
    f = nt.read_checkpoint(tmp_path / "plain.npz")
    assert f["tc"] is False and NTupleTDAfterstateTFEGPU.load(tmp_path / "plain.npz", torch.device("cuda:0")).acc_abs is None


def test_score():
    """The default network, 4,096 games per round, max_steps 4,096, epsilon 0, gamma 1, alpha 1, seed 0, lambda 0; two agents, with and
    without tc, 12 rounds each, each evaluated greedily on the same 2,048 default boards.  Asserted: the tc agent beats zero weights by
    five standard errors (section 13's condition).  Printed and NOT asserted: the tc agent minus the agent without, paired by board --
    the rehearsed gain of TC is at round 39, and whether it is ahead as early as round 12 is a measurement.
    On an MI355X (one run): 1,993.3 +- 19.9 on zero weights; without tc 13,165.7 +- 112.0 (mean length 778.1); with tc 13,683.2 +- 120.5
    (802.4); tc minus no tc, paired by board: +517.5 +- 165.9; mean rho of round 12: 0.9801.  No game cut, no difference clamped."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    se = lambda e: e["std_score"] / e["games"] ** .5
    evals = {}
    for tc in (False, True):
        a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0, tc=tc)
        if tc:
            evals["zero"] = a.evaluate(n_games=2048)
        rho = []
        for _ in range(12):
            a.learn_batch()
            if tc:
                rho.append(round(a.tc_summary()["mean_rho"], 4))
        evals[tc] = a.evaluate(n_games=2048, per_game=True)
        st = a.stats()
        assert st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not a.acc.any().item()
        print("tc", tc, "after 12 rounds: greedy mean score on 2,048 games", evals[tc]["mean_score"], "+-", se(evals[tc]), "mean length",
              evals[tc]["mean_length"], "cut", evals[tc]["truncated"], "stats", st, "mean rho per round", rho)
        del a
        torch.cuda.empty_cache()
    diff = (evals[True]["total_score"] - evals[False]["total_score"]).astype(np.float64)
    print("zero weights", evals["zero"]["mean_score"], "+-", se(evals["zero"]), "; tc minus no tc, paired by board:", diff.mean(), "+-",
          diff.std(ddof=1) / np.sqrt(diff.size))
    assert evals[True]["mean_score"] - evals["zero"]["mean_score"] >= 5.0 * np.hypot(se(evals[True]), se(evals["zero"]))
