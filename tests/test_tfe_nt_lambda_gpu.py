"""The 2048 n-tuple network's TD(lambda) learner on the device (csrc/tfe_ntuple_lambda.hip:
pulse_tfe_nt_learn_lambda) against the host's statement of it (lambda_deltas_on_host, learn_lambda_nt_on_host, apply_nt_on_host) on
the device's own recorded games.  Every comparison is exact: the lambda-differences as float64 bit patterns, the accumulators and
counters as integers, the weights as float32 bit patterns.  Every buffer a launch is handed sits between guard words; `deltas` holds
a pattern before the first launch and must keep it at and beyond a game's length.

Shape: the learners' regime (tests/tfe_nt_support.py) -- 257 games (one full workgroup of the adds and one of one lane; five wavefronts of the walk, the last
of one lane, with games of mixed lengths in each), max_steps 256, epsilon .25, the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), seed
457, board_id0 3000 -- at lambda .5, gamma 1.  Three rounds, played once and shared; rounds 1 and 2 run on the device's own weights.
(The roll-out itself is held to the host's in test_tfe_nt_gpu.py; here its records are the input.)"""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, guards_intact
from tests.tfe_nt_support import EPSILON_PLAY as EPSILON
from tests.tfe_nt_support import BOARD_ID0, GAMES, MAX_STEPS, ROUNDS, SEED, TUPLES, bits, learner_agent, learner_round, nt, worked_games

pytestmark = pytest.mark.gpu

LAM = .5
DELTAS_PATTERN = -4321.125
_agent = functools.partial(learner_agent, extra_buffers=("deltas",), patterns=dict(PATTERNS, deltas=DELTAS_PATTERN), lam=LAM)


def _round(a):
    """learner_round with this file's verdicts on `deltas`: at t < L the host's lambda-differences, at t >= L what the buffer held
    before the launch; not the one-step differences; and trajectory_deltas() is the buffer trimmed to the longest game"""
    deltas_before = bits(a.deltas.cpu().numpy())

    def after_learn(a, h):
        deltas, steps = bits(a.deltas.cpu().numpy()), h.got["steps"]
        return dict(deltas_equal=np.array_equal(deltas[h.played], bits(h.host_deltas)[h.played]),
                    deltas_kept=np.array_equal(deltas[~h.played], deltas_before[~h.played]),
                    deltas_differ=int((deltas[h.played] != bits(nt().lambda_deltas_on_host(h.values, steps, h.L, a.gamma, 0.0))[h.played]).sum()),
                    trajectory_equal=np.array_equal(bits(a.trajectory_deltas()), deltas[:int(h.L.max())]))
    return learner_round(a, after_learn)


@functools.lru_cache(maxsize=None)
def _rounds():
    a = _agent()
    out = [_round(a) for _ in range(ROUNDS)]
    guards_intact(a)
    return a, out


def test_every_round_has_ended_and_cut_games():
    """... and every wavefront of the walk has games of different lengths"""
    _, rounds = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["ended"] >= 8 and rec["cut"] >= 8 and rec["ended"] + rec["cut"] == GAMES, (r, rec["ended"], rec["cut"])
        assert all(len(set(rec["lengths"][w:w + 64].tolist())) > 1 for w in range(0, 256, 64)), r
        assert 0 < rec["lengths"].min() < rec["lengths"].max() == MAX_STEPS


def test_deltas_equal_the_host_bit_for_bit():
    """G1: at t < L the float64 bit patterns of lambda_deltas_on_host on the device's own values / steps / lengths; at t >= L what
    `deltas` held before the launch -- the pattern in round 0.  lambda enters: they are not the one-step differences."""
    a, rounds = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["deltas_equal"] and rec["deltas_kept"] and rec["trajectory_equal"], r
        assert rec["deltas_differ"] > 0, r
    assert rounds[1]["values_any"] and rounds[2]["values_any"]
    deltas, L = bits(a.deltas.cpu().numpy()), np.maximum.reduce([rec["lengths"] for rec in rounds])
    never = np.arange(MAX_STEPS)[:, None] >= L[None, :]                    # rows no round has played
    assert never.any() and (deltas[never] == bits([DELTAS_PATTERN])[0]).all()


def test_learn_and_apply_equal_the_host():
    """G2: acc read back before the apply launch, over all W; the three counters; the weights after the apply launch"""
    a, rounds = _rounds()
    for r, rec in enumerate(rounds):
        assert rec["acc_equal"] and rec["stats"] == rec["host"], (r, rec["stats"], rec["host"])
        assert rec["stats"]["learnt"] + rec["stats"]["skipped"] == rec["moves"] and rec["stats"]["skipped"] == rec["cut"], r
        assert rec["acc_adds"] == a.n_features * rec["stats"]["learnt"], r
        assert rec["weights_equal"] and rec["acc_zero"] and rec["moved"] > 0, r


def test_lambda_zero_is_pulse_tfe_nt_learn():
    """G3: on the games the third round recorded, the new entry point at lambda 0 leaves the accumulators and counters of
    pulse_tfe_nt_learn, device against device"""
    a, _ = _rounds()
    assert not a.acc.any().item()
    out = []
    for lam in (LAM, 0.0):                                                 # learn() of an agent with lam 0 is pulse_tfe_nt_learn
        a.lam, before = lam, a.stats()
        if lam:
            a.learn_lambda_launch(0.0)
        else:
            a.learn()
        out.append((a.acc.cpu().numpy(), {k: v - before[k] for k, v in a.stats().items()}))
        a.acc.zero_()
    a.lam = LAM
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][1]["learnt"] > 0 and out[0][0][:, 1].any()
    guards_intact(a)


@pytest.mark.parametrize("kw", [dict(symmetric=False), dict(gamma=0.9)], ids=["plain", "gamma"])
def test_other_settings(kw):
    """G4: one feature per tuple; gamma .9, where gl = .45 is a rounded product.  On weights that are not zero, so V enters."""
    import torch
    a = _agent(**kw)
    w = (np.random.default_rng(19).standard_normal(a.n_weights) * 3).astype(np.float32)
    a.weights_dev.copy_(torch.from_numpy(w))
    rec = _round(a)
    guards_intact(a)
    assert rec["values_any"] and rec["ended"] >= 1 and rec["cut"] >= 1
    assert rec["deltas_equal"] and rec["deltas_kept"] and rec["deltas_differ"] > 0
    assert rec["acc_equal"] and rec["stats"] == rec["host"] and rec["acc_adds"] == a.n_features * rec["stats"]["learnt"]
    assert rec["weights_equal"] and rec["acc_zero"]


def test_hand_made_buffers():
    """G5: the hand-worked games (tests/tfe_nt_support.py: worked_games) copied into an agent of 2 games and 3 moves: the clamp of the add (twice), the
    unclamped carry and the cut game's skipped move, on the device"""
    import torch
    keys, values, steps, lengths = worked_games()
    a = _agent(2, tuples=((0, 3),), max_steps=3, gamma=1.0)
    a.keys.copy_(torch.from_numpy(keys.view(np.int64)))
    a.values.copy_(torch.from_numpy(values))
    a.steps.copy_(torch.from_numpy(steps))
    a.lengths.copy_(torch.tensor(lengths, dtype=torch.int32))
    a.learn()
    st = a.stats()
    assert (st["learnt"], st["skipped"], st["clamped"]) == (4, 1, 2)
    deltas = a.deltas.cpu().numpy()
    assert bits(deltas).tolist() == bits([[9993.0, 7.5], [-19996.0, 0.0], [-2.0, DELTAS_PATTERN]]).tolist()
    total = 8192 * 65536 - 8192 * 65536 - 2 * 65536 + 491520
    want = np.zeros((256, 2), dtype=np.int64)
    want[0], want[1], want[16] = (4 * total, 16), (2 * total, 8), (2 * total, 8)
    assert np.array_equal(a.acc.cpu().numpy(), want)
    guards_intact(a)


def test_save_and_load_continue_the_run(tmp_path):
    """G6: saved after two rounds, loaded and run one more round: the weights of the uninterrupted agent after three, bit for bit"""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    a, _ = _rounds()
    b = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), GAMES, tuples=TUPLES, epsilon=EPSILON, max_steps=MAX_STEPS, seed=SEED, board_id0=BOARD_ID0, lam=LAM)
    b.learn_batch().learn_batch().save(tmp_path / "net.npz")
    c = NTupleTDAfterstateTFEGPU.load(tmp_path / "net.npz", torch.device("cuda:0"))
    assert c.lam == LAM and c.deltas is not None and c.round == 2
    c.learn_batch()
    assert c.round == a.round == 3 and np.array_equal(c.weights().view(np.uint32), a.weights().view(np.uint32))
    plain = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), GAMES, tuples=TUPLES, max_steps=MAX_STEPS)
    assert plain.lam == 0.0 and plain.deltas is None                       # lam = 0 allocates nothing more


def test_score():
    """G7.  The default network, 4,096 games per round, max_steps 4,096, epsilon 0, gamma 1, alpha 1, seed 0; two agents, lambda 0 and
    lambda .5, 12 rounds each, each evaluated greedily on the same 2,048 default boards.  Asserted: the lambda agent beats zero weights
    by five standard errors (section 13's condition), and is no worse than the lambda-0 agent by three standard errors of the paired
    per-board difference.  Rehearsed on the host at 256 games per round: lambda .5 ahead by 1,158 +- 381 at round 12.  On an MI355X
    (one run): 1,993.3 +- 19.9 on zero weights; lambda 0: 13,165.7 +- 112.0 (mean length 778.1); lambda .5: 16,237.1 +- 134.3 (925.0);
    lambda .5 minus lambda 0, paired by board: +3,071.4 +- 173.1.  No game cut, no difference clamped."""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    se = lambda e: e["std_score"] / e["games"] ** .5
    evals = {}
    for lam in (0.0, LAM):
        a = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), 4096, max_steps=4096, seed=0, lam=lam)
        if lam:
            evals["zero"] = a.evaluate(n_games=2048)
        for _ in range(12):
            a.learn_batch()
        evals[lam] = a.evaluate(n_games=2048, per_game=True)
        st = a.stats()
        assert st["learnt"] + st["skipped"] == st["moves"] and st["skipped"] == st["truncated"] and not a.acc.any().item()
        print("lambda", lam, "after 12 rounds: greedy mean score on 2,048 games", evals[lam]["mean_score"], "+-", se(evals[lam]), "mean length",
              evals[lam]["mean_length"], "cut", evals[lam]["truncated"], "stats", st)
        del a
        torch.cuda.empty_cache()
    diff = (evals[LAM]["total_score"] - evals[0.0]["total_score"]).astype(np.float64)
    diff_se = diff.std(ddof=1) / np.sqrt(diff.size)
    print("zero weights", evals["zero"]["mean_score"], "+-", se(evals["zero"]), "; lambda .5 minus lambda 0, paired by board:", diff.mean(), "+-", diff_se)
    assert evals[LAM]["mean_score"] - evals["zero"]["mean_score"] >= 5.0 * np.hypot(se(evals[LAM]), se(evals["zero"]))
    assert diff.mean() >= -3.0 * diff_se, (diff.mean(), diff_se)
