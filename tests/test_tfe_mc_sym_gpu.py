"""The 2048 Monte-Carlo symmetries and evaluation launch on the device (csrc/tfe_mc.hip: pulse_tfe_mc_rollout_canon,
pulse_tfe_mc_evaluate) against the plain roll-out, the host mirror (tests/tfe_host.py) and the
environment's own kernels.  Every buffer a launch is handed sits between guard words.

Shapes: 300 games (two workgroups, the second partial) at n = 2 and n = 3 with max_steps = 64, 70 games at n = 4 with max_steps = 48,
capacity 2^12.  Rehearsed on the host: n = 3 cuts 5 of 300 games at 64 moves in round 0 and finishes the rest, n = 4 cuts 68 - 70 of 70,
n = 2 finishes all but a few; every shape draws tie coins from round 1 on.  One round of 300 games at n = 3 meets 8,019 states (6,394
canonical ones), and three rounds at n = 4 9,403: more than 2^12 slots, so there the learner DROPS first visits and WHICH keys are
stored is a race.  At capacity 2^12 the tables of n = 3 and n = 4 are therefore held to what a race cannot change (a stored entry
holds all of its key's returns; stored + dropped = all), and the same shapes run again at 2^16, where nothing is dropped and
every table must equal the host's exactly, as n = 2 must at 2^12."""
import numpy as np
import pytest

from tests.tfe_gpu_support import guard, guarded, guards_intact, read, replay

pytestmark = pytest.mark.gpu

BUFFERS = ("entries", "keys", "steps", "lengths", "total_score", "episode_reward", "counters", "_eval")
#         n, games, max_steps, capacity
SHAPES = [(2, 300, 64, 1 << 12), (3, 300, 64, 1 << 12), (4, 70, 48, 1 << 12)]
ROOMY = [(3, 300, 64, 1 << 16), (4, 70, 48, 1 << 16)]


def _fits(shape):
    return shape[0] == 2 or shape[3] >= 1 << 16


def _agent(shape, symmetric, seed=None, **kw):
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    n, n_games, max_steps, capacity = shape
    a = guard(OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), n_games, board_size=n, capacity=capacity, max_steps=max_steps,
                                         seed=10 * n + 1 if seed is None else seed, board_id0=7, symmetric=symmetric, **kw), BUFFERS)
    assert a.entries.data_ptr() % 128 == 0
    return a


def _read(a):
    """the last roll-out: keys / actions / rewards / first [T, B] over the moves played (`played`), and the per-game arrays"""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import unpack_steps
    got = read(a)
    act, rew, first = unpack_steps(got["steps"])
    return dict(got, actions=act.astype(np.int64), rewards=rew, first=first, played=np.arange(a.max_steps)[:, None] < got["lengths"][None, :])


def _replay(a, got):
    """The recorded games through TFEBatch (pulse_tfe_reset / pulse_tfe_step): the environment meets the recorded states (after
    canonicalisation for a symmetric agent) under the actions mapped back to the board's frame.  Returns the final boards."""
    from tests.tfe_host import ACTION_UNMAP, canon_many, pack_boards

    def recorded_state(t, live, boards, actions):
        keys, j = canon_many(boards) if a.symmetric else (pack_boards(boards), np.zeros(a.n_games, dtype=np.int64))
        assert np.array_equal(keys[live], got["keys"][t][live]), t
        return ACTION_UNMAP[j, actions]
    final, _, done = replay(a, got, recorded_state)
    assert (done | (got["lengths"] == a.max_steps)).all()                  # a game ends where the environment says, or at max_steps
    return final


def _branches(a, got, table, epsilon):
    """(present, greedy) bool[T, B] of the recorded moves: the state had an entry; and the draw was not the epsilon branch's --
    recomputed from Philox (agent_seed, board id, t) on the host"""
    from tests.tfe_host import philox_many
    eps_q24 = int(np.floor(epsilon * 2.0 ** 24))
    ids = [a.round_board_id0() + g for g in range(a.n_games)]
    present = np.isin(got["keys"], np.array(sorted(table), dtype=np.uint64)) & got["played"]
    greedy = np.zeros_like(present)
    for t in np.nonzero(present.any(axis=1))[0].tolist():
        x = philox_many(a.agent_seed, ids, t)[:, 0]
        greedy[t] = present[t] & ((x >> 8) >= eps_q24)
    return present, greedy


# ------------------------------------------------------------------ 1. an empty table
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_empty_table_plays_the_plain_games(shape):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import first_visit_flags_on_host
    from tests.tfe_host import ACTION_MAP, canon_keys
    plain, sym = _agent(shape, False), _agent(shape, True)
    p, s = _read(plain.rollout()), _read(sym.rollout())
    for name in ("lengths", "total_score", "episode_reward"):
        assert np.array_equal(p[name], s[name]), name
    on = p["played"]
    key_c, j = canon_keys(p["keys"], shape[0])
    assert np.array_equal(s["keys"][on], key_c[on])
    assert np.array_equal(s["actions"][on], ACTION_MAP[j, p["actions"]][on])
    assert np.array_equal(s["rewards"][on], p["rewards"][on]) and np.array_equal(s["first"][on], p["first"][on])
    assert (j[on] > 0).any() and (p["keys"][on] != key_c[on]).any()         # the frames differ somewhere
    for g in range(0, shape[1], 7):                                         # ... and the first bits are the dict rule on canonical pairs
        L = int(s["lengths"][g])
        assert np.array_equal(s["first"][:L, g], first_visit_flags_on_host(s["keys"][:L, g], s["actions"][:L, g]))
    cut = int((p["lengths"] == shape[2]).sum())
    assert plain.stats()["truncated"] == sym.stats()["truncated"] <= cut and sym.stats()["steps"] == int(p["lengths"].sum())
    if shape[0] >= 3:
        assert sym.stats()["truncated"] > 0                                # rehearsed: 5 of 300 at n = 3, 70 of 70 at n = 4
    if shape[0] <= 3:
        assert sym.stats()["truncated"] < shape[1] // 2                    # ... and games that finish
    guards_intact(plain, sym)


# ------------------------------------------------------------------ 2. the fold
@pytest.mark.parametrize("shape", SHAPES + ROOMY, ids=str)
def test_one_round_learns_the_folded_table(shape):
    """The games of round 0 are the same in both frames, so the symmetric table is the plain one folded -- in exact integers -- and
    the host learner's over the recorded canonical trajectory."""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    plain, sym = _agent(shape, False), _agent(shape, True)
    plain.rollout().learn()
    sym.rollout().learn()
    s, p = _read(sym), _read(plain)
    host = mc.learn_on_host(s["keys"], s["steps"], s["lengths"], sym.gamma, sym.frac_bits, {})
    host_plain = mc.learn_on_host(p["keys"], p["steps"], p["lengths"], plain.gamma, plain.frac_bits, {})
    assert mc.fold_table_on_host(host_plain, shape[0]) == host              # (the host's statement of the claim)
    table, stats = sym.table(), sym.stats()
    print(shape, "states", len(table), "of", len(host), "canonical,", len(plain.table()), "of", len(host_plain), "plain; dropped", stats["dropped"], plain.stats()["dropped"])
    assert all(mc.canon_key_on_host(k, shape[0]) == (k, 0) for k in table)
    assert stats["first_visits"] == sum(sum(c) for c, _ in table.values())
    assert stats["first_visits"] + stats["dropped"] == sum(sum(c) for c, _ in host.values())
    if _fits(shape):
        assert stats["dropped"] == 0 and plain.stats()["dropped"] == 0
        assert table == host
        assert table == mc.fold_table_on_host(plain.table(), shape[0])
        assert len(table) < len(plain.table())
    else:                                                                   # which keys found room is a race; what is stored is whole
        assert table == {k: host[k] for k in table}
        assert plain.table() == {k: host_plain[k] for k in plain.table()}
    guards_intact(plain, sym)


# ------------------------------------------------------------------ 3. a warm table
@pytest.mark.parametrize("shape", SHAPES + ROOMY, ids=str)
def test_three_symmetric_rounds(shape):
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_on_host
    a = _agent(shape, True)
    n = shape[0]
    host, mirror, ties, greedy_moves = {}, {}, 0, 0
    for r in range(3):
        before = a.table()
        a.rollout()
        got = _read(a)
        # the policy: on the non-epsilon branch of a state with an entry the recorded action is the entry's greedy one, in the canonical frame
        present, greedy = _branches(a, got, before, a.epsilon)
        assert (r == 0) == (not present.any())
        for t, g in zip(*np.nonzero(greedy)):
            key = int(got["keys"][t, g])
            asked = []

            def coins(*args):
                asked.append(args)
                return mc.philox4x32(*args)
            assert got["actions"][t, g] == mc.greedy_on_host(before[key], key, a.tie_seed, r, coins), (r, t, g)
            ties += len(asked)
        greedy_moves += int(greedy.sum())
        final = _replay(a, got)                                            # the games are the environment's own
        assert final.max() >= 8
        if _fits(shape):                                                    # ... and the host mirror's, word for word
            want = rollout_on_host(a.n_games, n, a.max_steps, a.epsilon, mirror, a.env_seed, a.agent_seed, a.tie_seed, a.round_board_id0(), r, canonical=True)
            on = got["played"]
            assert np.array_equal(got["lengths"], want["lengths"]) and np.array_equal(got["total_score"], want["total_score"])
            assert np.array_equal(got["keys"][on], want["keys"][on]) and np.array_equal(got["steps"][on], want["steps"][on])
            mc.learn_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, mirror)
        a.learn()
        a.round += 1
        mc.learn_on_host(got["keys"], got["steps"], got["lengths"], a.gamma, a.frac_bits, host)
        table, stats = a.table(), a.stats()
        assert all(mc.canon_key_on_host(k, n) == (k, 0) for k in table)
        assert stats["first_visits"] == sum(sum(c) for c, _ in table.values())
        assert stats["first_visits"] + stats["dropped"] == sum(sum(c) for c, _ in host.values())
        if _fits(shape):
            assert stats["dropped"] == 0 and table == host == mirror
        else:
            assert table == {k: host[k] for k in table}
    print(shape, "greedy moves", greedy_moves, "tie draws", ties, "states", len(table), "dropped", stats["dropped"], "truncated", stats["truncated"])
    assert greedy_moves > 40 and ties > 0
    guards_intact(a)


# ------------------------------------------------------------------ 4. evaluate against the roll-out
def _evaluate(a, epsilon, zero=True):
    """pulse_tfe_mc_evaluate with guarded per-game outputs; the counters are the agent's (guarded) `_eval` words"""
    import ctypes as C
    import torch
    from pulselib_amd import _native
    score, f1, g1 = guarded(torch.zeros(a.n_games, dtype=torch.int64, device=a.device), -1)
    lengths, f2, g2 = guarded(torch.zeros(a.n_games, dtype=torch.int32, device=a.device), -1)
    o = _native.TfeMCEval()
    o.entries, o.capacity, o.n_games, o.n, o.max_steps, o.frac_bits = a.entries.data_ptr(), a.capacity, a.n_games, a.n, a.max_steps, a.frac_bits
    o.epsilon, o.env_seed, o.agent_seed, o.tie_seed, o.round = epsilon, a.env_seed, a.agent_seed, a.tie_seed, a.round
    o.board_id0, o.canonical = a.round_board_id0(), int(a.symmetric)
    if zero:
        a._eval.zero_()
    o.summary, o.max_tile_hist, o.total_score, o.lengths = a._eval.data_ptr(), a._eval[8:].data_ptr(), score.data_ptr(), lengths.data_ptr()
    _native.check(a._lib.pulse_tfe_mc_evaluate(C.byref(o), _native.current_stream(a.device)), "pulse_tfe_mc_evaluate")
    words = a._eval.cpu().tolist()
    guards_intact([("eval total_score", f1, g1), ("eval lengths", f2, g2)])
    return words, score.cpu().numpy(), lengths.cpu().numpy()


@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_evaluate_plays_the_rollouts_games(shape, symmetric):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import EVAL_SUMMARY, eval_summary_on_host
    from tests.tfe_host import eval_words
    a = _agent(shape, symmetric)
    a.learn_batch().learn_batch()                                          # a table to play against (at 2^12 slots: whatever found room)
    table, raw = a.table(), a.entries.cpu().numpy().copy()
    assert len(table) > 40
    for epsilon in (0.0, 0.1):
        a.epsilon = epsilon
        a.counters.zero_()
        got = _read(a.rollout())                                           # round 2's boards under round 2's coins, not learnt
        words, score, lengths = _evaluate(a, epsilon)
        assert np.array_equal(score, got["total_score"]) and np.array_equal(lengths, got["lengths"])
        present, greedy = _branches(a, got, table, epsilon)
        cut = a.stats()["truncated"]
        want = eval_words(got["total_score"], got["lengths"], _replay(a, got), cut, present.sum(), greedy.sum())
        print(shape, symmetric, epsilon, dict(zip(EVAL_SUMMARY, want)), want[8:])
        assert words == want
        assert present.any() and greedy.any() and (epsilon == 0.0) == (int(present.sum()) == int(greedy.sum()))
        again, _, _ = _evaluate(a, epsilon, zero=False)                    # a second call adds to the counters; the maximum stays
        assert again == [w if i == 4 else 2 * w for i, w in enumerate(want)]
        out = a.evaluate(epsilon=epsilon, board_id0=a.round_board_id0(), per_game=True)          # the class: the same launch, zeroed counters
        assert np.array_equal(out.pop("total_score"), score) and np.array_equal(out.pop("lengths"), lengths)
        assert [out[k] for k in EVAL_SUMMARY] + out["max_tile_hist"] == want and out == eval_summary_on_host(want)
        few = a.evaluate(n_games=65, epsilon=epsilon, board_id0=a.round_board_id0(), per_game=True)    # another batch size; no per-game arrays
        assert np.array_equal(few["total_score"], score[:65]) and few["games"] == 65
        assert a.evaluate(n_games=65, epsilon=epsilon, board_id0=a.round_board_id0())["score_sum"] == int(score[:65].sum())
    assert np.array_equal(a.entries.cpu().numpy(), raw)                     # the table's bytes: only read
    assert a.evaluate()["games"] == shape[1] and a.eval_board_id0() == 7 + (1 << 62)
    guards_intact(a)


# ------------------------------------------------------------------ 5. it learns
def test_it_learns_with_symmetry():
    """tests/test_tfe_mc_gpu.py::test_it_learns under symmetric=True, the scores taken from evaluate(epsilon=0) on the table before
    each round (boards board_id0 + 2^62 + g, the same for every call): 4,096 games of 3 x 3 per round, gamma .9, epsilon .1, seed 0.
    Rehearsed on the CPU with the host mirror (tests/tfe_host.py): mean final score 172.18 +- 1.47 before round 0 (the uniform
    policy), 235.80 +- 1.71, 249.21 +- 1.69 and 266.22 +- 1.76 before round 3 (1,178 of the 4,096 greedy games repeat a move that
    changes nothing on a full board and are cut at 1,024 moves with the score they had): a difference of 94.0 = 41 standard errors
    of the difference (2.29).  Without symmetry the same rehearsal gives 172.18, 187.86, 187.18, 196.67 (DESIGN.md section 12.1;
    reported, not asserted).  The assertion asks for five standard errors."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    a = OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), 4096, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 20, max_steps=1024, seed=0,
                                   symmetric=True)
    mean, se = [], []
    for _ in range(4):
        e = a.evaluate(epsilon=0.0)
        mean.append(e["mean_score"])
        se.append(e["std_score"] / np.sqrt(e["games"]))
        print("evaluate before round", a.round, {k: e[k] for k in ("mean_score", "std_score", "max_score", "mean_length", "truncated", "coverage")}, e["max_tile_hist"])
        a.learn_batch()
    assert a.stats()["dropped"] == 0
    assert mean[3] - mean[0] >= 5.0 * np.hypot(se[0], se[3]), (mean, se)
