"""2048 Monte-Carlo control on afterstates on the device (csrc/tfe_mc.hip: pulse_tfe_mc_rollout_after,
_after_canon, pulse_tfe_mc_learn_after, pulse_tfe_mc_evaluate_after, pulse_tfe_mc_table_fold_after) against the host's statement of
it (tests/tfe_host.py: the oracle's environment and Philox under greedy_after_on_host; learn_after_on_host,
fold_values_on_host) and the environment's own kernels.  Every comparison is exact.  Every buffer a launch is handed sits between
guard words, and the rows of keys / steps at and beyond a game's length must keep what they held.

Shapes: 257 games (one full workgroup and one of one lane), max_steps 128, capacity 2^14; and capacity 2^8, where probes overflow and
first visits are dropped.  Three rounds per shape, played once and shared: the roll-out of round r runs on the DEVICE's table after
r learn launches, read back, so a roll-out is held to the mirror whatever the learner dropped; the learner is held to the host's
on the recorded games.  Which keys a full table stores is a race among lanes, but a key that found no room never finds any later
(slots are not freed), so a stored entry holds ALL of its key's returns: the stored part of the table is compared exactly."""
import functools

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guards_intact, replay, rollout

pytestmark = pytest.mark.gpu

GAMES, MAX_STEPS, ROOMY, TIGHT, ROUNDS = 257, 128, 1 << 14, 1 << 8, 3
BUFFERS = ("entries", "keys", "steps", "lengths", "total_score", "episode_reward", "counters")


def _host_rollout(a, table, **kw):
    from tests.tfe_host import rollout_after_on_host
    return rollout_after_on_host(a.n_games, a.n, a.max_steps, a.epsilon, a.gamma, a.frac_bits, table, a.env_seed, a.agent_seed, a.tie_seed,
                                 a.round_board_id0(), a.round, canonical=a.symmetric, **kw)


@functools.lru_cache(maxsize=None)
def _rounds(n, symmetric=False, capacity=ROOMY):
    """Three rounds on the device and on the host, once per shape: (the agent after them, per round a record)."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import learn_after_on_host
    a = guard(OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), GAMES, board_size=n, afterstate=True, symmetric=symmetric, capacity=capacity,
                                         max_steps=MAX_STEPS, seed=100 * n + 57, board_id0=7), BUFFERS, **PATTERNS)
    assert a.entries.data_ptr() % 128 == 0
    host, out, flags = {}, [], 0
    for _ in range(ROUNDS):
        policy = a.table()
        want = _host_rollout(a, policy, keep_boards="before")
        got = rollout(a)
        a.learn()
        learn_after_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, host)
        flags += int((want["steps"] >> 7).sum())
        out.append(dict(got=got, want=want, policy=policy, table=a.table(), host={k: (list(c), list(s)) for k, (c, s) in host.items()},
                        stats=a.stats(), flags=flags, board_id0=a.round_board_id0()))
        a.round += 1
    guards_intact(a)
    return a, out


@pytest.mark.parametrize("n,symmetric", [(2, False), (3, False), (4, False), (3, True)], ids=["2", "3", "4", "3-canon"])
def test_rollout_after_equals_the_host_word_for_word(n, symmetric):
    """keys, steps, lengths, scores and rewards: round 0 on an empty table, round 2 on the table after two learning rounds -- where
    the comparison itself must have met entries and drawn tie coins"""
    _, rounds = _rounds(n, symmetric)
    moves = 0
    for r, rec in enumerate(rounds):
        assert_rollout(rec["got"], rec["want"], (n, symmetric, r))
        moves += int(rec["want"]["lengths"].sum())
        assert rec["stats"]["steps"] == moves
    assert rounds[0]["want"]["present"] == 0 and rounds[0]["policy"] == {}
    assert rounds[2]["want"]["present"] > 0 and rounds[2]["want"]["tie_draws"] > 0 and rounds[2]["want"]["greedy"] > 0
    assert (rounds[2]["want"]["lengths"] > 1).all() and rounds[2]["stats"]["truncated"] == sum(rec["want"]["truncated"] for rec in rounds)
    if n == 4:
        assert max(rounds[2]["policy"]) >= 1 << 36                          # keys that use the upper cells


@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
def test_recorded_actions_replay_through_the_environment(symmetric):
    """TFEBatch (pulse_tfe_reset / pulse_tfe_step) with the same seed and board ids, stepped by the recorded actions, meets the boards
    whose move_on_host images pack to the recorded keys (to their canonical keys with `symmetric`), with the recorded rewards."""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import afterstates_on_host, unpack_steps
    a, rounds = _rounds(3, symmetric)
    got = rounds[2]["got"]
    rewards = unpack_steps(got["steps"])[1]

    def recorded_afterstate(t, live, boards, actions):
        for g in np.nonzero(live)[0].tolist():
            keys, rs = afterstates_on_host(boards[g], symmetric)
            assert keys[actions[g]] == int(got["keys"][t, g]) and rs[actions[g]] == int(rewards[t, g]), (t, g)
        return actions
    replay(a, got, recorded_afterstate, rounds[2]["board_id0"])


@pytest.mark.parametrize("n,symmetric,capacity", [(3, False, ROOMY), (3, True, ROOMY), (2, False, ROOMY), (4, False, ROOMY), (3, False, TIGHT),
                                                  (3, True, TIGHT)], ids=["3", "3-canon", "2", "4", "3-tight", "3-canon-tight"])
def test_learn_after_equals_the_host_as_a_map(n, symmetric, capacity):
    """Exact integers: the adds commute.  Only cnt[0] / sum[0] are written; added + dropped = the `first` flags of the games; what is
    stored is the host's entry of that key; and where nothing was dropped the whole table is the host's.  Rehearsed on the host: in
    2^14 slots n = 2 stores 331 afterstates in three rounds and n = 3 canonical 10,180, n = 3 plain 11,816 in two (15,995 in three: a
    load of .98, where a probe may run past its limit), so those rounds must drop nothing; n = 4 meets 25,507 in round 0 alone, and
    2^8 slots fill in round 0."""
    from tests.tfe_host import values_of
    _, rounds = _rounds(n, symmetric, capacity)
    for r, rec in enumerate(rounds):
        table, host, st = rec["table"], rec["host"], rec["stats"]
        values_of(table)                                                   # cnt[1..3] and sum[1..3] are 0 everywhere
        assert table == {k: host[k] for k in table}, (n, symmetric, capacity, r)
        assert st["first_visits"] + st["dropped"] == rec["flags"] and st["first_visits"] == sum(c[0] for c, _ in table.values())
        if capacity == ROOMY and r < {(2, False): 3, (3, True): 3, (3, False): 2}.get((n, symmetric), 0):
            assert st["dropped"] == 0, (n, symmetric, r)
        if st["dropped"] == 0:
            assert table == host, (n, symmetric, capacity, r)
    assert len(table) > 4 and max(c[0] for c, _ in table.values()) > 1
    if capacity == TIGHT:
        assert rounds[0]["stats"]["dropped"] > 0 and len(table) == TIGHT     # (the later roll-outs ran against a table without a free slot)


@functools.lru_cache(maxsize=None)
def _evaluation(symmetric):
    """round 3 of the shape's agent, rolled out and evaluated with equal seeds, round, epsilon and table; and the host's mirror of it"""
    a, _ = _rounds(3, symmetric)
    want = _host_rollout(a, a.table())
    got = rollout(a)
    ev = a.evaluate(epsilon=a.epsilon, board_id0=a.round_board_id0(), per_game=True)
    guards_intact(a)
    return a, got, want, ev


@pytest.mark.parametrize("symmetric", [False, True], ids=["plain", "canonical"])
def test_evaluate_after_plays_the_rollouts_games(symmetric):
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import EVAL_BINS, EVAL_SUMMARY
    from tests.tfe_host import eval_words
    a, got, want, ev = _evaluation(symmetric)
    assert_rollout(got, want, symmetric)
    assert np.array_equal(ev["total_score"], got["total_score"]) and np.array_equal(ev["lengths"], got["lengths"])
    words = eval_words(want["total_score"], want["lengths"], want["final_boards"], want["truncated"], want["present"], want["greedy"])
    assert [ev[k] for k in EVAL_SUMMARY] + ev["max_tile_hist"] == words and len(words) == len(EVAL_SUMMARY) + EVAL_BINS
    assert ev["games"] == GAMES and ev["moves"] == int(got["lengths"].sum()) and ev["score_sum"] == int(got["total_score"].sum())
    assert 0 < ev["moves_greedy"] < ev["moves_with_entry"] <= ev["moves"]
    greedy = a.evaluate(n_games=64)                                        # the defaults: epsilon 0, other boards, no arrays
    assert greedy["games"] == 64 and greedy["moves_greedy"] == greedy["moves_with_entry"] and "total_score" not in greedy


def test_fold_grow_checkpoint_and_refusals(tmp_path):
    """to_symmetric() on the learnt plain value table is fold_values_on_host exactly; grow() and save / load keep the map and the
    kind; the two kinds of table do not mix."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    a, rounds = _rounds(3)
    table = rounds[2]["table"]
    assert a.table() == table
    sym = a.to_symmetric()
    folded = mc.fold_values_on_host(table, 3)
    assert sym.afterstate and sym.symmetric and sym.table() == folded and len(folded) < len(table) and sym.round == a.round
    assert sym.merge_stats() == dict(live=len(table), placed=len(table), dropped=0)
    with pytest.raises(ValueError, match="already holds canonical"):
        sym.to_symmetric()
    path = tmp_path / "values.npz"
    a.save(path)
    assert mc.read_checkpoint(path)["afterstate"] is True
    dev = torch.device("cuda:0")
    b = OnPolicyFirstVisitMCTFEGPU.load(path, dev, capacity=1 << 15, afterstate=True)
    assert b.afterstate and not b.symmetric and b.round == a.round and b.capacity == 1 << 15 and b.table() == table
    assert b.grow(1 << 16).table() == table and b.capacity == 1 << 16 and b.occupancy() == len(table)
    assert b.v() == {k: mc.v_of_entry(e, b.frac_bits) for k, e in table.items()} and max(b.v().values()) > 0.0
    with pytest.raises(ValueError, match="afterstate values"):
        b.q()
    with pytest.raises(ValueError, match="holds afterstate values, not Q"):
        OnPolicyFirstVisitMCTFEGPU.load(path, dev, afterstate=False)
    q = OnPolicyFirstVisitMCTFEGPU(dev, 64, board_size=3, capacity=1 << 12, max_steps=MAX_STEPS, seed=a.seed)
    assert not q.afterstate
    with pytest.raises(ValueError, match=r"Q\(state, action\)"):
        q.v()
    for dst, src in ((q, b), (b, q), (q, sym)):
        with pytest.raises(ValueError, match="merge_from: the source holds"):
            dst.merge_from(src)
    qpath = tmp_path / "q.npz"
    q.learn_batch().save(qpath)
    assert mc.read_checkpoint(qpath)["afterstate"] is False and not OnPolicyFirstVisitMCTFEGPU.load(qpath, dev).afterstate
    with pytest.raises(ValueError, match=r"holds Q\(state, action\), not afterstate"):
        OnPolicyFirstVisitMCTFEGPU.load(qpath, dev, afterstate=True)
    sym.merge_from(b)                                                      # a plain value table into a symmetric one: folded on the way
    assert sym.table() == mc.merge_tables_on_host({k: (list(c), list(s)) for k, (c, s) in folded.items()}, folded)
    # greedy(): the host statement of the rule on boards, the rule the roll-out was held to above
    boards = rounds[2]["want"]["boards"][4][:16]                            # the boards before the fifth move
    want = [mc.greedy_after_on_host(x, table, a.gamma, a.frac_bits, a.tie_seed, 1)[0] for x in boards]
    assert a.greedy(boards, round=1) == want and any(w is not None for w in want)


def test_it_learns():
    """3 x 3, seed 0, 4,096 games per round, gamma .9, epsilon .1; the greedy policy (epsilon 0) evaluated on 2,048 games from reset.
    One round on afterstates beats the empty table (the uniform policy) by at least five standard errors of the difference, and
    beats one round of the default Q(state, action) agent with the same seeds by as much.  Rehearsed on the CPU with another tie
    coin: 169.3 +- 2.0 on the empty table, 241.7 +- 2.2 after one round (+72 +- 3), against 185.6 +- 3.1 for Q (+56 +- 3.8).  On an
    MI355X: 171.1 +- 2.1, 241.5 +- 2.3 and 186.1 +- 2.1."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    kw = dict(board_size=3, gamma=.9, epsilon=.1, capacity=1 << 20, max_steps=1024, seed=0)
    dev = torch.device("cuda:0")
    v, q = OnPolicyFirstVisitMCTFEGPU(dev, 4096, afterstate=True, **kw), OnPolicyFirstVisitMCTFEGPU(dev, 4096, **kw)
    empty = v.evaluate(n_games=2048)
    after, plain = v.learn_batch().evaluate(n_games=2048), q.learn_batch().evaluate(n_games=2048)
    se = lambda e: e["std_score"] / e["games"] ** .5
    print("greedy mean score on 2,048 games: empty table", empty["mean_score"], "+-", se(empty), "afterstate, one round", after["mean_score"], "+-",
          se(after), "Q(s, a), one round", plain["mean_score"], "+-", se(plain), "cut at max_steps", after["truncated"])
    # (a greedy game may repeat, to max_steps, a move that changes nothing on a full board; it keeps the score it had: after["truncated"])
    assert v.stats()["dropped"] == 0 and v.stats()["truncated"] == 0 and empty["moves_with_entry"] == 0
    assert after["mean_score"] - empty["mean_score"] >= 5.0 * np.hypot(se(after), se(empty)), (after["mean_score"], empty["mean_score"])
    assert after["mean_score"] - plain["mean_score"] >= 5.0 * np.hypot(se(after), se(plain)), (after["mean_score"], plain["mean_score"])
