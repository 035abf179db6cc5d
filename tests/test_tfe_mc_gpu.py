"""On-policy first-visit Monte-Carlo control for 2048 on the device (csrc/tfe_mc.hip, agents/tfe_on_policy_mc_gpu.py) against the
host's statement of it (tests/tfe_host.py: the oracle's environment and Philox under the kernel's policy rule;
learn_on_host / greedy_on_host) and against the reference's dict-based class.  Every buffer the launches are handed sits between
guard words, and the rows of keys / steps at and beyond a game's length must keep what they held."""
import functools
import random

import numpy as np
import pytest

from tests.tfe_gpu_support import PATTERNS, assert_rollout, guard, guards_intact, read, replay, rollout

pytestmark = pytest.mark.gpu

BUFFERS = ("entries", "keys", "steps", "lengths", "total_score", "episode_reward", "counters")
BATCHES = (1, 63, 64, 65, 257)       # one lane, a wavefront less one, a whole one, one more, more than one workgroup and ragged


def _agent(n_games, n=3, **kw):
    """The agent with every device buffer re-seated between guard words; keys / steps pre-filled with a pattern."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    kw.setdefault("capacity", 1 << 16)
    kw.setdefault("max_steps", 256)
    a = guard(OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), n_games, board_size=n, **kw), BUFFERS, **PATTERNS)
    assert a.entries.data_ptr() % 128 == 0
    return a


def _host_rollout(a, table, **kw):
    from tests.tfe_host import rollout_on_host
    return rollout_on_host(a.n_games, a.n, a.max_steps, a.epsilon, table, a.env_seed, a.agent_seed, a.tie_seed, a.round_board_id0(), a.round, **kw)


@functools.lru_cache(maxsize=None)
def _four_rounds(n, n_games):
    """Four rounds on the device and on the host, once per (n, B): per round the device's and the host's roll-out and table."""
    a = _agent(n_games, n, seed=100 * n + n_games, board_id0=7)
    table, rounds, steps = {}, [], 0
    for _ in range(4):
        want = _host_rollout(a, table)
        got = rollout(a)
        a.learn()
        from pulselib_amd.agents.tfe_on_policy_mc_gpu import learn_on_host
        learn_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, table)
        steps += int(want["lengths"].sum())
        rounds.append(dict(got=got, want=want, table=a.table(), host_table={k: (list(c), list(s)) for k, (c, s) in table.items()},
                           stats=a.stats(), steps=steps))
        a.round += 1
    guards_intact(a)
    return rounds


@pytest.mark.parametrize("n", [3, 2])
@pytest.mark.parametrize("n_games", BATCHES)
def test_rollout_equals_the_host_word_for_word(n, n_games):
    """Round 0 runs on an empty table (the uniform default policy); round 3 on the table of three earlier rounds."""
    rounds = _four_rounds(n, n_games)
    for r, rec in enumerate(rounds):
        assert_rollout(rec["got"], rec["want"], (n, n_games, r))
        assert rec["stats"]["steps"] == rec["steps"] and rec["stats"]["truncated"] == 0
    assert rounds[0]["want"]["present"] == 0
    if n_games >= 63:                                                      # the present-entry and the tie paths ran
        assert rounds[3]["want"]["present"] > 0 and rounds[3]["want"]["tie_draws"] > 0


@pytest.mark.parametrize("n", [3, 2])
@pytest.mark.parametrize("n_games", BATCHES)
def test_learn_equals_the_host_as_a_map(n, n_games):
    """exact integers: the adds commute"""
    for r, rec in enumerate(_four_rounds(n, n_games)):
        assert rec["table"] == rec["host_table"], (n, n_games, r)
        assert rec["stats"]["first_visits"] == sum(sum(c) for c, _ in rec["table"].values()) and rec["stats"]["dropped"] == 0
    assert len(rec["table"]) > 4 and (n_games < 63 or max(max(c) for c, _ in rec["table"].values()) > 1)


def test_games_are_the_environments_own():
    """TFEBatch (pulse_tfe_reset / pulse_tfe_step) replayed with the recorded actions visits the recorded states"""
    from tests.tfe_host import pack_boards
    a = _agent(65, 3, seed=21, board_id0=1000)
    a.learn_batch().learn_batch()                                          # the second round's games: under a table, other board ids
    a.round -= 1
    got = read(a)

    def recorded_state(t, live, boards, actions):
        assert np.array_equal(pack_boards(boards)[live], got["keys"][t][live]), t
        return actions
    assert replay(a, got, recorded_state)[2].all()                         # every game ends where the environment says
    guards_intact(a)


def test_one_game_per_round_against_the_cpu_class():
    """B = 1 for 200 rounds: the policy improves after every game, as the reference's does.  The CPU class is fed the episodes read
    back; each contribution is rounded to 2^-frac_bits, so every q agrees within 2^-frac_bits."""
    from pulselib_amd.agents import OnPolicyFirstVisitMC
    a = _agent(1, 3, seed=9, max_steps=512)
    random.seed(1)
    cpu = OnPolicyFirstVisitMC(a.gamma, a.epsilon, n_actions=4)
    for _ in range(200):
        a.learn_batch()
        (episode,) = a.episodes()
        cpu.learn([((k,), act, r) for k, act, r in episode])
    q, table = a.q(), a.table()
    assert {(k, act) for k, (c, _) in table.items() for act in range(4) if c[act]} == set(cpu.returns) and len(cpu.returns) > 1000
    for (k, act), (_, count) in cpu.returns.items():
        assert table[k][0][act] == count
        assert abs(q[(k, act)] - cpu.q[(k, act)]) <= 2.0 ** -a.frac_bits, (k, act)
    assert a.stats()["truncated"] == 0 and a.stats()["dropped"] == 0
    guards_intact(a)


def test_truncation_at_max_steps():
    """max_steps = 8: cut games are counted, lengths are capped, the learner starts G at 0 from the cut, and row 8 does not exist:
    the guard words behind row 7 stay."""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import learn_on_host
    a = _agent(257, 3, seed=4, max_steps=8)
    table, cut = {}, 0
    for r in range(2):
        want = _host_rollout(a, table)
        got = rollout(a)
        assert_rollout(got, want, r)
        cut += want["truncated"]
        assert got["keys"].shape[0] == 8 and got["lengths"].max() == 8 and want["truncated"] > 100
        a.learn()
        learn_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, table)
        assert a.table() == table
        a.round += 1
        assert a.stats()["truncated"] == cut
    guards_intact(a)


def test_a_full_table_drops_and_ends():
    """capacity = 16 under 257 games: first visits are dropped and counted, the launch ends, nothing outside the table is written,
    and what is stored is right: a key enters at its first contribution or never, so every stored entry holds all of its key's."""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import learn_on_host
    a = _agent(257, 3, seed=6, capacity=16)
    want = _host_rollout(a, {})
    assert_rollout(rollout(a), want, 0)
    a.learn()
    a.round += 1
    host = learn_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, {})
    table, stats = a.table(), a.stats()
    assert len(table) == 16 and len(host) > 16 and stats["dropped"] > 0
    assert table == {k: host[k] for k in table}
    total = sum(sum(c) for c, _ in host.values())
    assert stats["first_visits"] == sum(sum(c) for c, _ in table.values()) and stats["first_visits"] + stats["dropped"] == total
    want = _host_rollout(a, table)                                         # the roll-out against a table without a free slot
    assert_rollout(rollout(a), want, 1)
    # ... and one that is sure to meet its entries.  Which 16 keys were placed is a race among the learner's lanes -- each wavefront
    # starts at its games' last moves -- and round 1's boards pass through few such states (on the host: no lookup of theirs hits
    # under most outcomes of the race).  Round 0's own games do: the game that placed a key plays as before up to the first entry met.
    a.round = 0
    want = _host_rollout(a, table)
    assert_rollout(rollout(a), want, 2)
    assert want["present"] > 0
    guards_intact(a)


def test_same_seeds_same_result_and_clear():
    a = _agent(257, 3, seed=12)

    def three_rounds():
        out = []
        for _ in range(3):
            a.learn_batch()
            got = read(a)
            played = np.arange(a.max_steps)[:, None] < got["lengths"][None, :]
            out.append((got["keys"][played].tobytes(), got["steps"][played].tobytes(), got["lengths"].tobytes(), got["total_score"].tobytes()))
        return out, a.table(), a.stats()

    first = three_rounds()
    a.clear()
    assert a.table() == {} and a.round == 0 and set(a.stats().values()) == {0}
    assert first == three_rounds() and len(first[1]) > 1000
    guards_intact(a)


def test_four_by_four_smoke():
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import learn_on_host
    a = _agent(64, 4, seed=3, max_steps=64)
    table = {}
    for r in range(2):
        want = _host_rollout(a, table)
        assert_rollout(rollout(a), want, r)
        a.learn()
        learn_on_host(want["keys"], want["steps"], want["lengths"], a.gamma, a.frac_bits, table)
        assert a.table() == table
        a.round += 1
    assert a.stats()["truncated"] > 0 and max(table) >= 1 << 36               # cut games; keys that use the upper cells
    guards_intact(a)


def test_it_learns():
    """B = 4,096 games of 3 x 3 per round, four rounds, gamma .9, epsilon .1, seed 0.  Rehearsed on the CPU with the host mirror
    (the same games: the table is the same map): mean final score 172.14 +- 1.46 in round 0 (the uniform policy), 191.80 +- 1.48,
    199.52 +- 1.52 and 206.87 +- 1.53 in round 3: a difference of 34.7 = 16 standard errors of the difference (2.12).  The
    assertion asks for five."""
    import torch
    from pulselib_amd.agents import OnPolicyFirstVisitMCTFEGPU
    a = OnPolicyFirstVisitMCTFEGPU(torch.device("cuda:0"), 4096, board_size=3, gamma=.9, epsilon=.1, capacity=1 << 20, max_steps=1024, seed=0)
    scores = []
    for _ in range(4):
        a.learn_batch()
        scores.append(a.total_score.cpu().numpy().astype(np.float64))
    mean = [s.mean() for s in scores]
    se = [s.std(ddof=1) / np.sqrt(s.size) for s in scores]
    print("mean final score per round", mean, "standard errors", se)
    assert a.stats()["dropped"] == 0 and a.stats()["truncated"] == 0
    assert mean[3] - mean[0] >= 5.0 * np.hypot(se[0], se[3]), (mean, se)
