"""The host's roll-out of the 2048 Monte-Carlo games on afterstates (csrc/tfe_mc.hip: pulse_tfe_mc_rollout_after,
pulse_tfe_mc_rollout_after_canon, pulse_tfe_mc_evaluate_after), for the tests: the same games, played with the oracle's environment
and Philox under the kernel's policy rule as the agent module states it (greedy_after_on_host), so that a device roll-out can be
compared word for word.  A helper, not a test."""
import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
from tests.tfe_mc_host import philox_many


def rollout_after_on_host(n_games, n, max_steps, epsilon, gamma, frac_bits, table, env_seed, agent_seed, tie_seed, board_id0, round,
                          canonical=False, keep_boards=False):
    """pulse_tfe_mc_rollout_after (canonical False) or pulse_tfe_mc_rollout_after_canon on the host.  table: {key: (cnt[4], sum[4])},
    read only.  Returns a dict: keys uint64[max_steps, B] and steps uint8[max_steps, B] (zero at and beyond a game's length), lengths
    int32[B], total_score int64[B], episode_reward int32[B], final_boards int32[B, n, n], truncated (games cut at max_steps), present
    (moves where one of the four keys had an entry), greedy (moves decided greedily), tie_draws (greedy scans that drew coins) and,
    with keep_boards, boards: the int32[B, n, n] boards BEFORE every move."""
    B = int(n_games)
    eps_q24 = int(np.floor(epsilon * 2.0 ** 24))
    boards = np.zeros((B, n, n), dtype=np.int32)
    score = np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, env_seed, board_id0)
    ids = np.array([(int(board_id0) + g) & (2 ** 64 - 1) for g in range(B)], dtype=np.uint64)
    out = dict(keys=np.zeros((max_steps, B), dtype=np.uint64), steps=np.zeros((max_steps, B), dtype=np.uint8),
               lengths=np.zeros(B, dtype=np.int32), total_score=np.zeros(B, dtype=np.int64), episode_reward=np.zeros(B, dtype=np.int32),
               final_boards=np.zeros((B, n, n), dtype=np.int32), present=0, greedy=0, tie_draws=0, boards=[])
    active = np.ones(B, dtype=bool)
    prev = np.zeros(B, dtype=np.uint64)

    def coins(seed, key, r):
        out["tie_draws"] += 1
        return philox_many(seed, [key], r)[0]
    for t in range(max_steps):
        live = np.nonzero(active)[0]
        if live.size == 0:
            break
        if keep_boards:
            out["boards"].append(boards.copy())
        draws = philox_many(agent_seed, ids[live], t)
        actions, keys, want = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.int32)
        for g, (x, y) in zip(live.tolist(), draws[:, :2].tolist()):
            a, ka, ra = mc.greedy_after_on_host(boards[g], table, gamma, frac_bits, tie_seed, round, canonical, coins)
            out["present"] += a is not None
            if a is None or (x >> 8) < eps_q24:
                a = y >> 30
            else:
                out["greedy"] += 1
            actions[g], keys[g], want[g] = a, ka[a], ra[a]
        first = keys != prev                                              # (no afterstate of a live board packs to 0: true at t = 0)
        prev = keys
        orc.tfe_step(boards, score, actions, rewards, dones, n, env_seed, t + 1, board_id0)
        assert np.array_equal(rewards[live], want[live])                    # the host move's reward is the environment's
        out["keys"][t, live] = keys[live]
        out["steps"][t, live] = (actions[live] | (rewards[live].astype(np.int64) << 2) | (first[live].astype(np.int64) << 7)).astype(np.uint8)
        out["episode_reward"][live] += rewards[live]
        out["lengths"][live] = t + 1
        out["total_score"][live] = score[live]
        out["final_boards"][live] = boards[live]
        active &= dones == 0
    out["truncated"] = int(active.sum())
    return out


def values_of(table):
    """{key: (cnt[0], sum[0])} of a value table, after checking that the other six words of every entry are 0"""
    assert all(c[1:] == [0, 0, 0] and s[1:] == [0, 0, 0] for c, s in table.values())
    return {k: (c[0], s[0]) for k, (c, s) in table.items()}
