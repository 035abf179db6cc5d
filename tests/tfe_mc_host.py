"""The host's roll-out of the 2048 Monte-Carlo games (csrc/tfe_mc.hip: pulse_tfe_mc_rollout), for the tests: the same games,
played with the oracle's environment (oracle.tfe_reset / oracle.tfe_step) and the oracle's Philox under the kernel's policy rule,
so that a device roll-out can be compared word for word.  A helper, not a test."""
import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc


def philox_many(seed, subseqs, offset):
    """uint32[len(subseqs), 4]: oracle.philox4x32(seed, s, offset) for every s"""
    return np.stack([orc.philox4x32(int(seed), int(s), int(offset)) for s in subseqs]) if len(subseqs) else np.zeros((0, 4), np.uint32)


def pack_boards(boards):
    """uint64[B]: the state keys of int32[B, n, n] boards"""
    cells = boards.reshape(boards.shape[0], -1).astype(np.int64)
    logs = np.where(cells > 0, np.minimum(np.floor(np.log2(np.maximum(cells, 1))).astype(np.int64), 15), 0).astype(np.uint64)
    key = np.zeros(boards.shape[0], dtype=np.uint64)
    for i in range(cells.shape[1]):
        key |= logs[:, i] << np.uint64(4 * i)
    return key


def rollout_on_host(n_games, n, max_steps, epsilon, table, env_seed, agent_seed, tie_seed, board_id0, round, philox_many=philox_many,
                    keep_boards=False):
    """pulse_tfe_mc_rollout on the host.  table: {key: (cnt[4], sum[4])}, read only.  Returns a dict: keys uint64[max_steps, B] and
    steps uint8[max_steps, B] (zero at and beyond a game's length), lengths int32[B], total_score int64[B], episode_reward int32[B],
    truncated (the number of games cut at max_steps) and, with keep_boards, boards: the int32[B, n, n] boards after every move."""
    B = int(n_games)
    eps_q24 = int(np.floor(epsilon * 2.0 ** 24))
    boards = np.zeros((B, n, n), dtype=np.int32)
    score = np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, env_seed, board_id0)
    ids = board_id0 + np.arange(B, dtype=np.uint64)
    out = dict(keys=np.zeros((max_steps, B), dtype=np.uint64), steps=np.zeros((max_steps, B), dtype=np.uint8),
               lengths=np.zeros(B, dtype=np.int32), total_score=np.zeros(B, dtype=np.int64), episode_reward=np.zeros(B, dtype=np.int32),
               boards=[])
    active = np.ones(B, dtype=bool)
    prev, taken = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.int64)
    out["present"] = out["tie_draws"] = 0          # moves that found an entry / greedy scans that drew coins: what a comparison exercised

    def coins(seed, key, r):
        out["tie_draws"] += 1
        return philox_many(seed, [key], r)[0]
    for t in range(max_steps):
        live = np.nonzero(active)[0]
        if live.size == 0:
            break
        keys = pack_boards(boards)
        draws = philox_many(agent_seed, ids[live], t)
        actions = np.zeros(B, dtype=np.int64)
        for g, (x, y) in zip(live.tolist(), draws[:, :2].tolist()):
            entry = table.get(int(keys[g]))
            out["present"] += entry is not None
            if entry is None or (x >> 8) < eps_q24:
                actions[g] = y >> 30
            else:
                actions[g] = mc.greedy_on_host(entry, int(keys[g]), tie_seed, round, coins)
        taken[keys != prev] = 0
        prev = keys
        first = ((taken >> actions) & 1) == 0
        taken |= 1 << actions
        orc.tfe_step(boards, score, actions, rewards, dones, n, env_seed, t + 1, board_id0)
        out["keys"][t, live] = keys[live]
        out["steps"][t, live] = (actions[live] | (rewards[live].astype(np.int64) << 2) | (first[live].astype(np.int64) << 7)).astype(np.uint8)
        out["episode_reward"][live] += rewards[live]
        out["lengths"][live] = t + 1
        out["total_score"][live] = score[live]
        if keep_boards:
            out["boards"].append(boards.copy())
        active &= dones == 0
    out["truncated"] = int(active.sum())
    return out
