"""The host's side of the 2048 Monte-Carlo symmetries and evaluation launch (csrc/tfe_mc.hip: pulse_tfe_mc_rollout_canon,
pulse_tfe_mc_evaluate), for the tests: the oracle's move without its spawn, the canonical keys of many boards at once, the
roll-out of either frame played with the oracle's environment and Philox, and the evaluation's 24 counters as numpy reductions.
A helper, not a test."""
import functools

import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
from tests.tfe_mc_host import pack_boards, philox_many

MOVE_SEED = 0x5EED


@functools.lru_cache(maxsize=None)
def _spawn_counters():
    """Two step counters of board 0 under MOVE_SEED whose spawn draw picks the FIRST and the LAST empty cell whatever their number
    (<= 16): cell k = (r_cell * empty) >> 32 is 0 for r_cell < 2^28 and empty - 1 for r_cell >= 15 * 2^28."""
    lo = next(c for c in range(1, 4096) if int(orc.philox4x32(MOVE_SEED, 0, c)[0]) < 1 << 28)
    hi = next(c for c in range(1, 4096) if int(orc.philox4x32(MOVE_SEED, 0, c)[0]) >= 15 << 28)
    return lo, hi


def _oracle_step(board, a, counter):
    n = board.shape[-1]
    b = np.ascontiguousarray(board, dtype=np.int32).reshape(1, n, n).copy()
    score, rewards, dones = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint8)
    orc.tfe_step(b, score, np.array([a], dtype=np.int64), rewards, dones, n, MOVE_SEED, counter, 0)
    return b[0], int(score[0])


def move_on_host(board, a):
    """(board, merge score, spawned) of move `a` by the oracle's step (the move, then a spawn while a cell is empty), stepped twice
    with spawns into the first and into the last empty cell.  With two or more empty cells after the move the two spawns differ and
    the cell-wise minimum is the moved board BEFORE the spawn (spawned False).  With one, both steps fill it with the same tile (one
    draw decides 2 or 4): the board comes back full, AFTER that spawn, and spawned is True.  With none there is no spawn."""
    lo, hi = _spawn_counters()
    x, score = _oracle_step(board, a, lo)
    y, score_y = _oracle_step(board, a, hi)
    assert score == score_y
    if (x != 0).all():                                                     # no or one empty cell after the move
        return x, score, int(x.sum()) != int(np.asarray(board).sum())
    return np.minimum(x, y), score, False


def _canon_logs(logs, n):
    images = np.zeros((logs.shape[0], 8), dtype=np.uint64)
    for j, src in enumerate(mc.transforms_on_host(n)):
        for i, s in enumerate(src.tolist()):
            images[:, j] |= logs[:, s] << np.uint64(4 * i)
    return images.min(axis=1), images.argmin(axis=1)                      # (argmin: the first, so the smallest, j)


def canon_many(boards):
    """(key_c uint64[B], j* int64[B]) of int32[B, n, n] boards: mc.canon_on_host for every board, in numpy."""
    B, n = boards.shape[0], boards.shape[-1]
    cells = boards.reshape(B, -1).astype(np.int64)
    logs = np.where(cells > 0, np.minimum(np.floor(np.log2(np.maximum(cells, 1))).astype(np.int64), 15), 0).astype(np.uint64)
    return _canon_logs(logs, n)


def canon_keys(keys, n):
    """(key_c, j*) of an array of state keys, in its shape: mc.canon_key_on_host for every key, in numpy."""
    keys = np.asarray(keys, dtype=np.uint64)
    logs = np.stack([(keys.ravel() >> np.uint64(4 * i)) & np.uint64(15) for i in range(n * n)], axis=1)
    key_c, j = _canon_logs(logs, n)
    return key_c.reshape(keys.shape), j.reshape(keys.shape)


ACTION_MAP, ACTION_UNMAP = np.array(mc.ACTION_MAP, dtype=np.int64), np.array(mc.ACTION_UNMAP, dtype=np.int64)


def rollout_on_host(n_games, n, max_steps, epsilon, table, env_seed, agent_seed, tie_seed, board_id0, round, canonical=False):
    """pulse_tfe_mc_rollout (canonical False) or pulse_tfe_mc_rollout_canon on the host.  table: {key: (cnt[4], sum[4])}, read only.
    Returns what tests/tfe_mc_host.rollout_on_host returns (keys / steps in the frame asked for) and: moved int64[max_steps, B] the
    action the board moved by, final_boards int32[B, n, n], greedy = the moves decided greedily."""
    B = int(n_games)
    eps_q24 = int(np.floor(epsilon * 2.0 ** 24))
    boards = np.zeros((B, n, n), dtype=np.int32)
    score = np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, env_seed, board_id0)
    ids = np.array([(int(board_id0) + g) & (2 ** 64 - 1) for g in range(B)], dtype=np.uint64)
    out = dict(keys=np.zeros((max_steps, B), dtype=np.uint64), steps=np.zeros((max_steps, B), dtype=np.uint8),
               moved=np.zeros((max_steps, B), dtype=np.int64), lengths=np.zeros(B, dtype=np.int32), total_score=np.zeros(B, dtype=np.int64),
               episode_reward=np.zeros(B, dtype=np.int32), final_boards=np.zeros((B, n, n), dtype=np.int32), present=0, greedy=0, tie_draws=0)
    active = np.ones(B, dtype=bool)
    prev, taken = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.int64)

    def coins(seed, key, r):
        out["tie_draws"] += 1
        return philox_many(seed, [key], r)[0]
    for t in range(max_steps):
        live = np.nonzero(active)[0]
        if live.size == 0:
            break
        keys, js = canon_many(boards) if canonical else (pack_boards(boards), np.zeros(B, dtype=np.int64))
        draws = philox_many(agent_seed, ids[live], t)
        actions = np.zeros(B, dtype=np.int64)                              # in the frame of `keys`
        for g, (x, y) in zip(live.tolist(), draws[:, :2].tolist()):
            entry = table.get(int(keys[g]))
            out["present"] += entry is not None
            if entry is None or (x >> 8) < eps_q24:
                actions[g] = ACTION_MAP[js[g], y >> 30]
            else:
                out["greedy"] += 1
                actions[g] = mc.greedy_on_host(entry, int(keys[g]), tie_seed, round, coins)
        moved = ACTION_UNMAP[js, actions]
        taken[keys != prev] = 0
        prev = keys
        first = ((taken >> actions) & 1) == 0
        taken |= 1 << actions
        orc.tfe_step(boards, score, moved, rewards, dones, n, env_seed, t + 1, board_id0)
        out["keys"][t, live] = keys[live]
        out["steps"][t, live] = (actions[live] | (rewards[live].astype(np.int64) << 2) | (first[live].astype(np.int64) << 7)).astype(np.uint8)
        out["moved"][t, live] = moved[live]
        out["episode_reward"][live] += rewards[live]
        out["lengths"][live] = t + 1
        out["total_score"][live] = score[live]
        out["final_boards"][live] = boards[live]
        active &= dones == 0
    out["truncated"] = int(active.sum())
    return out


def eval_words(total_score, lengths, final_boards, truncated, present, greedy):
    """pulse_tfe_mc_evaluate's summary[8] + max_tile_hist[16] of one launch as numpy reductions, a list of 24 Python ints."""
    s = np.asarray(total_score).astype(object)
    top = np.asarray(final_boards).reshape(len(s), -1).max(axis=1)
    hist = np.bincount(np.minimum(np.floor(np.log2(top)).astype(np.int64), 15), minlength=16)
    return [len(s), int(np.asarray(lengths).sum()), int(s.sum()), int((s * s).sum()), int(s.max()), int(truncated), int(present), int(greedy)] + hist.tolist()
