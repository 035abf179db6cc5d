"""The host's side of the 2048 agents (csrc/tfe_mc.hip, csrc/tfe_ntuple.hip), for the tests: ONE game loop on the oracle's environment
(oracle.tfe_reset / oracle.tfe_step) and a policy per roll-out kernel -- the Q table plain or canonical and the afterstate table here,
the n-tuple network's in tests/tfe_nt_host.py -- each under the kernel's rule as the agent modules state it, so that a device roll-out
can be compared word for word; the keys of many boards at once, the oracle's move without its spawn, and an evaluation's 24 counters
as numpy reductions.  A helper, not a test."""
import functools

import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc

MOVE_SEED = 0x5EED
ACTION_MAP, ACTION_UNMAP = np.array(mc.ACTION_MAP, dtype=np.int64), np.array(mc.ACTION_UNMAP, dtype=np.int64)


def philox_many(seed, subseqs, offset):
    """uint32[len(subseqs), 4]: oracle.philox4x32(seed, s, offset) for every s"""
    return np.stack([orc.philox4x32(int(seed), int(s), int(offset)) for s in subseqs]) if len(subseqs) else np.zeros((0, 4), np.uint32)


# ------------------------------------------------------------------ keys of many boards
def _logs(boards):
    cells = boards.reshape(boards.shape[0], -1).astype(np.int64)
    return np.where(cells > 0, np.minimum(np.floor(np.log2(np.maximum(cells, 1))).astype(np.int64), 15), 0).astype(np.uint64)


def _pack(logs, src):
    """uint64[B]: nibble i of key b is logs[b, src[i]]"""
    key = np.zeros(logs.shape[0], dtype=np.uint64)
    for i, s in enumerate(src):
        key |= logs[:, s] << np.uint64(4 * i)
    return key


def _canon(logs, n):
    images = np.stack([_pack(logs, src) for src in mc.transforms_on_host(n).tolist()], axis=1)
    return images.min(axis=1), images.argmin(axis=1)                      # (argmin: the first, so the smallest, j)


def pack_boards(boards):
    """uint64[B]: the state keys of int32[B, n, n] boards"""
    logs = _logs(boards)
    return _pack(logs, range(logs.shape[1]))


def canon_many(boards):
    """(key_c uint64[B], j* int64[B]) of int32[B, n, n] boards: mc.canon_on_host for every board, in numpy."""
    return _canon(_logs(boards), boards.shape[-1])


def canon_keys(keys, n):
    """(key_c, j*) of an array of state keys, in its shape: mc.canon_key_on_host for every key, in numpy."""
    keys = np.asarray(keys, dtype=np.uint64)
    key_c, j = _canon(np.stack([(keys.ravel() >> np.uint64(4 * i)) & np.uint64(15) for i in range(n * n)], axis=1), n)
    return key_c.reshape(keys.shape), j.reshape(keys.shape)


# ------------------------------------------------------------------ the oracle's move without its spawn
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


# ------------------------------------------------------------------ the policies
class _Policy:
    """What differs between the roll-outs.  Per move the game loop calls choose(t, ids, live, boards) with the live games' board ids,
    indices and boards and gets (the recorded key, the recorded action, the action the board moves by, the reward the policy expects
    or None, the recorded value or None); once the environment has stepped it calls flag(live, keys, actions, over) for bit 7 of the
    per-move byte.  The epsilon branch and the counters are here: `present` the moves that found an entry, `greedy` the moves decided
    greedily, `tie_draws` the greedy scans that drew coins -- what a comparison exercised."""
    philox_many, counters = staticmethod(philox_many), ("present", "greedy", "tie_draws")

    def __init__(self, n_games, epsilon, agent_seed, tie_seed, round, **rest):
        self.eps_q24, self.agent_seed, self.tie_seed, self.round = int(np.floor(epsilon * 2.0 ** 24)), agent_seed, tie_seed, round
        self.__dict__.update(rest)
        self.counts = dict.fromkeys(self.counters, 0)
        self.prev, self.taken = np.zeros(int(n_games), dtype=np.uint64), np.zeros(int(n_games), dtype=np.int64)

    def coins(self, seed, key, r):
        self.counts["tie_draws"] += 1
        return philox_many(seed, [key], r)[0]

    def branch(self, t, ids, present=None):
        """(greedy bool[live]: an entry, where the policy has entries, and not the epsilon branch; the uniform action int64[live])"""
        draws = self.philox_many(self.agent_seed, ids, t)
        greedy = (draws[:, 0] >> 8) >= self.eps_q24
        if present is not None:
            self.counts["present"] += int(present.sum())
            greedy &= present
        self.counts["greedy"] += int(greedy.sum())
        return greedy, (draws[:, 1] >> 30).astype(np.int64)


class _QTable(_Policy):
    """pulse_tfe_mc_rollout / _canon: Q(state, action) of {key: (cnt[4], sum[4])}; bit 7 is the run mask over unchanged keys"""
    def choose(self, t, ids, live, boards):
        keys, js = canon_many(boards) if self.canonical else (pack_boards(boards), np.zeros(live.size, dtype=np.int64))
        entries = [self.table.get(k) for k in keys.tolist()]
        greedy, uniform = self.branch(t, ids, np.array([e is not None for e in entries]))
        actions = ACTION_MAP[js, uniform]                                  # in the frame of `keys`
        for i in np.nonzero(greedy)[0].tolist():
            actions[i] = mc.greedy_on_host(entries[i], int(keys[i]), self.tie_seed, self.round, self.coins)
        return keys, actions, ACTION_UNMAP[js, actions], None, None

    def flag(self, live, keys, actions, over):
        taken = np.where(keys != self.prev[live], 0, self.taken[live])      # four bits per game: the actions taken on this key
        self.prev[live], self.taken[live] = keys, taken | 1 << actions
        return ((taken >> actions) & 1) == 0


class _AfterTable(_Policy):
    """pulse_tfe_mc_rollout_after / _after_canon: V(afterstate) of {key: (cnt[4], sum[4])}; bit 7 is a change of the key"""
    def choose(self, t, ids, live, boards):
        looks = [mc.greedy_after_on_host(b, self.table, self.gamma, self.frac_bits, self.tie_seed, self.round, self.canonical, self.coins) for b in boards]
        greedy, uniform = self.branch(t, ids, np.array([a is not None for a, _, _ in looks]))
        actions = np.where(greedy, np.array([0 if a is None else a for a, _, _ in looks], dtype=np.int64), uniform)
        rows = np.arange(live.size)
        keys, rewards = np.array([k for _, k, _ in looks], dtype=np.uint64), np.array([r for _, _, r in looks], dtype=np.int64)
        return keys[rows, actions], actions, actions, rewards[rows, actions], None

    def flag(self, live, keys, actions, over):
        first = keys != self.prev[live]                                    # (no afterstate of a live board packs to 0: true at t = 0)
        self.prev[live] = keys
        return first


# ------------------------------------------------------------------ the game loop
def _play(policy, n_games, n, max_steps, env_seed, board_id0, boards0=None, keep_boards=None, tile_cap=None):
    """The games of one roll-out launch under `policy`.  Returns a dict: keys uint64[max_steps, B], steps uint8[max_steps, B] and moved
    int64[max_steps, B], the action the board moved by (zero at and beyond a game's length; values float64[max_steps, B] too where the
    policy gives them), lengths int32[B], total_score int64[B], episode_reward int32[B], final_boards int32[B, n, n], ended (games
    that were over), truncated (games cut: stopped without being over), capped (games stopped at a `tile_cap` tile), the policy's
    counters, and boards: with keep_boards "before" / "after" the int32[B, n, n] boards before / after every move.  boards0:
    int32[B, n, n] to start from instead of the reset's boards."""
    assert keep_boards in (None, "before", "after")
    B = int(n_games)
    boards, score = np.zeros((B, n, n), dtype=np.int32), np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, env_seed, board_id0)
    if boards0 is not None:
        boards[:] = boards0
    ids = np.array([(int(board_id0) + g) & (2 ** 64 - 1) for g in range(B)], dtype=np.uint64)
    out = dict(keys=np.zeros((max_steps, B), dtype=np.uint64), steps=np.zeros((max_steps, B), dtype=np.uint8),
               moved=np.zeros((max_steps, B), dtype=np.int64), lengths=np.zeros(B, dtype=np.int32), total_score=np.zeros(B, dtype=np.int64),
               episode_reward=np.zeros(B, dtype=np.int32), final_boards=boards.copy(), boards=[])
    over, capped = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for t in range(max_steps):
        live = np.nonzero(~over & ~capped)[0]
        if live.size == 0:
            break
        if keep_boards == "before":
            out["boards"].append(boards.copy())
        keys, recorded, moved, expected, values = policy.choose(t, ids[live], live, boards[live])
        actions = np.zeros(B, dtype=np.int64)
        actions[live] = moved
        orc.tfe_step(boards, score, actions, rewards, dones, n, env_seed, t + 1, board_id0)
        assert expected is None or np.array_equal(rewards[live], expected)   # the host move's reward is the environment's
        over[live] = dones[live] != 0
        if tile_cap is not None:
            capped[live] = boards[live].reshape(live.size, -1).max(axis=1) >= tile_cap
        first = policy.flag(live, keys, recorded, over[live])
        out["keys"][t, live], out["moved"][t, live] = keys, moved
        if values is not None:
            out.setdefault("values", np.zeros((max_steps, B), dtype=np.float64))[t, live] = values
        out["steps"][t, live] = (recorded | (rewards[live].astype(np.int64) << 2) | (first.astype(np.int64) << 7)).astype(np.uint8)
        out["episode_reward"][live] += rewards[live]
        out["lengths"][live] = t + 1
        out["total_score"][live] = score[live]
        out["final_boards"][live] = boards[live]
        if keep_boards == "after":
            out["boards"].append(boards.copy())
    return dict(out, ended=int(over.sum()), truncated=int((~over).sum()), capped=int(capped.sum()), **policy.counts)


def rollout_on_host(n_games, n, max_steps, epsilon, table, env_seed, agent_seed, tie_seed, board_id0, round, canonical=False, keep_boards=None):
    """pulse_tfe_mc_rollout (canonical False) or pulse_tfe_mc_rollout_canon on the host, keys / steps in the frame asked for.  table:
    {key: (cnt[4], sum[4])}, read only; an empty one gives the uniform default policy."""
    policy = _QTable(n_games, epsilon, agent_seed, tie_seed, round, table=table, canonical=canonical)
    return _play(policy, n_games, n, max_steps, env_seed, board_id0, keep_boards=keep_boards)


def rollout_after_on_host(n_games, n, max_steps, epsilon, gamma, frac_bits, table, env_seed, agent_seed, tie_seed, board_id0, round,
                          canonical=False, keep_boards=None):
    """pulse_tfe_mc_rollout_after (canonical False) or pulse_tfe_mc_rollout_after_canon on the host.  table as rollout_on_host's;
    `present` counts the moves where one of the four afterstates had an entry."""
    policy = _AfterTable(n_games, epsilon, agent_seed, tie_seed, round, table=table, canonical=canonical, gamma=gamma, frac_bits=frac_bits)
    return _play(policy, n_games, n, max_steps, env_seed, board_id0, keep_boards=keep_boards)


def values_of(table):
    """{key: (cnt[0], sum[0])} of a value table, after checking that the other six words of every entry are 0"""
    assert all(c[1:] == [0, 0, 0] and s[1:] == [0, 0, 0] for c, s in table.values())
    return {k: (c[0], s[0]) for k, (c, s) in table.items()}


def eval_words(total_score, lengths, final_boards, *words):
    """An evaluation launch's summary[8] + max_tile_hist[16] as numpy reductions, a list of 24 Python ints.  words: the three counters
    of summary[5..7] -- truncated, present, greedy for pulse_tfe_mc_evaluate(_after), truncated, greedy, capped for pulse_tfe_nt_evaluate."""
    s = np.asarray(total_score).astype(object)
    top = np.asarray(final_boards).reshape(len(s), -1).max(axis=1)
    hist = np.bincount(np.minimum(np.floor(np.log2(top)).astype(np.int64), 15), minlength=16)
    assert len(words) == 3
    return [len(s), int(np.asarray(lengths).sum()), int(s.sum()), int((s * s).sum()), int(s.max())] + [int(w) for w in words] + hist.tolist()
