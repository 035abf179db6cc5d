"""The host's roll-out of the n-tuple network's games (csrc/tfe_ntuple.hip: pulse_tfe_nt_rollout, pulse_tfe_nt_evaluate), for the tests:
the same games, played with the oracle's environment (oracle.tfe_reset / oracle.tfe_step) under the kernel's policy rule as the agent
module states it (greedy_nt_on_host), vectorised over the games, so that a device roll-out can be compared word for word.  A helper,
not a test."""
import numpy as np

from oracle import oracle as orc
from pulselib_amd.agents import tfe_ntuple_td_gpu as nt
from tests.tfe_mc_host import pack_boards


def rollout_nt_on_host(n_games, max_steps, epsilon, gamma, weights, tuples, symmetric, env_seed, agent_seed, tie_seed, board_id0, round,
                       boards0=None):
    """pulse_tfe_nt_rollout on the host.  Returns a dict: keys uint64[max_steps, B], values float64[max_steps, B] and steps
    uint8[max_steps, B] (zero at and beyond a game's length), lengths int32[B], total_score int64[B], episode_reward int32[B],
    final_boards int32[B, 4, 4], ended (games that were over), truncated (games cut: stopped without being over), capped (games
    stopped at a 32,768 tile) and greedy (moves not decided by the epsilon branch).  boards0: int32[B, 4, 4] to start from instead
    of the reset's boards."""
    B, n = int(n_games), 4
    eps_q24 = int(np.floor(epsilon * 2.0 ** 24))
    boards = np.zeros((B, n, n), dtype=np.int32)
    score = np.zeros(B, dtype=np.int64)
    rewards, dones = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.uint8)
    orc.tfe_reset(boards, score, n, env_seed, board_id0)
    if boards0 is not None:
        boards[:] = boards0
    ids = np.array([(int(board_id0) + g) & (2 ** 64 - 1) for g in range(B)], dtype=np.uint64)
    out = dict(keys=np.zeros((max_steps, B), dtype=np.uint64), values=np.zeros((max_steps, B), dtype=np.float64),
               steps=np.zeros((max_steps, B), dtype=np.uint8), lengths=np.zeros(B, dtype=np.int32), total_score=np.zeros(B, dtype=np.int64),
               episode_reward=np.zeros(B, dtype=np.int32), final_boards=boards.copy(), greedy=0)
    active, over, capped = np.ones(B, dtype=bool), np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for t in range(max_steps):
        live = np.nonzero(active)[0]
        if live.size == 0:
            break
        draws = nt.philox_many_on_host(agent_seed, ids[live], t)
        choice = nt.greedy_nt_on_host(pack_boards(boards[live]), weights, tuples, symmetric, gamma, tie_seed, round)
        assert (choice["action"] >= 0).all()                                 # a board that is not over has a candidate
        explore = (draws[:, 0] >> np.uint32(8)) < eps_q24
        a = np.where(explore, (draws[:, 1] >> np.uint32(30)).astype(np.int64), choice["action"])
        out["greedy"] += int((~explore).sum())
        rows = np.arange(live.size)
        actions = np.zeros(B, dtype=np.int64)
        actions[live] = a
        orc.tfe_step(boards, score, actions, rewards, dones, n, env_seed, t + 1, board_id0)
        assert np.array_equal(rewards[live], choice["rewards"][rows, a])      # the host move's reward is the environment's
        over[live], capped[live] = dones[live] != 0, boards[live].reshape(live.size, -1).max(axis=1) >= 32768
        out["keys"][t, live], out["values"][t, live] = choice["after"][rows, a], choice["values"][rows, a]
        out["steps"][t, live] = (a | (rewards[live].astype(np.int64) << 2) | (over[live].astype(np.int64) << 7)).astype(np.uint8)
        out["episode_reward"][live] += rewards[live]
        out["lengths"][live] = t + 1
        out["total_score"][live] = score[live]
        out["final_boards"][live] = boards[live]
        active &= ~over & ~capped
    out["ended"], out["truncated"], out["capped"] = int(over.sum()), int((~over).sum()), int(capped.sum())
    return out


def eval_words(r):
    """pulse_tfe_nt_evaluate's summary[8] + max_tile_hist[16] of the games of one rollout_nt_on_host dict, a list of 24 Python ints."""
    s = r["total_score"].astype(object)
    top = r["final_boards"].reshape(len(s), -1).max(axis=1)
    hist = np.bincount(np.minimum(np.floor(np.log2(top)).astype(np.int64), 15), minlength=16)
    return [len(s), int(r["lengths"].sum()), int(s.sum()), int((s * s).sum()), int(s.max()), r["truncated"], r["greedy"], r["capped"]] + hist.tolist()
