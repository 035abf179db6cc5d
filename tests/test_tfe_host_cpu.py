"""The unified host roll-out (tests/tfe_host.py, and under the n-tuple network's policy tests/tfe_nt_host.py) held to what the four roll-outs it replaced returned, as recorded from them: a digest
of the arrays a device roll-out is compared with, and the counts.  The digest: the first 16 hex digits of SHA-256 over the C-contiguous
bytes of keys, (values,) steps, lengths, total_score, episode_reward (, final_boards)."""
import hashlib

import numpy as np
import pytest

MC = ("keys", "steps", "lengths", "total_score", "episode_reward")
NT = ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "final_boards")
DTYPES = dict(keys=np.uint64, values=np.float64, steps=np.uint8, lengths=np.int32, total_score=np.int64, episode_reward=np.int32, final_boards=np.int32)


def _digest(o, names):
    h = hashlib.sha256()
    for k in names:
        assert o[k].dtype == DTYPES[k], k
        h.update(np.ascontiguousarray(o[k]).tobytes())
    return h.hexdigest()[:16]


# per round: digest, moves, score sum, present, greedy, tie draws, truncated
MC_PINS = {
    ("plain", False): [("7ace85e5240cf330", 1364, 7264, 0, 0, 0, 3), ("1d11d845fefa6276", 1300, 6524, 62, 59, 29, 0)],
    ("plain", True): [("eb30474ace013999", 1364, 7264, 0, 0, 0, 3), ("58bcaf2143be01d0", 1495, 8068, 240, 219, 68, 0)],
    ("afterstate", False): [("625e82057df58ffc", 1364, 7264, 0, 0, 0, 3), ("1f1ae7f1fad5042e", 1255, 6076, 297, 266, 54, 0)],
    ("afterstate", True): [("f3dd8ad59e4f3e30", 1364, 7264, 0, 0, 0, 3), ("d341e548453282bd", 1353, 6916, 594, 532, 274, 2)],
}


@pytest.mark.parametrize("kind,canonical", list(MC_PINS), ids=lambda v: {True: "canonical", False: "own-frame"}.get(v, v))
def test_monte_carlo_rollouts_are_the_recorded_ones(kind, canonical):
    """40 games of 3 x 3, max_steps 64, epsilon .1, seed 8; round 0 on an empty table, round 1 on the table learnt from round 0"""
    from pulselib_amd.agents import tfe_on_policy_mc_gpu as mc
    from tests.tfe_host import rollout_after_on_host, rollout_on_host
    fb, table = mc.frac_bits_for(0.9, 64), {}
    for r, want in enumerate(MC_PINS[kind, canonical]):
        seeds = (8, 8 ^ mc.AGENT_KEY, 8 ^ mc.TIE_KEY, 3 + 40 * r, r)
        if kind == "plain":
            o = rollout_on_host(40, 3, 64, 0.1, table, *seeds, canonical=canonical)
            mc.learn_on_host(o["keys"], o["steps"], o["lengths"], 0.9, fb, table)
        else:
            o = rollout_after_on_host(40, 3, 64, 0.1, 0.9, fb, table, *seeds, canonical=canonical)
            mc.learn_after_on_host(o["keys"], o["steps"], o["lengths"], 0.9, fb, table)
        got = (_digest(o, MC), int(o["lengths"].sum()), int(o["total_score"].sum()), o["present"], o["greedy"], o["tie_draws"], o["truncated"])
        assert got == want, (kind, canonical, r)
        assert (o["ended"], o["capped"]) == (40 - o["truncated"], 0)


PATTERN = lambda: (np.arange(16 ** 4 + 16 ** 6) % 7).astype(np.float32)
#          weights, symmetric, max_steps, round: digest, moves, score sum, greedy, ended, truncated, capped
NT_PINS = [(lambda: np.zeros(16 ** 4 + 16 ** 6, dtype=np.float32), True, 48, 0, ("aa3902b2ab1b1293", 768, 5468, 565, 0, 16, 0)),
           (PATTERN, True, 400, 1, ("6500c88b28958b41", 1727, 15104, 1293, 16, 0, 0)),
           (PATTERN, False, 400, 1, ("b308db3b43756e54", 2030, 19116, 1513, 16, 0, 0))]


@pytest.mark.parametrize("weights,symmetric,max_steps,round,want", NT_PINS, ids=["zeros", "pattern", "pattern-plain"])
def test_ntuple_rollouts_are_the_recorded_ones(weights, symmetric, max_steps, round, want):
    """16 games, the tuples (0, 1, 2, 3) and (4, 5, 6, 8, 9, 10), epsilon .25, gamma 1, seed 8, board_id0 3"""
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import AGENT_KEY, TIE_KEY
    from tests.tfe_nt_host import nt_games_on_host
    o = nt_games_on_host(16, max_steps, 0.25, 1.0, weights(), ((0, 1, 2, 3), (4, 5, 6, 8, 9, 10)), symmetric, 8, 8 ^ AGENT_KEY, 8 ^ TIE_KEY, 3, round)
    assert (_digest(o, NT), int(o["lengths"].sum()), int(o["total_score"].sum()), o["greedy"], o["ended"], o["truncated"], o["capped"]) == want
