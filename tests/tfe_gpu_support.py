"""What the 2048 GPU tests share: device buffers re-seated between guard words, a roll-out launch read back in full and held to the
host's (tests/tfe_host.py) word for word, and the recorded games replayed through the environment's own kernels.  Each test file
keeps its shapes, seeds and the list of buffers it guards.  A helper, not a test."""
import numpy as np

GUARD_BYTES, GUARD_FILL = 256, 0x77      # a multiple of the table's 128-byte alignment
PATTERNS = dict(keys=0x5A5A5A5A5A5A5A5A, steps=0xEE, values=-12345.678)     # what the per-move rows hold before the first launch
PER_GAME = ("lengths", "total_score", "episode_reward")


def guarded(t, fill=None):
    """(the tensor re-seated between guard words, the whole allocation, the guard's length in elements); it keeps its contents, or
    holds `fill`"""
    import torch
    g = GUARD_BYTES // t.element_size()
    flat = torch.empty(t.numel() + 2 * g, dtype=t.dtype, device=t.device)
    flat.view(torch.uint8).fill_(GUARD_FILL)
    inner = flat[g:g + t.numel()].view(t.shape)
    if fill is None:
        inner.copy_(t)
    else:
        inner.fill_(fill)
    return inner, flat, g


def guard(a, names, fill=0, **fills):
    """The buffers `names` of an agent re-seated between guard words and listed in its `_guards`: each holds fills[name], else `fill`
    (None: its contents)."""
    a.__dict__.setdefault("_guards", [])
    for name in names:
        inner, flat, g = guarded(getattr(a, name), fills.get(name, fill))
        setattr(a, name, inner)
        a._guards.append((name, flat, g))
    return a


def guards_intact(*guards):
    """of agents (their `_guards`) or of lists of (name, allocation, guard length)"""
    import torch
    for entry in guards:
        for name, flat, g in getattr(entry, "_guards", entry):
            b, gb = flat.view(torch.uint8), g * flat.element_size()
            assert bool((b[:gb] == GUARD_FILL).all()) and bool((b[-gb:] == GUARD_FILL).all()), f"guard words of {name} were written"


def read(a, per_move=("keys", "steps")):
    """the last roll-out's buffers in full (not trimmed to the longest game); keys, and values, as uint64 bit patterns"""
    out = {k: getattr(a, k).cpu().numpy() for k in per_move + PER_GAME}
    return {k: v.view(np.uint64) if k in ("keys", "values") else v for k, v in out.items()}


def rollout(a, per_move=("keys", "steps")):
    """one roll-out launch; the read-back carries what the per-move rows held before it (the pattern, or an earlier round's rows)"""
    before = read(a, per_move)
    a.rollout()
    return dict(read(a, per_move), **{k + "_before": before[k] for k in per_move})


def assert_rollout(got, want, where, per_move=("keys", "steps")):
    """word for word (values as bit patterns); at and beyond a game's length the rows hold what they held before the launch"""
    L = want["lengths"]
    assert np.array_equal(got["lengths"], L), where
    played = np.arange(got["keys"].shape[0])[:, None] < L[None, :]
    for k in per_move:
        host = want[k].view(np.uint64) if k == "values" else want[k]
        assert np.array_equal(got[k][played], host[played]), (where, k)
        assert np.array_equal(got[k][~played], got[k + "_before"][~played]), (where, k)
    assert np.array_equal(got["total_score"], want["total_score"]) and np.array_equal(got["episode_reward"], want["episode_reward"]), where


def replay(a, got, check, board_id0=None):
    """The recorded games of `got` through TFEBatch (pulse_tfe_reset / pulse_tfe_step) with the agent's seed and the round's board ids
    (`board_id0`: another round's).  Per move check(t, live, boards, actions) is handed the environment's boards before the move and
    the recorded actions, asserts what the records say of them and returns the actions the boards move by.  Here: the environment
    gives the recorded rewards, no game is done before its last move, and the final scores are the recorded ones.  Returns (final
    boards int32[B, n, n], final scores int64[B], done bool[B]: the environment ended the game at its last move)."""
    import torch
    from pulselib_amd.agents.tfe_on_policy_mc_gpu import unpack_steps
    from pulselib_amd.environments.TFE.TFE import TFEBatch
    B, L = a.n_games, got["lengths"]
    actions, rewards, _ = unpack_steps(got["steps"])
    env = TFEBatch(a.device, B, a.n, seed=a.env_seed, board_id0=a.round_board_id0() if board_id0 is None else board_id0)
    boards, _ = env.reset()
    final, score, done = np.zeros((B, a.n, a.n), dtype=np.int32), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    for t in range(int(L.max())):
        live, ends = L > t, L == t + 1
        moved = np.where(live, check(t, live, boards.cpu().numpy(), actions[t].astype(np.int64)), 0).astype(np.int64)
        boards, rew, dones, _, info = env.step(torch.from_numpy(moved).to(a.device))
        dones = dones.cpu().numpy() != 0
        assert np.array_equal(rew.cpu().numpy()[live], rewards[t][live].astype(np.int32)), t
        assert not dones[live & ~ends].any(), t
        final[ends], score[ends], done[ends] = boards.cpu().numpy()[ends], info["score"].cpu().numpy()[ends], dones[ends]
    assert np.array_equal(score, got["total_score"])
    return final, score, done
