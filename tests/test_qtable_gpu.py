"""The tabular Q-learner's kernels (csrc/qtable.hip) where its other tests (the end of tests/test_envs_gpu.py) do not reach: 3 x 3
boards, regions without room, games that are over, the cell form of the fused 4 x 4 kernel, all against the host mirror
(tests/qtable_host.py: the cases and what they reach are held on the CPU by tests/test_qtable_cpu.py) -- and a shared table under
contention with a step size at which one lost or doubled update shows."""
import numpy as np
import pytest
import torch

from tests import qtable_host as qh
from tests import tfe_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ("three-calls", "fused")


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ private tables against the mirror
def _make(name):
    from pulselib_amd.agents import QLearningBatch
    from pulselib_amd.environments.TFE import TFEBatch
    n, B, slots, steps, board_id0 = qh.CASES[name]
    dev = torch.device(DEV)
    env = TFEBatch(dev, B, n, seed=qh.CFG["env_seed"], board_id0=board_id0)
    agent = QLearningBatch(dev, B, n, config={"ALPHA": qh.CFG["alpha"], "GAMMA": qh.CFG["gamma"], "EPSILON": qh.CFG["epsilon"]},
                           private_tables=True, slots=slots, seed=qh.CFG["agent_seed"], board_id0=board_id0)
    env.reset()
    return env, agent


def _regions(agent):
    """(keys uint64[B, slots], values as bit patterns uint64[B, slots, 4])"""
    B, slots = agent.batch_size, agent.region_slots
    return _np(agent.keys).view(np.uint64).reshape(B, slots), _np(agent.values).view(np.uint64).reshape(B, slots, 4)


def _step(form, agent, env, t):
    if form == "fused":
        agent.rollout_step(env, t)
    else:
        boards, rewards, dones, _, _ = env.step(agent.get_actions(env.boards, t))
        agent.update(boards, rewards, dones)


def _assert_step(form, agent, env, rec, t):
    """the step's actions, boards, rewards, done flags and scores are the mirror's; fused: the carried entry of every board is the row
    of the board it is on now, or negative where the mirror found no room for it"""
    for name, got in (("actions", agent.actions), ("boards", env.boards), ("rewards", env.rewards), ("dones", env.dones.view(torch.uint8)),
                      ("scores", env.total_score)):
        np.testing.assert_array_equal(_np(got), rec[name][t], err_msg=f"step {t} {name}")
    if form == "fused":
        B, slots = agent.batch_size, agent.region_slots
        carried, has_row = _np(agent.slots), rec["has_row"][t]
        np.testing.assert_array_equal(carried >= 0, has_row, err_msg=f"step {t}: boards with a row")
        assert (carried[~has_row] == -1).all()
        rows = carried[has_row]
        assert (rows // slots == np.arange(B)[has_row]).all(), f"step {t}: a carried entry outside its board's region"
        keys = _regions(agent)[0].reshape(-1)
        np.testing.assert_array_equal(keys[rows], tfe_host.pack_boards(rec["boards"][t])[has_row], err_msg=f"step {t}: carried entries")


def _assert_tables(agent, host):
    """every board's region: the mirror's keys, each once, and the mirror's values bit for bit"""
    keys, bits = _regions(agent)
    for g in range(agent.batch_size):
        used = keys[g] != 0
        got = dict(zip(keys[g][used].tolist(), bits[g][used]))
        assert len(got) == int(used.sum()), f"board {g}: a key in two entries"
        assert set(got) == set(host.tables[g]), f"board {g}: state sets differ"
        for k, q in host.tables[g].items():
            assert np.array_equal(got[k], q.view(np.uint64)), f"board {g} state {k:#x}: {got[k].view(np.float64)} != {q}"
        assert not bits[g][~used].any(), f"board {g}: values in a free entry"


def _play(name, form, before=None, between=None):
    host, rec = qh.run_case(name)
    env, agent = _make(name)
    if before is not None:
        before(env, agent)
    for t in range(qh.CASES[name][3]):
        _step(form, agent, env, t)
        _assert_step(form, agent, env, rec, t)
        if between is not None:
            between(t, env, agent)
    _assert_tables(agent, host)
    return agent


@pytest.mark.parametrize("form", FORMS)
def test_three_by_three_with_room_matches_the_mirror(form):
    """n = 3 (qtable_rollout_step_kernel<3>; cells = 9 in the select and update kernels), 200 boards -- a ragged workgroup and a
    ragged wavefront -- for 64 steps, in which 65 games end and go on being stepped: target = reward without the bootstrap."""
    _play("3x3-room", form)


@pytest.mark.parametrize("name", ["3x3-full", "3x3-full-id1000"])
@pytest.mark.parametrize("form", FORMS)
def test_three_by_three_without_room_matches_the_mirror(form, name):
    """16 slots per board: some 190 of the 200 regions fill up, after which a new state acts by its random draw and learns nothing,
    and a new s' counts as max q = 0 (rules a, b, c of tests/qtable_host.py); with board ids from 0 and from 1,000."""
    _play(name, form)


def test_three_by_three_drops_the_carried_entries_when_told():
    """the fused form halfway through a run: every second board is turned over behind the agent's back, forget_states() -- the
    mirror just goes on from the turned boards"""
    def flip(t, env, agent):
        if t == qh.FLIP_AFTER:
            env.boards[::2] = env.boards[::2].flip(1).contiguous()
            agent.forget_states()
    _play("3x3-flipped", "fused", between=flip)


_UNUSUAL = {}


def _unusual(form):
    """the 4 x 4 case under `form` (played once per form): the agent, after every check against the mirror"""
    if form not in _UNUSUAL:
        def start(env, agent):
            boards = qh.unusual_boards()
            env.boards.copy_(torch.from_numpy(boards))
            agent.forget_states()
            agent.get_actions(env.boards, 0)                        # inserts every board's first row (as the step itself would) ...
            row = int(agent.slots[qh.MERGER])
            assert int(agent.keys[row]) & (2 ** 64 - 1) == qh.pack_board(boards[qh.MERGER])
            agent.values[row, 0] = 1.0                              # ... so that MERGER's can be told to move left
            agent.forget_states()
        _UNUSUAL[form] = _play("4x4-unusual", form, before=start)
    return _UNUSUAL[form]


@pytest.mark.parametrize("form", FORMS)
def test_four_by_four_with_unusual_boards_matches_the_mirror(form):
    """Boards the packed 4 x 4 form cannot hold inside qtable_rollout_step_kernel<4>: a wavefront with one of them, a wavefront
    full of them, and a board that becomes one by merging 16,384s in the packed form (tests/test_qtable_cpu.py holds the layout).
    The wavefront then takes tfe_move<4> and pack_cells, and the key of s' must be the one the packed form would have given."""
    agent = _unusual(form)
    assert int(agent.keys.ne(0).sum()) == sum(len(t) for t in qh.run_case("4x4-unusual")[0].tables)


def test_four_by_four_with_unusual_boards_leaves_the_same_entries_in_both_forms():
    a, b = _unusual(FORMS[0]), _unusual(FORMS[1])
    assert torch.equal(a.entries, b.entries)


# ------------------------------------------------------------------ a shared table under contention, at a step size that shows a loss
def _contended(B, alpha, epsilon):
    """every board on one two-row state and the boards its move leads to, as test_shared_table_combines_simultaneous_updates_of_one_entry"""
    from pulselib_amd.agents import QLearningBatch
    dev = torch.device(DEV)
    agent = QLearningBatch(dev, B, 4, config={"ALPHA": alpha, "GAMMA": 0.0, "EPSILON": epsilon}, slots=1 << 12, seed=qh.SHARED_SEED)
    board = torch.tensor([[2, 4, 8, 16], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 2, 0]], dtype=torch.int32, device=dev)
    boards = board.repeat(B, 1, 1).contiguous()
    nxt = boards.clone(); nxt[:, 1, 1] = 2
    return agent, boards, nxt, torch.zeros(B, dtype=torch.bool, device=dev), qh.pack_board(_np(board)), qh.pack_board(_np(nxt[0]))


def _deferred(agent, launch):
    """transitions of launch number `launch` that lost their compare-and-swap: the segment lengths of its parity (pulse_env.h)"""
    W = -(-agent.batch_size // 256)
    return int(agent._scratch_tensors["count"][64 + (launch & 1) * W:64 + (launch & 1) * W + W].sum())


def _assert_scratch_clean(agent):
    t = agent._scratch_tensors
    assert int(t["acc_key"].ne(0).sum()) == 0 and int(t["acc_cnt"].ne(0).sum()) == 0 and int(t["acc_sum"].ne(0).sum()) == 0


@pytest.mark.parametrize("B,alpha", [(700, 2.0 ** -10), (1300, 2.0 ** -10), (66000, 2.0 ** -10), (66000, 2.0 ** -16)],
                         ids=["700", "1300", "66000", "66000-alpha-2^-16"])
def test_four_cells_of_one_entry_take_every_update_once(B, alpha):
    """All B boards in ONE state, random actions (epsilon = 1), reward = action + 1, gamma = 0: the four cells of one entry are
    contended at once, each by the k_a boards that drew a, all with the target a + 1.  Whatever mix of compare-and-swap winners and
    combined losers a cell saw, it must hold its k_a updates one after another, q + (1 - (1 - alpha)^k_a) (a + 1 - q), over three
    rounds, and the scratch must be clean after each.
    Tolerance, derived: an update is three rounded operations (t - q, alpha *, q +) on values of at most max(|t|, |q|), and every
    later update multiplies an earlier one's error by 1 - alpha < 1, so k updates are within 3 k 2^-53 max(|t|, |q0|) of the exact
    value; a few units more for the pow of the combined form and of the expected value: 4 k 2^-53 max(|t|, |q0|) per round, from the
    value the device held before the round; along the closed form from q = 0 the rounds' tolerances add up.  alpha = 2^-10 is exact,
    and one lost or doubled update moves a cell by alpha t (1 - alpha)^k, more than 10^4 tolerances at 700 and 1,300 boards; at 66,000
    boards (k = 16,500) it does so with alpha = 2^-16 only (tests/test_qtable_cpu.py has the figures), hence that size twice.
    700 boards: at most 1,024 deferred transitions, the follow-up launch's one-workgroup form, a ragged last workgroup; 1,300: more
    than 1,024, its 64 workgroups meet; 66,000: 258 segments, two per thread of the prefix sum, 208 live lanes in the last workgroup."""
    agent, boards, nxt, term, key, key_next = _contended(B, alpha, 1.0)
    chain, chain_tol, before = np.zeros(4), np.zeros(4), np.zeros(4)
    for rnd in range(3):
        acts = agent.get_actions(boards, rnd)
        if B <= 1300:
            np.testing.assert_array_equal(_np(acts), qh.random_actions(qh.SHARED_SEED, 0, B, rnd))
        rewards = (acts + 1).to(torch.int32)
        agent.update(nxt, rewards, term)
        counts = np.bincount(_np(acts), minlength=4)
        assert counts.sum() == B and counts.min() > B // 8
        deferred = _deferred(agent, rnd)
        print(f"B {B} round {rnd}: k = {counts.tolist()}, deferred {deferred}")
        # (a cell that has reached its fixed point, q + alpha (t - q) == q, loses no compare-and-swap: 66,000 boards, alpha = 2^-10, third round)
        if all(q + alpha * (a + 1.0 - q) != q for a, q in enumerate(before.tolist())):
            assert (0 < deferred <= 1024) if B == 700 else (1024 < deferred < B)
        tab = agent.table()
        assert set(tab) == {key, key_next} and not tab[key_next].any()
        got = tab[key]
        for a, k in enumerate(counts.tolist()):
            t = a + 1.0
            tol = qh.combined_tolerance(k, t, before[a])
            chain[a], chain_tol[a] = qh.combined(chain[a], t, k, alpha), chain_tol[a] + qh.combined_tolerance(k, t, chain[a])
            want = qh.combined(before[a], t, k, alpha)
            print(f"  cell {a}: got {got[a]!r}, want {want!r} (off by {abs(got[a] - want):.3g}, tolerance {tol:.3g}); from q = 0 {chain[a]!r}")
            assert abs(got[a] - want) <= tol, (rnd, a, k, got[a], want, tol)
            assert abs(got[a] - chain[a]) <= chain_tol[a], (rnd, a, k, got[a], chain[a], chain_tol[a])
        before = got.copy()
        _assert_scratch_clean(agent)


def test_rollout_step_on_a_shared_table_takes_every_update_once():
    """pulse_qtable_rollout_step on 1,300 boards right after a reset (a ragged last workgroup): they sit in 281 two-tile states, up
    to 15 in one; greedy on an empty table every board moves left and the boards of a state get the same reward, so a state's cell
    must hold t (1 - (1 - alpha)^k) -- part (ii) of test_fused_rollout_step_at_config3_size, with alpha = 2^-10 for which every
    state's k counts, to the derived tolerance 4 k 2^-53 t."""
    from pulselib_amd.agents import QLearningBatch
    from pulselib_amd.environments.TFE import TFEBatch
    B, alpha = 1300, 2.0 ** -10
    dev = torch.device(DEV)
    env = TFEBatch(dev, B, 4, seed=5)
    agent = QLearningBatch(dev, B, 4, config={"ALPHA": alpha, "GAMMA": 0.0, "EPSILON": 0.0}, slots=1 << 12, seed=3)
    env.reset()
    keys = tfe_host.pack_boards(_np(env.boards))
    _, rew, _, _, _ = agent.rollout_step(env, 0)
    assert int(agent.actions.abs().max()) == 0
    rew = _np(rew).astype(np.float64)
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    target = np.zeros(len(uniq)); target[inverse] = rew
    assert np.array_equal(target[inverse], rew)                                   # the same for every board of a state
    assert len(uniq) > 200 and counts.max() >= 10 and int((target > 0).sum()) >= 15 and int(counts[target > 0].sum()) >= 150
    deferred = _deferred(agent, 0)
    print(f"{len(uniq)} states, k up to {counts.max()}, {int((target > 0).sum())} with a reward; deferred {deferred}")
    assert deferred > 0
    table = agent.table()
    assert set(table) == set(uniq.tolist()) | set(tfe_host.pack_boards(_np(env.boards)).tolist())
    for key, k, t in zip(uniq.tolist(), counts.tolist(), target.tolist()):
        got, want = table.pop(key), qh.combined(0.0, t, k, alpha)
        assert abs(got[0] - want) <= qh.combined_tolerance(k, t, 0.0) and got[1] == got[2] == got[3] == 0.0, (hex(key), k, t, got, want)
    assert all(not q.any() for q in table.values())                               # states only reached: rows without a value
    _assert_scratch_clean(agent)


def test_unequal_targets_in_one_cell_combine_by_their_mean():
    """Every update deferred (the scratch's diagnostic reserved0 = 1: no compare-and-swap), 1,300 boards in one state, greedy, so
    one cell takes all of them, with rewards 1 + (g mod 7): the combined update is the k transitions with the MEAN of their targets,
    q0 + (1 - (1 - alpha)^B) (mean - q0).  The sum of the integer targets is exact, so the derived tolerance of the equal-target test
    holds, with max |t| = 7.  Two rounds."""
    B, alpha = 1300, 2.0 ** -10
    agent, boards, nxt, term, key, key_next = _contended(B, alpha, 0.0)
    rewards = (1 + torch.arange(B, device=boards.device) % 7).to(torch.int32)
    mean = float(_np(rewards).astype(np.int64).sum()) / B
    agent._scratch.reserved0 = 1
    try:
        q0 = 0.0
        for rnd in range(2):
            acts = agent.get_actions(boards, rnd)
            assert int(acts.abs().max()) == 0
            agent.update(nxt, rewards, term)
            assert _deferred(agent, rnd) == B
            tab = agent.table()
            assert set(tab) == {key, key_next} and not tab[key_next].any()
            got, want, tol = tab[key], qh.combined(q0, mean, B, alpha), qh.combined_tolerance(B, 7.0, q0)
            print(f"round {rnd}: got {got[0]!r}, want {want!r} (off by {abs(got[0] - want):.3g}, tolerance {tol:.3g})")
            assert abs(got[0] - want) <= tol and got[1] == got[2] == got[3] == 0.0, (rnd, got, want, tol)
            _assert_scratch_clean(agent)
            q0 = float(got[0])
    finally:
        agent._scratch.reserved0 = 0
