"""The 2048 n-tuple network's training roll-out at the adaptive search depth, on the device (DESIGN.md section 13.13;
csrc/tfe_ntuple_search_rollout.hip: pulse_tfe_nt_rollout_adaptive) against the host's statement of it
(tests/tfe_nt_host.py: the oracle's environment under search_adaptive_nt_on_host, recording V of the chosen afterstate
and search_backed_on_host of the q), against the two-layer recording launches at E = 16, and through the agent: whole rounds with
backed targets, games continued across rounds and restarted rounds.  Every comparison is exact: integers word for word, float64 and
float32 as bit patterns.  Every buffer a launch is handed sits between guard words -- `backed`, `start` and `depth_stats` too -- and
the rows of keys / values / steps / backed at and beyond a game's length must keep what they held.

Shape (tests/tfe_nt_adaptive_support.py, where the rehearsals are written down): the tuples (0, 1, 2,
3) and (4, 5, 6, 8, 9, 10), weights all zero or a seeded normal array of scale 4, gamma 1, 7 games of at most 256 moves, one workgroup
each, E = 3.  The host's games are played once per case and shared (about 2 s per case)."""
import numpy as np
import pytest

from tests.tfe_continue_host import Carried, pick_on_host
from tests.tfe_gpu_support import assert_rollout, guard, guards_intact, read
from tests.tfe_nt_adaptive_support import (CASES, DEEP_EMPTY_MAX, EPSILON, FROM_CASE, FROM_REHEARSED, GAMES, MAX_STEPS, SEED, UNUSABLE, host_rollout, host_rollout_from,
                                           start_boards)
from tests.tfe_nt_host import nt_games_on_host
from tests.tfe_nt_support import PER_MOVE, TUPLES, bits, nt, search_agent

pytestmark = pytest.mark.gpu

E = DEEP_EMPTY_MAX
ENTRY = "pulse_tfe_nt_rollout_adaptive"
BACKED_PATTERN, DELTAS_PATTERN = -4321.125, 777.0625                       # what `backed` and `deltas` hold before the first launch
PER_GAME = ("lengths", "total_score", "episode_reward")
LEARNER_STATE = ("deltas", "acc_abs", "E", "A", "tc_stats")


def _agent(name="seeded", symmetric=True, epsilon=EPSILON, games=GAMES, max_steps=MAX_STEPS, start=None, continued=False, **kw):
    """the agent of the shape with every device buffer between guard words: `backed` (a pattern), `start` (`start`, or zeros),
    `depth_stats` (zeros) and what a learner holds too; continued: the carries and `finished` as well"""
    import torch
    a = search_agent(games, max_steps, SEED, name, symmetric, epsilon=epsilon, **kw)
    a.backed, a.depth_stats = torch.zeros_like(a.values), torch.zeros(2, dtype=torch.int64, device=a.device)
    if a.deltas is None:
        a.deltas = torch.zeros_like(a.values)
    a._continue_state() if continued else a._restart_state()
    names = ("backed", "start", "restart_stats", "depth_stats") + tuple(k for k in LEARNER_STATE if getattr(a, k) is not None)
    names += ("carry_score", "carry_moves", "finished") if continued else ()
    a = guard(a, names, backed=BACKED_PATTERN, deltas=DELTAS_PATTERN)
    if start is not None:
        a.start.copy_(torch.from_numpy(np.array(start, dtype=np.uint64).view(np.int64)))
    assert all(getattr(a, k).data_ptr() % 8 == 0 for k in ("backed", "start", "depth_stats"))
    return a


def _start_of(a):
    return a.start.cpu().numpy().view(np.uint64)


def _read(a):
    return dict(read(a, PER_MOVE), backed=bits(a.backed.cpu().numpy()))


def _launched(a, launch):
    """`launch` on the agent; the read-back carries what the per-move rows held before it, the counters' differences and the depth
    words' differences"""
    before, st, depth = _read(a), a.stats(), a.depth_stats.cpu().tolist()
    launch()
    after, now = a.stats(), a.depth_stats.cpu().tolist()
    return dict(_read(a), **{k + "_before": before[k] for k in PER_MOVE + ("backed",)}, **{k: after[k] - st[k] for k in ("moves", "truncated")},
                depth=[x - y for x, y in zip(now, depth)])


def _assert_games(a, got, want, where, backed):
    """keys, values as bit patterns, step bytes, lengths, scores, episode rewards, the two stats words, the moves at each depth and,
    with `backed`, its rows of every recorded move; without it `backed` keeps what it held"""
    assert_rollout(got, want, where, PER_MOVE)
    played = np.arange(got["backed"].shape[0])[:, None] < want["lengths"][None, :]
    if backed:
        assert np.array_equal(got["backed"][played], bits(want["backed"])[played]), where
        assert np.array_equal(got["backed"][~played], got["backed_before"][~played]), where      # (on zero weights every game is cut: no such row)
    else:
        assert np.array_equal(got["backed"], got["backed_before"]), where
    assert got["moves"] == int(want["lengths"].sum()) and got["truncated"] == want["truncated"], where
    assert got["depth"] == [want["deep"], want["shallow"]] and sum(got["depth"]) == got["moves"], where
    guards_intact(a)


def _same_records(x, y, keys=PER_MOVE + PER_GAME + ("backed", "moves", "truncated", "depth")):
    for k in keys:
        assert np.array_equal(x[k], y[k]), k


# ------------------------------------------------------------------ the games, word for word
@pytest.mark.parametrize("name,epsilon,symmetric", CASES)
def test_records_equal_the_mirrors(name, epsilon, symmetric):
    """one agent, two launches of the same round: without `backed` (the buffer keeps its pattern), then with it"""
    want = host_rollout(name, epsilon, symmetric)
    assert want["deep"] >= 5 and want["shallow"] >= 5 and want["capped"] == 0
    assert name != "seeded" or (want["ended"] >= 1 and want["truncated"] >= 1)
    a = _agent(name, symmetric, epsilon)
    got = _launched(a, lambda: a.rollout_adaptive_launch(E))
    _assert_games(a, got, want, (name, epsilon, symmetric, "plain"), False)
    assert (got["backed"] == bits(np.float64(BACKED_PATTERN))).all()
    assert a.rollout_depth_summary() == dict(moves_deep=want["deep"], moves_shallow=want["shallow"]) and not a.depth_stats.any().item()
    got = _launched(a, lambda: a.rollout_adaptive_launch(E, backed=True))
    _assert_games(a, got, want, (name, epsilon, symmetric, "backed"), True)
    assert np.isfinite(want["backed"]).all() and (name == "zero" or want["backed"].any())
    assert not a.start.any().item()                                        # never handed to the launch


def test_sixteen_is_the_two_layer_recording_launches():
    """device against device, every record: 7 games capped at 96 moves, where two layers on every board stay affordable"""
    agents = [_agent(max_steps=96) for _ in range(4)]
    mine, search, mine_b, backed = agents
    got = [_launched(mine, lambda: mine.rollout_adaptive_launch(16)), _launched(search, lambda: search.rollout_search_launch(2)),
           _launched(mine_b, lambda: mine_b.rollout_adaptive_launch(16, backed=True)), _launched(backed, lambda: backed.rollout_backed_launch(2))]
    skip_depth = PER_MOVE + PER_GAME + ("backed", "moves", "truncated")
    _same_records(got[0], got[1], skip_depth)
    _same_records(got[2], got[3], skip_depth)
    _same_records(got[0], got[2], PER_MOVE + PER_GAME)
    assert got[0]["depth"] == got[2]["depth"] == [got[1]["moves"], 0] and got[1]["depth"] == got[3]["depth"] == [0, 0]
    assert got[1]["moves"] > GAMES and int(got[1]["lengths"].max()) == 96
    assert (got[0]["backed"] == bits(np.float64(BACKED_PATTERN))).all() and not (got[2]["backed"] == bits(np.float64(BACKED_PATTERN))).all()
    guards_intact(*agents)


# ------------------------------------------------------------------ from `start`
def test_the_games_from_start_are_the_mirrors():
    """four late boards and the three kinds of unusable entry (tests/tfe_nt_adaptive_support.py): the unusable ones fall back to the
    reset and read 0 afterwards, the usable ones are unchanged"""
    name, epsilon, symmetric = FROM_CASE
    start, want = start_boards(), host_rollout_from()
    left = want["start_left"]
    assert {k: (want[k].tolist() if k == "lengths" else want[k]) for k in FROM_REHEARSED} == FROM_REHEARSED
    assert want["deep"] >= 5 and want["shallow"] >= 5 and want["ended"] >= 1 and want["truncated"] >= 1
    unusable = np.isin(np.arange(GAMES), list(UNUSABLE))
    assert (left[unusable] == 0).all() and np.array_equal(left[~unusable], start[~unusable]) and (start[~unusable] != 0).all()
    assert np.count_nonzero(start[unusable]) == 2                          # (the dead board and the one with nibble 15; the third is 0)
    a = _agent(name, symmetric, epsilon, start=start)
    got = _launched(a, lambda: a.rollout_adaptive_launch(E, backed=True, from_start=True))
    _assert_games(a, got, want, "from start", True)
    assert np.array_equal(_start_of(a), left)
    reset = host_rollout(name, epsilon, symmetric)
    for g in UNUSABLE:                                                     # the games at their resets are the case's own
        assert np.array_equal(got["keys"][:, g][:reset["lengths"][g]], reset["keys"][:, g][:reset["lengths"][g]]), g
    assert not np.array_equal(got["keys"][0], reset["keys"][0])


def test_a_start_of_zeros_is_the_launch_without_start():
    a, b = _agent(), _agent()
    mine, null = _launched(a, lambda: a.rollout_adaptive_launch(E, from_start=True)), _launched(b, lambda: b.rollout_adaptive_launch(E))
    _same_records(mine, null)
    assert not a.start.any().item() and mine["moves"] > GAMES
    guards_intact(a, b)


# ------------------------------------------------------------------ the depth words
def test_a_null_depth_stats_leaves_the_records_equal():
    """one direct launch with depth_stats = NULL beside the agent's own call; the launch alone adds and never zeroes"""
    a, b = _agent(), _agent()
    mine = _launched(a, lambda: a.rollout_adaptive_launch(E, backed=True))
    null = _launched(b, lambda: b._launch(ENTRY, b._rollout_struct(), E, b.backed.data_ptr(), None, None))
    _same_records(mine, null, PER_MOVE + PER_GAME + ("backed", "moves", "truncated"))
    assert null["depth"] == [0, 0] and not b.depth_stats.any().item() and mine["depth"][0] > 0 and mine["depth"][1] > 0
    a.rollout_adaptive_launch(E)
    assert a.depth_stats.cpu().tolist() == [2 * d for d in mine["depth"]]
    assert a.rollout_depth_summary(clear=False) == dict(moves_deep=2 * mine["depth"][0], moves_shallow=2 * mine["depth"][1])
    assert a.depth_stats.cpu().tolist() == [2 * d for d in mine["depth"]]
    guards_intact(a, b)


# ------------------------------------------------------------------ whole rounds through the agent
def _set(a, **attributes):
    for k, v in attributes.items():
        setattr(a, k, v)
    return a


def _host_learn(n, a, games, policy, coherence):
    """the host's learner and apply on `games` under the agent's options: (acc before the apply, acc_abs or None, counts, weights after)"""
    host_acc = np.zeros((a.n_weights, 2), dtype=np.int64)
    host_abs = np.zeros(a.n_weights, dtype=np.int64) if a.tc else None
    records = (games["keys"], games["values"]) + ((games["backed"],) if a.backed_targets else ()) + (games["steps"], games["lengths"], a.tuples, a.symmetric, a.gamma)
    if a.backed_targets:
        host = n.learn_backed_nt_on_host(*records, a.lam, host_acc, host_abs)
    else:
        host = n.learn_nt_on_host(*records, host_acc)
    acc, ab, host_w = host_acc.copy(), None if host_abs is None else host_abs.copy(), policy.copy()
    if a.tc:
        n.apply_tc_nt_on_host(host_w, host_acc, host_abs, *coherence, a.alpha / a.n_features)
    else:
        assert n.apply_nt_on_host(host_w, host_acc, a.alpha / a.n_features) > 0
    return acc, ab, host, host_w


@pytest.mark.parametrize("tc", [False, True], ids=["plain", "tc"])
def test_two_rounds_with_backed_targets_are_the_hosts(tc):
    """rollout_layers = 2, rollout_deep_empty_max = 3, backed_targets, lambda .5: per round the records against the mirror's games, acc
    over all W before the apply against learn_backed_nt_on_host on the MIRROR's games, the weights as float32 bit patterns after it;
    then learn_batch() twice on a twin agent leaves the same weights and records.  Round 0's games are the shared case's."""
    n = nt()
    options = dict(rollout_layers=2, rollout_deep_empty_max=E, backed_targets=True)
    a, b = _set(_agent(lam=0.5, tc=tc), **options), _set(_agent(lam=0.5, tc=tc), **options)
    coherence = (np.zeros(a.n_weights), np.zeros(a.n_weights)) if tc else None
    for r in range(2):
        policy = a.weights()
        want = host_rollout(*FROM_CASE) if r == 0 else nt_games_on_host(
            GAMES, MAX_STEPS, a.epsilon, a.gamma, policy, TUPLES, True, a.env_seed, a.agent_seed, a.tie_seed, a.round_board_id0(), a.round, deep_empty_max=E, backed=True)
        got, st0 = _launched(a, a.rollout), a.stats()
        _assert_games(a, got, want, ("round", r), True)
        a.learn()
        acc, ab, host, host_w = _host_learn(n, a, want, policy, coherence)
        st = a.stats()
        assert np.array_equal(a.acc.cpu().numpy(), acc) and int(acc[:, 1].sum()) == a.n_features * host["learnt"] > 0, r
        assert not tc or (np.array_equal(a.acc_abs.cpu().numpy(), ab) and ab.any()), r
        assert {k: st[k] - st0[k] for k in ("learnt", "skipped", "clamped")} == {k: host[k] for k in ("learnt", "skipped", "clamped")}, r
        assert host["skipped"] == want["truncated"] and host["learnt"] + host["skipped"] == int(want["lengths"].sum()), r
        a.apply()
        assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)) and not np.array_equal(host_w.view(np.uint32), policy.view(np.uint32)), r
        assert not a.acc.any().item() and not (tc and a.acc_abs.any().item())
        guards_intact(a)
        a.round += 1
    if tc:
        Ea, Aa = a.coherence()
        assert np.array_equal(bits(Ea), bits(coherence[0])) and np.array_equal(bits(Aa), bits(coherence[1]))
    b.learn_batch().learn_batch()
    _assert_twins(a, b, ("backed", "deltas"))
    assert b.rollout_depth_summary() == a.rollout_depth_summary() and a.round == b.round == 2
    guards_intact(b)


def _assert_twins(a, b, more=(), state=()):
    """two agents after the same rounds: the weights, the per-game arrays, the counters and `state` whole, the per-move rows up to each
    game's length"""
    import torch
    for k in ("weights_dev", "lengths", "total_score", "episode_reward", "counters") + tuple(state):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    played = np.arange(a.max_steps)[:, None] < a.lengths.cpu().numpy()[None, :]
    for k in PER_MOVE + tuple(more):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint64 if x.itemsize == 8 else x.dtype)[played], y.view(np.uint64 if y.itemsize == 8 else y.dtype)[played]), k


def _recorded(agent):
    """the recorder of tests/test_tfe_nt_launches_gpu.py on this agent: per launch the entry point's name without its prefix and the
    plain ints below 65,536 passed beside the struct; every launch recorded has run"""
    calls, launch, prefix = [], agent._launch, "pulse_tfe_nt_"

    def recorder(name, o, *args):
        assert name.startswith(prefix)
        calls.append((name[len(prefix):],) + tuple(x for x in args if type(x) is int and 0 <= x < 65536))
        return launch(name, o, *args)
    agent._launch = recorder
    return calls


def test_three_continued_rounds_with_backed_targets_are_the_hosts():
    """8 games in segments of 16 moves, continue_games, E = 3, backed targets, lambda .5: after each learn_batch() the records, `start`,
    both carries, `finished` and the weights against the host's chain (the mirror from `start`, learn_backed_nt_on_host, apply_nt_on_host,
    continue_pick_on_host); a round is the adaptive roll-out, the backed learner, the apply and the continue pick.  A twin agent that
    allocates its own state (round 0: start NULL) ends in the same state."""
    n, games, segment = nt(), 8, 16
    options = dict(rollout_layers=2, rollout_deep_empty_max=E, backed_targets=True, continue_games=True)
    a = _set(_agent(games=games, max_steps=segment, continued=True, lam=0.5), **options)
    b = _set(search_agent(games, segment, SEED, "seeded", epsilon=EPSILON, lam=0.5), **options)
    calls, twin_calls, c, counts = _recorded(a), _recorded(b), Carried(games), []
    round_ = [("rollout_adaptive", E), ("learn_backed",), ("apply",), ("continue_pick",)]
    for r in range(3):
        policy, board_id0 = a.weights(), a.round_board_id0()
        want = nt_games_on_host(games, segment, a.epsilon, a.gamma, policy, TUPLES, True, a.env_seed, a.agent_seed, a.tie_seed, board_id0, a.round,
                                deep_empty_max=E, backed=True, start=c.start)
        assert np.array_equal(want["start_left"], c.start)                  # boards a game moved on: none is zeroed
        _, _, host, host_w = _host_learn(n, a, want, policy, None)
        words, cut = pick_on_host(c, want, segment, a.env_seed, board_id0)
        before = _read(a)
        a.learn_batch()
        got = dict(_read(a), **{k + "_before": before[k] for k in PER_MOVE})
        assert_rollout(got, want, ("round", r), PER_MOVE)
        played = np.arange(segment)[:, None] < want["lengths"][None, :]
        assert np.array_equal(got["backed"][played], bits(want["backed"])[played]), r
        assert np.array_equal(_start_of(a), c.start) and np.array_equal(a.carry_score.cpu().numpy(), c.score), r
        assert np.array_equal(a.carry_moves.cpu().numpy(), c.moves) and a.finished.cpu().tolist() == c.finished, r
        assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32)), r
        assert calls[4 * r:] == round_ and host["skipped"] == words[5] == want["truncated"], (r, calls)
        counts.append((words[0], words[5]))
        guards_intact(a)
    print("games finished / continued per round:", counts, "depth words:", a.depth_stats.cpu().tolist())
    assert counts[0][1] >= 1 and a.round == 3 and sum(a.depth_stats.cpu().tolist()) == a.stats()["moves"]
    assert b.start is None
    for _ in range(3):
        b.learn_batch()
    assert twin_calls == 3 * round_
    _assert_twins(a, b, ("backed", "deltas"), ("start", "carry_score", "carry_moves", "finished", "depth_stats"))


def test_a_restarted_round_is_the_hosts():
    """restart_fraction .5 at E = 3, TD(0) on the records' targets: round 0 from the resets (the shared case's games) with its pick, then
    one round from the picked boards"""
    n = nt()
    a = _set(_agent(), rollout_layers=2, rollout_deep_empty_max=E, restart_fraction=0.5)
    a.start = None                                                          # (round 0 plays without `start`; the pick allocates it)
    a._guards = [g for g in a._guards if g[0] not in ("start", "restart_stats")]
    calls, policy = _recorded(a), a.weights()
    want = host_rollout(*FROM_CASE)
    _, _, _, host_w = _host_learn(n, a, want, policy, None)
    start, picked = n.restart_pick_on_host(want["keys"], want["lengths"], MAX_STEPS, a.env_seed, a.round_board_id0(), 0.5, a.restart_min_length)
    before = _read(a)
    a.learn_batch()
    got = dict(_read(a), **{k + "_before": before[k] for k in PER_MOVE})
    assert_rollout(got, want, "round 0", PER_MOVE)
    assert np.array_equal(_start_of(a), start) and tuple(a.restart_stats.cpu().tolist()) == picked and picked[0] >= 3
    assert np.array_equal(a.weights().view(np.uint32), host_w.view(np.uint32))
    assert calls == [("rollout_adaptive", E), ("learn",), ("apply",), ("restart_pick",)]
    want = nt_games_on_host(GAMES, MAX_STEPS, a.epsilon, a.gamma, host_w, TUPLES, True, a.env_seed, a.agent_seed, a.tie_seed, a.round_board_id0(), a.round,
                            deep_empty_max=E, start=start)
    left = want["start_left"]
    assert np.array_equal(left, start) and want["deep"] >= 5 and want["shallow"] >= 5
    got = _launched(a, a.rollout)
    _assert_games(a, got, want, "round 1", False)
    assert np.array_equal(_start_of(a), left) and calls[4:] == [("rollout_adaptive", E)]
    assert (got["backed"] == bits(np.float64(BACKED_PATTERN))).all()


def test_the_attribute_off_is_todays_round_and_the_rules_hold_on_the_device():
    a = _agent()
    calls = _recorded(_set(a, rollout_layers=2))
    assert a.rollout_deep_empty_max is None
    a.learn_batch()
    assert calls == [("rollout_search", 2), ("learn",), ("apply",)] and not a.depth_stats.any().item()
    for attributes, message in ((dict(rollout_layers=1, rollout_deep_empty_max=E), "rollout_deep_empty_max needs rollout_layers = 2"),
                                (dict(rollout_layers=2, rollout_deep_empty_max=17), "deep_empty_max must be None or an int in 0..16"),
                                (dict(rollout_layers=2, rollout_deep_empty_max=None, continue_games=True), "continue_games needs rollout_layers in (0, 1)")):
        with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
            _set(a, **attributes).rollout()
    assert len(calls) == 3
    guards_intact(a)
