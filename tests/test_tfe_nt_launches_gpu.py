"""The launches of the 2048 n-tuple agent, by name: which entry points two learn_batch rounds and the evaluation
calls go through, in which order and with which depth or threshold beside the struct, for every opt-in, against a table recorded on the
agent as it was before its Python layer was taken apart.  `_launch` of the instance is replaced by a recorder that calls through, so every
launch recorded has run; nothing is read back but by the evaluations.  8 games of at most 16 moves: a fraction of a second per case."""
import pytest

pytestmark = pytest.mark.gpu

GAMES, TUPLES = 8, ((0, 1, 2, 3), (4, 5, 6, 7))
P = "pulse_tfe_nt_"
PLAIN = [("rollout",), ("learn",), ("apply",)]
BACKED = [("rollout_backed", 1), ("learn_backed",), ("apply",)]
# id: (__init__'s keywords, attributes set on the agent, round 1's launches, round 2's)
ROUNDS = {
    "default": ({}, {}, PLAIN, PLAIN),
    "lam": (dict(lam=.5), {}, [("rollout",), ("learn_lambda",), ("apply",)], [("rollout",), ("learn_lambda",), ("apply",)]),
    "tc": (dict(tc=True), {}, [("rollout",), ("learn_tc",), ("apply_tc",)], [("rollout",), ("learn_tc",), ("apply_tc",)]),
    "layers1": ({}, dict(rollout_layers=1), [("rollout_search", 1), ("learn",), ("apply",)], [("rollout_search", 1), ("learn",), ("apply",)]),
    "layers2": ({}, dict(rollout_layers=2), [("rollout_search", 2), ("learn",), ("apply",)], [("rollout_search", 2), ("learn",), ("apply",)]),
    "backed": ({}, dict(rollout_layers=1, backed_targets=True), BACKED, BACKED),
    "restart": ({}, dict(restart_fraction=.5), PLAIN + [("restart_pick",)], [("rollout_from", 0), ("learn",), ("apply",), ("restart_pick",)]),
    "restart-backed": ({}, dict(restart_fraction=.5, rollout_layers=1, backed_targets=True), BACKED + [("restart_pick",)],
                       [("rollout_from", 1), ("learn_backed",), ("apply",), ("restart_pick",)]),
    "continue": (dict(max_steps=4), dict(continue_games=True), PLAIN + [("continue_pick",)],
                 [("rollout_from", 0), ("learn",), ("apply",), ("continue_pick",)]),
    "staged": (dict(stage_tiles=(8,)), {}, [("rollout_staged", 0), ("learn_staged",), ("apply",), ("apply",)],
               [("rollout_staged", 0), ("learn_staged",), ("apply",), ("apply",)]),
    "staged-tc": (dict(stage_tiles=(8,), tc=True), {}, [("rollout_staged", 0), ("learn_staged",), ("apply_tc",), ("apply_tc",)],
                  [("rollout_staged", 0), ("learn_staged",), ("apply_tc",), ("apply_tc",)]),
}
# id: (__init__'s keywords, the method, its keywords, the launches)
EVALUATIONS = {
    "evaluate": ({}, "evaluate", {}, [("evaluate",)]),
    "search1": ({}, "evaluate_search", dict(layers=1), [("evaluate_search",)]),
    "search2": ({}, "evaluate_search", dict(layers=2), [("evaluate_search_deep", 2)]),
    "adaptive": ({}, "evaluate_search", dict(layers=2, deep_empty_max=3), [("evaluate_search_adaptive", 3)]),
    "launch-adaptive": ({}, "evaluate_search_launch", dict(layers=2, deep_empty_max=3), [("evaluate_search_adaptive", 3)]),
    "staged-evaluate": (dict(stage_tiles=(8,)), "evaluate", {}, [("evaluate_staged", 0)]),
    "staged-search1": (dict(stage_tiles=(8,)), "evaluate_search", dict(layers=1), [("evaluate_staged", 1)]),
}


def recorded_agent(init, attributes):
    """(the agent, the list its launches are recorded in): per launch the entry point's name without its prefix and the plain ints below
    65,536 passed beside the struct -- the depths and thresholds; a device pointer is an int too, and never that small"""
    import torch
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    agent = NTupleTDAfterstateTFEGPU(torch.device("cuda:0"), GAMES, **dict(dict(tuples=TUPLES, max_steps=16, seed=11), **init))
    for k, v in attributes.items():
        setattr(agent, k, v)
    calls, launch = [], agent._launch

    def recorder(name, o, *args):
        assert name.startswith(P)
        calls.append((name[len(P):],) + tuple(a for a in args if type(a) is int and 0 <= a < 65536))
        return launch(name, o, *args)
    agent._launch = recorder
    return agent, calls


def rounds_launches(init, attributes):
    agent, calls = recorded_agent(init, attributes)
    agent.learn_batch()
    first = len(calls)
    agent.learn_batch()
    torch_sync(agent)
    return agent, calls[:first], calls[first:]


def evaluation_launches(init, method, kw):
    agent, calls = recorded_agent(init, {})
    getattr(agent, method)(n_games=GAMES, **kw)
    torch_sync(agent)
    return agent, calls


def torch_sync(agent):
    import torch
    torch.cuda.synchronize(agent.device)


def _holds_no_entry_point(agent):
    """neither the agent nor its class has the attributes an evaluation under search used to leave its entry point in"""
    return not any(hasattr(x, "_eval_" + k) for x in (agent, type(agent)) for k in ("entry", "args", "layers"))


@pytest.mark.parametrize("case", ROUNDS)
def test_two_rounds_go_through_the_launches_they_went_through(case):
    init, attributes, first, second = ROUNDS[case]
    agent, one, two = rounds_launches(init, attributes)
    assert (one, two) == (first, second) and agent.round == 2
    assert _holds_no_entry_point(agent)


@pytest.mark.parametrize("case", EVALUATIONS)
def test_an_evaluation_goes_through_the_launch_it_went_through(case):
    init, method, kw, want = EVALUATIONS[case]
    agent, calls = evaluation_launches(init, method, kw)
    assert calls == want
    assert _holds_no_entry_point(agent)
