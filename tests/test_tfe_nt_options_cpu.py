"""Which options of the 2048 n-tuple agent go together, without a GPU: check_options over all 96 rounds -- the
depth of the roll-out's search, backed targets, restarts, continuation, the cap on a game's moves, stages -- in the agent's words and in
the script's, held to the rules written out here a second time, in the order the agent tests them; the agent's rollout() on an object
that has no device raises exactly when the function does, with its message; and the script's run() and main() say the function's."""
import itertools

import pytest

from tests.tfe_nt_support import nt as _nt

ROUNDS = list(itertools.product((0, 1, 2), (False, True), (0.0, 0.5), (False, True), (1, 64), (False, True)))
# (depth, backed_targets, restart_fraction, continue_games, max_steps, staged) -> broken; how the agent's message begins; the script's
RULES = ((lambda d, b, r, c, m, s: c and r > 0, "continue_games does not go with restart_fraction > 0", "--continue-games does not go with --restart"),
         (lambda d, b, r, c, m, s: c and d == 2, "continue_games needs rollout_layers in (0, 1)", "--continue-games does not go with --train-layers 2"),
         (lambda d, b, r, c, m, s: c and m < 2, "continue_games needs max_steps >= 2", "--continue-games needs --max-steps 2 or more"),
         (lambda d, b, r, c, m, s: s and d == 2, "rollout_layers = 2 on an agent with stage_tiles", "--stages / --add-stage do not go with two chance layers"),
         (lambda d, b, r, c, m, s: r > 0 and d == 2, "restart_fraction > 0 needs rollout_layers in (0, 1)", "--restart does not go with --train-layers 2"),
         (lambda d, b, r, c, m, s: b and d == 0, "backed_targets needs rollout_layers in (1, 2)", "--backed needs --train-layers 1 or 2"))


def _expected(round_):
    """(the agent's opening words, the script's) of the first rule the round breaks, or None"""
    return next(((mine, flags) for broken, mine, flags in RULES if broken(*round_)), None)


def _said(call):
    try:
        call()
    except ValueError as refused:
        return str(refused)
    return None


def test_there_are_96_rounds_and_both_kinds():
    refused = [r for r in ROUNDS if _expected(r)]
    assert len(ROUNDS) == 96 and 0 < len(refused) < 96
    assert {_expected(r)[0] for r in refused} == {mine for _, mine, _ in RULES}        # every rule is the first one broken somewhere


@pytest.mark.parametrize("round_", ROUNDS, ids=lambda r: "-".join(str(x) for x in r))
def test_both_vocabularies_refuse_the_same_rounds(round_):
    nt, want = _nt(), _expected(round_)
    depth, backed, restart, cont, max_steps, staged = round_
    mine, flags = _said(lambda: nt.check_options(*round_)), _said(lambda: nt.check_options(*round_, script=True))
    assert (mine is None) == (flags is None) == (want is None)
    if want is None:
        assert nt.check_options(*round_) == nt.check_options(*round_, script=True) == (depth, restart > 0 or cont, 0, None)
    else:
        assert mine.startswith(want[0]) and flags.startswith(want[1]) and ": " in mine and ": " in flags


@pytest.mark.parametrize("round_", ROUNDS, ids=lambda r: "-".join(str(x) for x in r))
def test_rollout_refuses_what_the_function_refuses(round_):
    """on an object without a device: a refused round raises the function's words before anything is touched, an accepted one goes on to
    buffers the object has not got"""
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU as Agent
    depth, backed, restart, cont, max_steps, staged = round_
    agent = Agent.__new__(Agent)
    agent.rollout_layers, agent.backed_targets, agent.restart_fraction, agent.continue_games, agent.max_steps = depth, backed, restart, cont, max_steps
    agent.stage_tiles = (8,) if staged else ()
    want = _said(lambda: _nt().check_options(*round_))
    for call in (agent.rollout, agent.learn_batch):
        if want is None:
            with pytest.raises(AttributeError):
                call()
        else:
            assert _said(call) == want
    assert vars(agent).keys() == {"rollout_layers", "backed_targets", "restart_fraction", "continue_games", "max_steps", "stage_tiles"}


def test_the_script_says_the_functions_words(capsys):
    from pulselib_amd.scripts import tfe_ntuple as script
    nt = _nt()
    for round_ in ROUNDS:
        depth, backed, restart, cont, max_steps, staged = round_
        want = _said(lambda: nt.check_options(*round_, script=True))
        if want is None:
            continue
        kw = dict(train_layers=depth, backed=backed, restart=restart, continue_games=cont, max_steps=max_steps, stages=(512,) if staged else ())
        assert _said(lambda: script.run(None, 1, **kw)) == want, round_      # (refused before a device is asked for)
        argv = ["--train-layers", str(depth), "--restart", str(restart), "--max-steps", str(max_steps)]
        argv += ["--backed"] * backed + ["--continue-games"] * cont + ["--stages", "512"] * staged
        with pytest.raises(SystemExit) as err:
            script.main(argv)
        assert err.value.code == 2 and want in capsys.readouterr().err, argv


def test_the_evaluations_rules_come_first_and_stages_refuse_any_second_layer():
    nt = _nt()
    for kw, mine, flags in ((dict(search=True, layers=1, deep_empty_max=3), "deep_empty_max needs layers = 2", "--deep-empty-max needs --search --layers 2"),
                            (dict(deep_empty_max=3), "deep_empty_max needs layers = 2", "--deep-empty-max needs --search --layers 2"),
                            (dict(staged=True, search=True, layers=2, deep_empty_max=3), "layers = 2 on an agent with stage_tiles", "--deep-empty-max does not go with --stages"),
                            (dict(staged=True, search=True, layers=2), "layers = 2 on an agent with stage_tiles", "--stages / --add-stage do not go with two chance layers"),
                            (dict(depth=2, staged=True, search=True, layers=2, deep_empty_max=3, continue_games=True), "layers = 2 on an agent with stage_tiles",
                             "--deep-empty-max does not go with --stages")):
        assert _said(lambda: nt.check_options(**kw)).startswith(mine) and _said(lambda: nt.check_options(**kw, script=True)).startswith(flags), kw
    assert nt.check_options(staged=True, layers=2) == (0, False, 0, None)     # (no search: its depth is not asked about)
    assert nt.check_options(1, True, 0.5, search=True, layers=2, deep_empty_max=16) == (1, True, 2, 16)
    for bad in (dict(depth=3), dict(depth=True), dict(restart_fraction=1.0), dict(search=True, layers=0), dict(deep_empty_max=17)):
        with pytest.raises(ValueError, match="must be"):
            nt.check_options(**bad)
