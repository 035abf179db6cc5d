"""Launch times of the 2048 n-tuple network (csrc/tfe_ntuple.hip, agents/tfe_ntuple_td_gpu.py), ONE JSON line
per batch size B (65,536 and 1,048,576 games per round by default; a size whose buffers do not fit the free device memory is
skipped and says so) and state of the weights:
  zero    : every timed round starts from ZERO weights (the weights are cleared before it, untimed): greedy on the reward, short
            games, every lane of a wavefront on the same few hot weights.
  trained : --trained-rounds T (8) untimed rounds first, then the timed rounds go on learning: longer games, spread indices.
Per state --warmup W (2) untimed rounds, then --repeats R (5) timed ones; the roll-out, the learn and the apply launch each sit between
their own pair of HIP events; min / median / max of each, the moves per round beside them, moves/s of the roll-out and of the learn
launch, 16-byte accumulator atomics/s of the learn launch (2 F per move) and bytes/s of the apply launch (20 bytes per weight read,
20 written where touched: only the read side is counted).  Then the evaluation launch on the weights the rounds left, --repeats
times after one untimed call.  --search: per B and per --search-games G (1,024: few wavefronts, the time of the longest game; 65,536: every compute unit busy) one more
line, {"search": ...}: G games on the weights the rounds left
from the default evaluation boards under the one-ply policy and under expectimax search one chance layer deep (DESIGN.md section
13.1), each launch between its own HIP events in the same process, --repeats times after one untimed call: seconds, moves, seconds
per move (a move = one move of one game; the launch's time over all the moves it played) and the ratio of the two.  --search --layers 2:
the line also holds "search2", the evaluation under search two chance layers deep (section 13.4) on the same boards, its per-move time
over the one-layer search's, and the yardstick of that ratio: the mean number of child searches a two-layer move makes, counted on the
host from the candidate and empty-cell masks of the boards of 32 games played under that policy (children_per_move); the ratio over
the count, and whether it is within the count + 50 %.  --search --layers 2 --deep-empty-max E [E ...]: per G and E
one more line, {"adaptive_search": ...}: the evaluation launches under one layer, under the search two layers deep on the boards with
at most E empty cells, and under two layers on every board, same weights and boards, alternating in turn in the same process, each
between its own HIP events, one untimed pass and then --repeats: the three launch times, the moves and the share of them searched two
layers deep, the mean scores with their standard errors, and the differences E - one layer and E - two layers paired by board.
--lambda L: per B one more line, {"lambda": ...}: on the games of the last timed round, in the same
process and back to back, the TD(0) learn launch (pulse_tfe_nt_learn) and the TD(lambda) launch (pulse_tfe_nt_learn_lambda: the backward
walk and the adds) each between its own pair of HIP events, --warmup untimed pairs and then --repeats timed ones, alternating; the
accumulators are zeroed, untimed, before every launch, so both add the same moves into empty cells.  --tc: per B one more line, marked {"tc": true}: on the games of the last timed round, in the same process and alternating, the fixed-step pair
(pulse_tfe_nt_learn, then pulse_tfe_nt_apply on what it added) and the temporal-coherence pair (pulse_tfe_nt_learn_tc, then
pulse_tfe_nt_apply_tc), with --lambda L also pulse_tfe_nt_learn_lambda beside pulse_tfe_nt_learn_tc at L; every launch
between its own pair of HIP events, the accumulators zeroed (untimed) before every learn launch; the weights are put back and E and
A zeroed afterwards.  --train-layers L (1 or 2): per B one more line, {"train_rollout": ...}: on the weights the rounds left, the recording
launch under search L chance layers deep (pulse_tfe_nt_rollout_search) and, alternating with it in the same
process, the evaluation launch under the same policy on the same boards, weights and epsilon, each between its own pair of HIP events;
the ratio of the medians, the evaluation's own spread (max / min) beside it, and the yardstick by count: 1 + 1 / (the mean number of
candidate moves per board), counted on the host over 32 games played under that policy, and whether the ratio is within it + 50 %.
--backed (with --train-layers L): per B two more lines.  {"backed_rollout": ...}: on the weights the rounds left, the
recording launch with the search's backed-up values (pulse_tfe_nt_rollout_backed) and, alternating with it in the same process, the
parent's recording launch (pulse_tfe_nt_rollout_search) on the same boards, weights and epsilon, each between its own pair of HIP
events; the ratio of the medians beside the parent launch's own spread (max / min) and whether the ratio is inside it; by count the new
launch adds one 8-byte store per move and three compares.  {"backed_learn": ...}: on the records of the last such launch,
pulse_tfe_nt_learn_backed and pulse_tfe_nt_learn_lambda at the same lambda (--lambda, 0 if not given), alternating, the accumulators
zeroed (untimed) before each; the walk reads 25 bytes per move against 17.  --backed-regime: instead of everything above, ONE line,
{"backed_regime": ...}: section 13.5's regime -- learn_batch --regime-rounds (12) times with the first --games games per round, then
--regime-eval-games (2,048) games from the default evaluation boards one ply deep and under one-layer search, paired by board -- for
four agents: rollout_layers = 0, rollout_layers = 1, and rollout_layers = 1 with backed_targets at lambda 0 and at lambda 0.5.
--restart F: per B two more lines.  {"restart_rollout": ...}: on the weights the rounds left and with `start` all zero, so that it
plays the parent's very games, the restarted recording launch (pulse_tfe_nt_rollout_from) beside pulse_tfe_nt_rollout (layers 0),
pulse_tfe_nt_rollout_search and pulse_tfe_nt_rollout_backed (one layer), each pair alternating in the same process between its own HIP
events; per pair the ratio of the medians beside the parent launch's own spread (max / min) and whether the ratio is inside it.
{"restart_pick": ...}: the pick launch (pulse_tfe_nt_restart_pick) at fraction F on the records of the last of those launches, by the
same events; by count it reads 4 + 8 bytes and writes 8 per game.  --restart-regime: instead of everything above, ONE line,
{"restart_regime": ...}: section 13.5's regime for four agents: restart_fraction 0 and --restart (0.5 if not given) one ply deep, and the
same two under rollout_layers = 1 with backed_targets at lambda 0.5; per round the games restarted and their mean depth, per agent
the moves learnt, and the evaluations' paired differences with and without restart.
--stages TILES (512,2048): per B one more line, {"staged": ...}: a second agent with those stage tiles and the
first agent's weights copied into every stage's slice, so that a staged launch plays, records and adds exactly what its unstaged
sibling does; ten pairs (the recording launch one ply deep and one layer deep with and without backed values, the TD(0), TD(lambda)
and backed learners, the two evaluations, the board search on the afterstates of move 64, and last the apply launch against the
apply launches of the three stages, each after an untimed TD(lambda) learn launch), each alternating between its own HIP events, with the ratio of the medians beside the sibling's own
spread.  --stage-regime: instead of everything above, ONE line, {"stage_regime": ...}: section 13.5's regime for the unstaged agent one
ply deep, and under one-layer search with backed targets at lambda 0.5 for the unstaged agent, for --stages from round 0 and for one
stage added half-way by add_stage; the evaluations' largest-tile histograms and paired differences.  Without --stages the two tiles are
chosen from the baseline's histogram: the largest tile at least half its evaluation games reached, and a quarter of it.
--continue-games: instead of everything above, per B ONE line, {"continue_pick": ...}: an agent with
max_steps = --continue-max-steps (64) and continue_games plays --continue-rounds (16) rounds and one more recording launch; on those
records the continue pick (pulse_tfe_nt_continue_pick) and the restart pick (pulse_tfe_nt_restart_pick, fraction 0.5) alternate, each
between its own pair of HIP events, --warmup untimed turns and then --repeats; the games continued and finished per launch beside them.
--continue-regime: instead, ONE line, {"continue_regime": ...}: section 13.5's regime one ply deep (--regime-rounds whole-game rounds)
and a continue_games agent of --continue-max-steps moves a segment trained until it has learnt at least as many moves: the rounds, their
summed launch time and the wall time, the whole games that finished, and both evaluations (capped at --max-steps) paired by board.
--train-layers 2 --train-deep-empty-max E [E ...]: per B and E one more line, {"adaptive_rollout": ...}, on the
weights the rounds left.  At E = 16 the recording launch at the adaptive depth (pulse_tfe_nt_rollout_adaptive) without and with backed
values beside the two-layer recording launches (pulse_tfe_nt_rollout_search, pulse_tfe_nt_rollout_backed at layers = 2), the four
alternating in the same process, each between its own pair of HIP events: medians with min and max, the ratios, and whether the new
launch's median is inside its parent's min .. max widened by 2 %.  At any other E the recording launch without and with backed values
beside the evaluation launch at the same E (pulse_tfe_nt_evaluate_search_adaptive) on the same boards, weights and epsilon: the ratios,
the moves and the deep share.  Then one {"adaptive_round": ...} line per B at the first E below 16: roll-out + learn + apply with backed
targets under one layer, under two layers and under two layers at E, each from the same weights and boards (put back, untimed, before
every round), and the continue pick and the restart pick on the records of the last.  --adaptive-regime: instead of everything above,
ONE line, {"adaptive_regime": ...}: section 13.5's regime with backed targets at lambda 0.5 under rollout_layers = 1 and under
rollout_layers = 2 with rollout_deep_empty_max = 3 (--train-deep-empty-max's first value if given), with rollout_layers = 2 on every
board between them (the two-layer backed round no regime had recorded), and the first pair again with continue_games
in segments of --continue-max-steps moves trained until each has learnt as many moves as its whole-game twin; per regime the wall time,
the deep share of its training moves and both evaluations, and the differences adaptive - one layer paired by board.
--exchange: instead of everything above, two lines, {"exchange": ...}, in a single process on the default
network with 4,096 games (--games' first value if given): at max_steps 64 and at whole games (--max-steps).  Per turn a real roll-out
and learn launch (untimed), then, each between its own pair of HIP events: the pack launch (pulse_tfe_nt_acc_pack, the list at its
default capacity) twice -- pack_first is the first reader of the accumulators after the learn launch's adds, pack reads them as the apply
launch does, behind a launch that has just read them --, the unpack launch of that list into a second, zeroed accumulator (pulse_tfe_nt_acc_unpack), and the apply launch, the
yardstick: the pack reads the bytes the apply launch reads.  The entries found, the medians with min and max, and the ratios to the
apply launch measured in the same run.  --exchange-ranks 2 adds one line, {"exchange_ranks": ...}: the wall time of --regime-rounds
rounds at max_steps 64 in one process beside the same rounds on two gloo ranks that share device 0 -- a REHEARSAL of the protocol: two
ranks on one device say nothing about scaling -- with the paths taken, the entries per rank and the bytes moved per round.
max_steps is --max-steps (4,096; the per-move buffers are B x max_steps x 17 bytes, 25 with deltas, 33 with backed).  Lines are also
appended to profiles/tfe_mc/bench_tfe_ntuple.jsonl.  Nothing is asserted about the rates."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def _timed_round(agent, torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    agent.rollout()
    ev[1].record()
    agent.learn()
    ev[2].record()
    agent.apply()
    ev[3].record()
    agent.round += 1
    ev[3].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(3)]


def _timed_evaluate(agent, torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    agent.eval_counters(clear=True)
    ev[0].record()
    agent.evaluate_launch()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3, agent.eval_counters()


def children_per_move(agent, torch, sample, max_moves, layers=2):
    """The mean number of one-layer searches a two-layer move makes: `sample` games from the default evaluation boards played through
    the environment's own launches under the two-layer policy (agent.search(layers=2), greedy), and on every board met, counted on the
    host from the moves' masks, the live children: 2 * n_empty(B_a) summed over the candidate moves a.  Stops after max_moves moves.
    Beside it candidates_per_move, the mean number of candidate moves of those boards; layers = 1: the games of the one-layer policy."""
    import numpy as np
    from pulselib_amd.agents.tfe_ntuple_td_gpu import moves_on_host
    from pulselib_amd.environments.TFE.TFE import TFEBatch
    env = TFEBatch(agent.device, sample, 4, seed=agent.env_seed, board_id0=agent.eval_board_id0())
    boards, _ = env.reset()
    live, children, candidates, moves = np.ones(sample, dtype=bool), 0, 0, 0
    shifts = np.uint64(4) * np.arange(16, dtype=np.uint64)
    for _ in range(max_moves):
        cells = boards.cpu().numpy().reshape(sample, 16).astype(np.int64)
        logs = np.where(cells > 0, np.log2(np.maximum(cells, 1)).round().astype(np.int64), 0).astype(np.uint64)
        keys = (logs << shifts).sum(axis=1, dtype=np.uint64)
        after, _ = moves_on_host(keys)
        n_empty = (((after[:, :, None] >> shifts) & np.uint64(15)) == 0).sum(axis=2)
        per_board = (2 * n_empty * (after != keys[:, None])).sum(axis=1)
        children, moves = children + int(per_board[live].sum()), moves + int(live.sum())
        candidates += int((after != keys[:, None])[live].sum())
        action = agent.search(keys, layers=layers)["action"].astype(np.int64)
        boards, _, dones, _, _ = env.step(torch.from_numpy(np.maximum(action, 0)))
        live &= ~dones.cpu().numpy() & (action >= 0)
        if not live.any():
            break
    return {"sample_games": sample, "sample_moves": moves, "children_per_move": children / max(moves, 1),
            "candidates_per_move": candidates / max(moves, 1)}


def train_rollout_line(agent, torch, layers, warmup, repeats):
    """the recording launch under search and the evaluation launch under the same policy, on the boards of the agent's next round"""
    board_id0, before = agent.round_board_id0(), agent.stats()
    launches = (("rollout_search", lambda: agent.rollout_search_launch(layers)),
                ("evaluate_search", lambda: agent.evaluate_search_launch(epsilon=agent.epsilon, board_id0=board_id0, layers=layers)))
    seconds = {name: [] for name, _ in launches}
    for i in range(warmup + repeats):
        for name, launch in launches:
            agent.eval_counters(clear=True)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch()
            ev[1].record()
            ev[1].synchronize()
            if i >= warmup:
                seconds[name].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    e, st = agent.eval_counters(), agent.stats()
    moves = (st["moves"] - before["moves"]) // (warmup + repeats)
    ro, ev_s = _spread(seconds["rollout_search"]), _spread(seconds["evaluate_search"])
    count = children_per_move(agent, torch, 32, agent.max_steps, layers)
    ratio, yardstick = ro["median"] / ev_s["median"], 1.0 + 1.0 / count["candidates_per_move"]
    return {"train_rollout": {"games": agent.n_games, "layers": layers, "epsilon": agent.epsilon, "trained_rounds": agent.round, "max_steps": agent.max_steps,
                              "warmup": warmup, "repeats": repeats, "moves": moves, "evaluate_moves": e["moves"], "rollout_search_s": ro,
                              "evaluate_search_s": ev_s, "ratio": ratio, "evaluate_spread": ev_s["max"] / ev_s["min"], **count,
                              "yardstick_by_count": yardstick, "ratio_over_yardstick": ratio / yardstick, "within_margin": ratio <= 1.5 * yardstick,
                              "mean_length": moves / agent.n_games, "mean_final_score": agent.total_score.double().mean().item(),
                              "record_bytes": 17 * moves}}


def _alternate(agent, torch, launches, warmup, repeats, before=None):
    """seconds per name: the launches in turn, each between its own pair of HIP events, `warmup` untimed turns and then `repeats`"""
    seconds = {name: [] for name, _ in launches}
    for i in range(warmup + repeats):
        for name, launch in launches:
            if before:
                before()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch()
            ev[1].record()
            ev[1].synchronize()
            if i >= warmup:
                seconds[name].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return seconds


def backed_lines(agent, torch, layers, lam, warmup, repeats):
    """the recording launch with backed values beside the parent's, then the backed learner beside the TD(lambda) learner on its records"""
    before = agent.stats()
    seconds = _alternate(agent, torch, (("rollout_search", lambda: agent.rollout_search_launch(layers)),
                                        ("rollout_backed", lambda: agent.rollout_backed_launch(layers))), warmup, repeats)
    moves = (agent.stats()["moves"] - before["moves"]) // (2 * (warmup + repeats))
    old, new = _spread(seconds["rollout_search"]), _spread(seconds["rollout_backed"])
    ratio, spread = new["median"] / old["median"], old["max"] / old["min"]
    common = {"games": agent.n_games, "layers": layers, "epsilon": agent.epsilon, "trained_rounds": agent.round, "max_steps": agent.max_steps,
              "warmup": warmup, "repeats": repeats}
    rollout = {"backed_rollout": {**common, "moves": moves, "rollout_search_s": old, "rollout_backed_s": new, "ratio": ratio, "parent_spread": spread,
                                  "inside_parent_spread": 1.0 / spread <= ratio <= spread, "more_bytes": 8 * moves,
                                  "mean_length": moves / agent.n_games}}
    before = agent.stats()
    seconds = _alternate(agent, torch, (("learn_lambda", lambda: agent.learn_lambda_launch(lam)), ("learn_backed", lambda: agent.learn_backed_launch(lam))),
                         warmup, repeats, before=agent.acc.zero_)
    agent.acc.zero_()
    learnt = (agent.stats()["learnt"] - before["learnt"]) // (2 * (warmup + repeats))
    old, new = _spread(seconds["learn_lambda"]), _spread(seconds["learn_backed"])
    ratio, spread = new["median"] / old["median"], old["max"] / old["min"]
    learn = {"backed_learn": {**common, "lambda": lam, "gamma": agent.gamma, "moves_learnt": learnt, "learn_lambda_s": old, "learn_backed_s": new,
                              "ratio": ratio, "parent_spread": spread, "inside_parent_spread": 1.0 / spread <= ratio <= spread,
                              "walk_bytes": 25 * learnt, "walk_bytes_lambda": 17 * learnt, "atomics": 2 * agent.n_features * learnt}}
    return [rollout, learn]


def backed_regime_line(torch, dev, games, rounds, eval_games, max_steps):
    """section 13.5's regime for the four agents; the evaluations are paired by board"""
    import numpy as np
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    out, ev = {"games": games, "rounds": rounds, "eval_games": eval_games, "seed": 0, "max_steps": max_steps}, {}
    for name, layers, backed, lam in (("layers_0", 0, False, 0.0), ("layers_1", 1, False, 0.0), ("layers_1_backed", 1, True, 0.0),
                                      ("layers_1_backed_lambda_0.5", 1, True, 0.5)):
        agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=max_steps, seed=0, lam=lam)
        agent.rollout_layers, agent.backed_targets = layers, backed
        per_round = []
        for _ in range(rounds):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            agent.learn_batch()
            e[1].record()
            e[1].synchronize()
            per_round.append({"seconds": e[0].elapsed_time(e[1]) * 1e-3, "mean_length": agent.lengths.double().mean().item(),
                              "mean_score": agent.total_score.double().mean().item()})
        ev[name] = {"one_ply": agent.evaluate(n_games=eval_games, per_game=True), "search": agent.evaluate_search(n_games=eval_games, per_game=True)}
        out[name] = {"rollout_layers": layers, "backed_targets": backed, "lambda": lam, "rounds": per_round, "stats": agent.stats(),
                     **{k: {"mean": e["mean_score"], "se": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "cut": e["truncated"]}
                        for k, e in ev[name].items()}}
        del agent
        torch.cuda.empty_cache()
    for name in ("layers_1_backed", "layers_1_backed_lambda_0.5"):
        for other in ("layers_0", "layers_1"):
            for k in ("one_ply", "search"):
                d = (ev[name][k]["total_score"] - ev[other][k]["total_score"]).astype(np.float64)
                out[f"{k}_eval_{name}_minus_{other}"] = {"mean": d.mean(), "se": d.std(ddof=1) / d.size ** .5}
    return {"backed_regime": out}


def restart_lines(agent, torch, fraction, min_length, warmup, repeats):
    """the restarted recording launch with `start` all zero beside each of its three parents, then the pick launch on the last records"""
    agent._restart_state()
    agent.start.zero_()
    common = {"games": agent.n_games, "epsilon": agent.epsilon, "trained_rounds": agent.round, "max_steps": agent.max_steps, "warmup": warmup, "repeats": repeats}
    pairs = {}
    for name, parent, new in (("layers_0", lambda: agent._launch("pulse_tfe_nt_rollout", agent._rollout_struct()), lambda: agent.rollout_from_launch(0)),
                              ("layers_1", lambda: agent.rollout_search_launch(1), lambda: agent.rollout_from_launch(1)),
                              ("layers_1_backed", lambda: agent.rollout_backed_launch(1), lambda: agent.rollout_from_launch(1, backed=True))):
        before = agent.stats()
        seconds = _alternate(agent, torch, (("parent", parent), ("from", new)), warmup, repeats)
        moves = (agent.stats()["moves"] - before["moves"]) // (2 * (warmup + repeats))
        old, fresh = _spread(seconds["parent"]), _spread(seconds["from"])
        ratio, spread = fresh["median"] / old["median"], old["max"] / old["min"]
        pairs[name] = {"moves": moves, "parent_s": old, "from_s": fresh, "ratio": ratio, "parent_spread": spread,
                       "inside_parent_spread": 1.0 / spread <= ratio <= spread, "started": int((agent.start != 0).sum().item())}
    seconds = _alternate(agent, torch, (("pick", lambda: agent.restart_pick_launch(fraction, min_length)),), warmup, repeats)
    summary = agent.restart_summary()
    agent.start.zero_()
    pick = {**common, "fraction": fraction, "min_length": min_length, "pick_s": _spread(seconds["pick"]), "picked": summary["picked"] // (warmup + repeats),
            "mean_depth": summary["mean_depth"], "bytes_read": 12 * agent.n_games, "bytes_written": 8 * agent.n_games}
    return [{"restart_rollout": {**common, **pairs}}, {"restart_pick": pick}]


def restart_regime_line(torch, dev, games, rounds, eval_games, max_steps, fraction, min_length):
    """section 13.5's regime with and without restart, one ply deep and under one-layer search with backed targets at lambda 0.5; the
    evaluations are from reset and paired by board"""
    import numpy as np
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    out = {"games": games, "rounds": rounds, "eval_games": eval_games, "seed": 0, "max_steps": max_steps, "fraction": fraction, "min_length": min_length}
    ev = {}
    rows = (("layers_0", 0, False, 0.0, 0.0), ("layers_0_restart", 0, False, 0.0, fraction),
            ("layers_1_backed_lambda_0.5", 1, True, 0.5, 0.0), ("layers_1_backed_lambda_0.5_restart", 1, True, 0.5, fraction))
    for name, layers, backed, lam, restart in rows:
        agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=max_steps, seed=0, lam=lam)
        agent.rollout_layers, agent.backed_targets, agent.restart_fraction, agent.restart_min_length = layers, backed, restart, min_length
        per_round, began = [], {"picked": 0, "mean_depth": 0.0}
        for _ in range(rounds):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            agent.learn_batch()
            e[1].record()
            e[1].synchronize()
            per_round.append({"seconds": e[0].elapsed_time(e[1]) * 1e-3, "mean_length": agent.lengths.double().mean().item(),
                              "mean_score": agent.total_score.double().mean().item(), "restarted": began["picked"],
                              "restarted_share": began["picked"] / games, "mean_depth": began["mean_depth"]})
            if restart:
                began = agent.restart_summary()                             # what this round's pick left for the next
        ev[name] = {"one_ply": agent.evaluate(n_games=eval_games, per_game=True), "search": agent.evaluate_search(n_games=eval_games, per_game=True)}
        st = agent.stats()
        out[name] = {"rollout_layers": layers, "backed_targets": backed, "lambda": lam, "restart_fraction": restart, "rounds": per_round, "stats": st,
                     "moves_learnt": st["learnt"],
                     **{k: {"mean": e["mean_score"], "se": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "cut": e["truncated"]}
                        for k, e in ev[name].items()}}
        del agent
        torch.cuda.empty_cache()
    for name in ("layers_0", "layers_1_backed_lambda_0.5"):
        for k in ("one_ply", "search"):
            d = (ev[name + "_restart"][k]["total_score"] - ev[name][k]["total_score"]).astype(np.float64)
            out[f"{k}_eval_{name}_restart_minus_{name}"] = {"mean": d.mean(), "se": d.std(ddof=1) / d.size ** .5}
    return {"restart_regime": out}


def continue_pick_line(torch, dev, games, segment, rounds, warmup, repeats):
    """the continue pick beside the restart pick on the records of an agent that has played `rounds` continued rounds of `segment` moves:
    the two launches alternate, each between its own pair of HIP events"""
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=segment, seed=0)
    agent.continue_games = True
    for _ in range(rounds):
        agent.learn_batch()
    agent.rollout()                                                         # the records the picks read: the next round's, under this round's ids
    agent.finished_summary()
    seconds = _alternate(agent, torch, (("restart_pick", lambda: agent.restart_pick_launch(0.5, 2)), ("continue_pick", agent.continue_pick_launch)),
                         warmup, repeats)
    done, turns = agent.finished_summary(), warmup + repeats
    restart = agent.restart_summary()
    old, new = _spread(seconds["restart_pick"]), _spread(seconds["continue_pick"])
    line = {"games": games, "max_steps": segment, "continued_rounds": rounds, "warmup": warmup, "repeats": repeats, "restart_pick_s": old, "continue_pick_s": new,
            "ratio": new["median"] / old["median"], "continued": done["continued"] // turns, "finished": done["games"] // turns,
            "restart_picked": restart["picked"] // turns, "bytes_read": (4 + 1 + 8 + 8 + 8 + 4) * games + 8 * (done["continued"] // turns),
            "bytes_written": (8 + 8 + 4) * games}
    del agent
    torch.cuda.empty_cache()
    return {"continue_pick": line}


def continue_regime_line(torch, dev, games, rounds, eval_games, max_steps, segment):
    """section 13.5's regime one ply deep -- `rounds` whole-game rounds -- beside a continue_games agent with max_steps = `segment`
    trained until it has learnt at least as many moves; the evaluations are from reset, capped at `max_steps`, and paired by board"""
    import time
    import numpy as np
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    out, ev = {"games": games, "rounds": rounds, "eval_games": eval_games, "seed": 0, "max_steps": max_steps, "segment": segment}, {}

    def timed_batch(agent):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        agent.learn_batch()
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]) * 1e-3

    def row(agent, seconds, wall, more):
        name = "continued" if agent.continue_games else "whole_games"
        ev[name] = {"one_ply": agent.evaluate(n_games=eval_games, per_game=True), "search": agent.evaluate_search(n_games=eval_games, per_game=True)}
        st = agent.stats()
        out[name] = {"max_steps": agent.max_steps, "rounds": agent.round, "round_seconds_sum": sum(seconds), "round_seconds": _spread(seconds),
                     "wall_seconds": wall, "stats": st, "moves_learnt": st["learnt"], **more,
                     **{k: {"mean": e["mean_score"], "se": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "cut": e["truncated"]}
                        for k, e in ev[name].items()}}
        return st["learnt"]

    agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=max_steps, seed=0)
    t0 = time.perf_counter()
    seconds = [timed_batch(agent) for _ in range(rounds)]
    target = row(agent, seconds, time.perf_counter() - t0, {})
    del agent
    torch.cuda.empty_cache()
    agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=segment, seed=0)
    agent.continue_games, agent.eval_max_steps = True, max_steps
    seconds, t0 = [], time.perf_counter()
    while agent.stats()["learnt"] < target:                                 # (synchronises once a round: inside the wall time, outside the events)
        seconds.append(timed_batch(agent))
    wall, done = time.perf_counter() - t0, agent.finished_summary()
    row(agent, seconds, wall, {"finished": {k: done[k] for k in ("games", "mean_score", "mean_length", "continued", "resumed", "tile_capped")}})
    for k in ("one_ply", "search"):
        d = (ev["continued"][k]["total_score"] - ev["whole_games"][k]["total_score"]).astype(np.float64)
        out[f"{k}_eval_continued_minus_whole_games"] = {"mean": d.mean(), "se": d.std(ddof=1) / d.size ** .5}
    return {"continue_regime": out}


def staged_lines(agent, torch, dev, stage_tiles, lam, warmup, repeats):
    """every staged launch beside its unstaged sibling, on `agent`'s weights copied into every stage's slice: the games, the moves and
    the adds per move are then the same, and a ratio is the stage arithmetic and the wider address range alone.  One line."""
    from pulselib_amd import _native
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    staged = NTupleTDAfterstateTFEGPU(dev, agent.n_games, max_steps=agent.max_steps, seed=agent.seed, stage_tiles=stage_tiles)
    staged.weights_dev.copy_(agent.weights_dev.repeat(staged.n_stages))
    staged.round = agent.round
    for a in (agent, staged):
        a._restart_state()
        a.start.zero_()
    common = {"games": agent.n_games, "stage_tiles": list(stage_tiles), "lambda": lam, "epsilon": agent.epsilon, "trained_rounds": agent.round,
              "max_steps": agent.max_steps, "warmup": warmup, "repeats": repeats, "weights": agent.n_weights, "staged_weights": staged.total_weights}
    zero = lambda: (agent.acc.zero_(), staged.acc.zero_())

    boards = agent.keys[min(64, agent.max_steps - 1)].clone()               # the afterstates the first agent's games recorded at their move 64

    def search_pair(a):
        q = torch.zeros((a.n_games, 4), dtype=torch.float64, device=dev)
        action, cand = torch.zeros(a.n_games, dtype=torch.int8, device=dev), torch.zeros(a.n_games, dtype=torch.uint8, device=dev)
        return lambda: a.search_launch(boards, q, action, cand)

    def learnt():                                                           # an apply launch moves what a learn launch left: both agents learn, untimed, before each
        zero()
        agent.learn_lambda_launch(lam)
        staged.learn_staged_launch(lam)
    pairs = (("rollout_layers_0", lambda: agent.rollout_from_launch(0), lambda: staged.rollout_staged_launch(0), None),
             ("learn", lambda: agent._launch("pulse_tfe_nt_learn", agent._moves(_native.TfeNtLearn())), lambda: staged.learn_staged_launch(0.0), zero),
             ("learn_lambda", lambda: agent.learn_lambda_launch(lam), lambda: staged.learn_staged_launch(lam), zero),
             ("evaluate", agent.evaluate_launch, staged.evaluate_launch, None),
             ("rollout_layers_1_backed", lambda: agent.rollout_from_launch(1, backed=True), lambda: staged.rollout_staged_launch(1, backed=True), None),
             ("learn_backed", lambda: agent.learn_backed_launch(lam), lambda: staged.learn_staged_launch(lam, backed=True), zero),
             ("evaluate_search", agent.evaluate_search_launch, staged.evaluate_search_launch, None),
             ("rollout_layers_1", lambda: agent.rollout_from_launch(1), lambda: staged.rollout_staged_launch(1), None),
             ("search", search_pair(agent), search_pair(staged), None),
             ("apply", agent.apply, staged.apply, learnt))                  # last: it moves the weights, and the slices are no longer equal
    out = {}
    for name, parent, new, before in pairs:
        seconds = _alternate(agent, torch, (("parent", parent), ("staged", new)), warmup, repeats, before=before)
        old, fresh = _spread(seconds["parent"]), _spread(seconds["staged"])
        ratio, spread = fresh["median"] / old["median"], old["max"] / old["min"]
        out[name] = {"parent_s": old, "staged_s": fresh, "ratio": ratio, "parent_spread": spread, "inside_parent_spread": 1.0 / spread <= ratio <= spread}
        if name.startswith("rollout"):                                      # equal slices: the two launches recorded the same games
            out[name]["same_games"] = bool(torch.equal(agent.lengths, staged.lengths) and torch.equal(agent.total_score, staged.total_score))
            out[name]["moves"] = int(agent.lengths.sum().item())
    zero()
    del staged
    torch.cuda.empty_cache()
    return [{"staged": {**common, **out}}]


def stage_regime_line(torch, dev, games, rounds, eval_games, max_steps, stage_tiles, lam=0.5):
    """section 13.5's regime for the unstaged agent one ply deep (the baseline of the sections before) and, under one-layer search with
    backed targets at lambda, for the unstaged agent, for stages from round 0 and for one stage added half-way by add_stage at the first
    of the stage tiles; the evaluations are from reset and paired by board.  The baseline's largest-tile histogram is in the line: it
    is what the thresholds are chosen from.  stage_tiles None: chosen here from that histogram (stage_tiles_from_hist)."""
    import numpy as np
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    out = {"games": games, "rounds": rounds, "eval_games": eval_games, "seed": 0, "max_steps": max_steps, "lambda": lam, "stage_tiles_given": stage_tiles is not None}
    ev = {}
    rows = (("layers_0", 0, False, 0.0, False, False), ("layers_1_backed_lambda", 1, True, lam, False, False),
            ("layers_1_backed_lambda_staged", 1, True, lam, True, False), ("layers_1_backed_lambda_promoted", 1, True, lam, False, True))
    for name, layers, backed, row_lam, from_round_0, promoted in rows:
        if name != "layers_0" and stage_tiles is None:                     # the baseline has been evaluated
            stage_tiles = stage_tiles_from_hist(ev["layers_0"]["one_ply"]["max_tile_hist"])
        tiles, promote = (tuple(stage_tiles) if from_round_0 else ()), (stage_tiles[0] if promoted else None)
        agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=max_steps, seed=0, lam=row_lam, stage_tiles=tiles)
        agent.rollout_layers, agent.backed_targets = layers, backed
        per_round = []
        for r in range(rounds):
            if promote is not None and r == rounds // 2:
                agent.add_stage(promote)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            agent.learn_batch()
            e[1].record()
            e[1].synchronize()
            per_round.append({"seconds": e[0].elapsed_time(e[1]) * 1e-3, "mean_length": agent.lengths.double().mean().item(),
                              "mean_score": agent.total_score.double().mean().item(), "stages": agent.n_stages})
        ev[name] = {"one_ply": agent.evaluate(n_games=eval_games, per_game=True), "search": agent.evaluate_search(n_games=eval_games, per_game=True)}
        W = agent.n_weights
        out[name] = {"rollout_layers": layers, "backed_targets": backed, "lambda": row_lam, "stage_tiles": list(agent.stage_tiles), "rounds": per_round,
                     "stats": agent.stats(), "nonzero_weights_per_stage": [int((agent.weights_dev[s * W:(s + 1) * W] != 0).sum().item()) for s in range(agent.n_stages)],
                     **{k: {"mean": e["mean_score"], "se": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "cut": e["truncated"],
                            "max_tile_hist": e["max_tile_hist"]} for k, e in ev[name].items()}}
        del agent
        torch.cuda.empty_cache()
    for name in ("layers_1_backed_lambda_staged", "layers_1_backed_lambda_promoted"):
        for other in ("layers_0", "layers_1_backed_lambda"):
            for k in ("one_ply", "search"):
                d = (ev[name][k]["total_score"] - ev[other][k]["total_score"]).astype(np.float64)
                out[f"{k}_eval_{name}_minus_{other}"] = {"mean": d.mean(), "se": d.std(ddof=1) / d.size ** .5}
    out["stage_tiles"] = list(stage_tiles)
    return {"stage_regime": out}


def stage_tiles_from_hist(hist):
    """Two stage tiles from an evaluation's largest-tile histogram (hist[k]: the games whose largest tile was 2^k): the upper one is
    the largest tile at least half the games reached, so that the last stage sees the later part of a typical game and not a few lucky
    ones; the lower one is a quarter of it, two doublings earlier, where a game is about a quarter as long."""
    games, reached = sum(hist), 0
    for k in range(15, 0, -1):
        reached += hist[k]
        if 2 * reached >= games:
            return (1 << max(k - 2, 1), 1 << max(k, 2))
    return (2, 4)


def search_line(agent, torch, games, repeats, layers=1):
    """the evaluation launch under the policies on the same weights and boards; layers = 2 adds the two-layer search and its yardstick"""
    out = {}
    policies = [("one_ply", agent.evaluate_launch), ("search", agent.evaluate_search_launch)]
    if layers == 2:
        policies.append(("search2", lambda n: agent.evaluate_search_launch(n, layers=2)))
    for name, launch in policies:
        agent.eval_counters(clear=True)
        launch(games)                                                       # untimed: the kernel's code object
        torch.cuda.synchronize()
        seconds = []
        for _ in range(repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            agent.eval_counters(clear=True)
            ev[0].record()
            launch(games)
            ev[1].record()
            ev[1].synchronize()
            seconds.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        e, s = agent.eval_counters(), _spread(seconds)
        out[name] = {"seconds": s, "moves": e["moves"], "seconds_per_move": s["median"] / e["moves"], "mean_score": e["mean_score"],
                     "std_score": e["std_score"], "mean_length": e["mean_length"], "truncated": e["truncated"]}
    line = {"games": games, "trained_rounds": agent.round, "train_games": agent.n_games, "max_steps": agent.max_steps, "repeats": repeats, **out,
            "seconds_per_move_ratio": out["search"]["seconds_per_move"] / out["one_ply"]["seconds_per_move"],
            "seconds_ratio": out["search"]["seconds"]["median"] / out["one_ply"]["seconds"]["median"]}
    if layers == 2:
        count = children_per_move(agent, torch, 32, agent.max_steps)
        ratio = out["search2"]["seconds_per_move"] / out["search"]["seconds_per_move"]
        line.update(layers=2, **count, search2_per_move_ratio=ratio, search2_over_yardstick=ratio / count["children_per_move"],
                    search2_within_margin=ratio <= 1.5 * count["children_per_move"])
    return {"search": line}


def adaptive_lines(agent, torch, games, thresholds, repeats):
    """One {"adaptive_search": ...} line per threshold E: the evaluation launch under one layer of search, under
    the adaptive search at every E and under two layers, on the same weights and boards, alternating in turn, each between its own pair
    of HIP events: one untimed pass (with its read-back: the scores per game, the counters, the moves at each depth), then `repeats`."""
    import numpy as np
    how = {"one": dict(layers=1), **{E: dict(layers=2, deep_empty_max=E) for E in thresholds}, "two": dict(layers=2)}
    scores, counters = {}, {}
    for name, kw in how.items():
        e = agent.evaluate_search(n_games=games, per_game=True, **kw)
        scores[name], counters[name] = e.pop("total_score").astype(np.float64), e
    launches = [(name, lambda kw=kw: agent.evaluate_search_launch(games, **kw)) for name, kw in how.items()]
    seconds = _alternate(agent, torch, launches, 0, repeats, before=lambda: agent.eval_counters(clear=True))

    def policy(name):
        e, t = counters[name], _spread(seconds[name])
        return {"seconds": t, "moves": e["moves"], "seconds_per_move": t["median"] / e["moves"], "mean_score": e["mean_score"],
                "se_score": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "truncated": e["truncated"]}

    def paired(a, b):
        d = scores[a] - scores[b]
        return {"mean": float(d.mean()), "se": float(d.std(ddof=1) / np.sqrt(d.size))}

    lines = []
    for E in thresholds:
        e, mine, one, two = counters[E], policy(E), policy("one"), policy("two")
        mine.update(moves_deep=e["moves_deep"], moves_shallow=e["moves_shallow"], deep_share=e["moves_deep"] / max(e["moves"], 1))
        lines.append({"adaptive_search": {"games": games, "deep_empty_max": E, "trained_rounds": agent.round, "train_games": agent.n_games,
                                          "max_steps": agent.max_steps, "repeats": repeats, "one_layer": one, "adaptive": mine, "two_layers": two,
                                          "adaptive_minus_one": paired(E, "one"), "adaptive_minus_two": paired(E, "two"),
                                          "seconds_over_one": mine["seconds"]["median"] / one["seconds"]["median"],
                                          "seconds_over_two": mine["seconds"]["median"] / two["seconds"]["median"]}})
    return lines


def adaptive_rollout_lines(agent, torch, thresholds, warmup, repeats):
    """One {"adaptive_rollout": ...} line per threshold on the boards of the agent's next round, then one
    {"adaptive_round": ...} line at the first threshold below 16"""
    board_id0 = agent.round_board_id0()
    common = {"games": agent.n_games, "epsilon": agent.epsilon, "trained_rounds": agent.round, "max_steps": agent.max_steps, "warmup": warmup, "repeats": repeats}
    lines = []
    for E in thresholds:
        mine = (("adaptive", lambda E=E: agent.rollout_adaptive_launch(E)), ("adaptive_backed", lambda E=E: agent.rollout_adaptive_launch(E, backed=True)))
        if E == 16:
            parents = (("rollout_search", lambda: agent.rollout_search_launch(2)), ("rollout_backed", lambda: agent.rollout_backed_launch(2)))
        else:
            parents = (("evaluate_adaptive", lambda E=E: agent.evaluate_search_launch(epsilon=agent.epsilon, board_id0=board_id0, layers=2, deep_empty_max=E)),)
        agent._depth_words().zero_()
        seconds = _alternate(agent, torch, parents + mine, warmup, repeats, before=lambda: agent.eval_counters(clear=True))
        deep, shallow = (x // ((warmup + repeats) * (2 if E == 16 else 3)) for x in agent.rollout_depth_summary().values())
        t = {name: _spread(xs) for name, xs in seconds.items()}
        line = {**common, "deep_empty_max": E, "moves": deep + shallow, "deep_share": deep / max(deep + shallow, 1), **{k + "_s": v for k, v in t.items()}}
        if E == 16:
            for new, old in (("adaptive", "rollout_search"), ("adaptive_backed", "rollout_backed")):
                line[new + "_over_" + old] = t[new]["median"] / t[old]["median"]
                line[new + "_inside_parent_min_max_plus_2_percent"] = t[old]["min"] / 1.02 <= t[new]["median"] <= t[old]["max"] * 1.02
        else:
            for new in ("adaptive", "adaptive_backed"):
                line[new + "_over_evaluate"] = t[new]["median"] / t["evaluate_adaptive"]["median"]
        lines.append({"adaptive_rollout": line})
    below = [E for E in thresholds if E < 16]
    if below:
        lines.append(adaptive_round_line(agent, torch, below[0], common))
    return lines


def adaptive_round_line(agent, torch, E, common):
    """roll-out + learn + apply with backed targets under one layer, two layers and two layers at E, from the same weights and boards"""
    weights, round0, saved = agent.weights_dev.clone(), agent.round, (agent.rollout_layers, agent.backed_targets, agent.rollout_deep_empty_max)
    rows, out = (("layers_1_backed", 1, None), ("layers_2_backed", 2, None), ("layers_2_adaptive_backed", 2, E)), {}
    for name, layers, threshold in rows:
        agent.rollout_layers, agent.backed_targets, agent.rollout_deep_empty_max = layers, True, threshold
        times = []
        for i in range(common["warmup"] + common["repeats"]):
            agent.weights_dev.copy_(weights)
            agent.round = round0
            t = _timed_round(agent, torch)
            if i >= common["warmup"]:
                times.append(t)
        ro, le, ap = (_spread([t[i] for t in times]) for i in range(3))
        out[name] = {"rollout_s": ro, "learn_s": le, "apply_s": ap, "round_s": _spread([sum(t) for t in times]), "moves": int(agent.lengths.sum().item())}
    agent.round = round0                                                    # the picks read the last records under their round's ids
    picks = _alternate(agent, torch, (("continue_pick", agent.continue_pick_launch), ("restart_pick", lambda: agent.restart_pick_launch(0.5, 64))),
                       common["warmup"], common["repeats"])
    agent.weights_dev.copy_(weights)
    agent.rollout_layers, agent.backed_targets, agent.rollout_deep_empty_max = saved
    agent._depth_words().zero_()
    return {"adaptive_round": {**common, "deep_empty_max": E, **out, **{k + "_s": _spread(v) for k, v in picks.items()},
                               "adaptive_over_one_layer": out["layers_2_adaptive_backed"]["round_s"]["median"] / out["layers_1_backed"]["round_s"]["median"],
                               "adaptive_over_two_layers": out["layers_2_adaptive_backed"]["round_s"]["median"] / out["layers_2_backed"]["round_s"]["median"]}}


def adaptive_regime_line(torch, dev, games, rounds, eval_games, max_steps, segment, E, lam=0.5):
    """section 13.5's regime with backed targets at lambda under one layer, under two layers and under two layers at E, the first and the last
    also continued in segments;
    a continued agent trains until it has learnt as many moves as its whole-game twin; the evaluations are from reset and paired by board"""
    import time
    import numpy as np
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    out, ev = {"games": games, "rounds": rounds, "eval_games": eval_games, "seed": 0, "max_steps": max_steps, "segment": segment, "deep_empty_max": E, "lambda": lam}, {}
    for name, layers, threshold, continued in (("layers_1", 1, None, False), ("layers_2", 2, None, False), ("adaptive", 2, E, False),
                                               ("layers_1_continued", 1, None, True), ("adaptive_continued", 2, E, True)):
        agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=segment if continued else max_steps, seed=0, lam=lam)
        agent.rollout_layers, agent.backed_targets, agent.rollout_deep_empty_max = layers, True, threshold
        if continued:
            agent.continue_games, agent.eval_max_steps = True, max_steps
        target, t0 = out[name[:-len("_continued")]]["moves_learnt"] if continued else None, time.perf_counter()
        while (agent.stats()["learnt"] < target) if continued else (agent.round < rounds):       # (synchronises once a round)
            agent.learn_batch()
        torch.cuda.synchronize(dev)
        wall, st = time.perf_counter() - t0, agent.stats()
        depth = agent.rollout_depth_summary() if threshold is not None else None
        ev[name] = {"one_ply": agent.evaluate(n_games=eval_games, per_game=True), "search": agent.evaluate_search(n_games=eval_games, per_game=True)}
        out[name] = {"rollout_layers": layers, "rollout_deep_empty_max": threshold, "continue_games": continued, "max_steps": agent.max_steps, "rounds": agent.round,
                     "wall_seconds": wall, "stats": st, "moves_learnt": st["learnt"],
                     "deep_share": None if depth is None else depth["moves_deep"] / max(depth["moves_deep"] + depth["moves_shallow"], 1),
                     "finished": agent.finished_summary()["games"] if continued else None,
                     **{k: {"mean": e["mean_score"], "se": e["std_score"] / e["games"] ** .5, "mean_length": e["mean_length"], "cut": e["truncated"]}
                        for k, e in ev[name].items()}}
        del agent
        torch.cuda.empty_cache()
    for mine, other in (("adaptive", "layers_1"), ("adaptive", "layers_2"), ("layers_2", "layers_1"), ("adaptive_continued", "layers_1_continued"),
                        ("adaptive_continued", "adaptive")):
        for k in ("one_ply", "search"):
            d = (ev[mine][k]["total_score"] - ev[other][k]["total_score"]).astype(np.float64)
            out[f"{k}_eval_{mine}_minus_{other}"] = {"mean": d.mean(), "se": d.std(ddof=1) / d.size ** .5}
    return {"adaptive_regime": out}


def exchange_line(torch, dev, games, max_steps, warmup, repeats):
    """the pack launch, the unpack launch into a second, zeroed accumulator and the apply launch on the accumulators a real learn launch
    left, each between its own pair of HIP events, in the same run"""
    from pulselib_amd import _native
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=max_steps, seed=0).set_shard(games, 0)
    side = agent._shard.side
    second, stats = torch.zeros_like(agent.acc), torch.zeros(2, dtype=torch.int64, device=dev)
    seconds, found, packed = {"pack_first": [], "pack": [], "unpack": [], "apply": []}, [], 0
    for turn in range(warmup + repeats):
        agent.rollout()
        agent.learn()
        second.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[4].record()
        side.pack()                                                         # the first reader of acc after the learn launch's scattered adds ...
        ev[0].record()
        words = side.pack()                                                 # ... and the same launch again, as the apply launch finds acc: just read
        ev[1].record()
        o = _native.TfeNtAccList()
        o.n_entries, o.acc, o.capacity, o.list, o.stats = agent.total_weights, second.data_ptr(), side.capacity, words.data_ptr(), stats.data_ptr()
        agent._launch("pulse_tfe_nt_acc_unpack", o)
        ev[2].record()
        agent.apply()
        ev[3].record()
        agent.round += 1
        ev[3].synchronize()
        packed += int(words[0].item())
        if turn >= warmup:
            for i, k in enumerate(("pack", "unpack", "apply")):
                seconds[k].append(ev[i].elapsed_time(ev[i + 1]) * 1e-3)
            seconds["pack_first"].append(ev[4].elapsed_time(ev[0]) * 1e-3)
            found.append(int(words[0].item()))
    assert stats.tolist() == [packed, 0], (stats.tolist(), packed)         # every entry of a packed list is a good one, and all were added
    spread = {k + "_s": _spread(v) for k, v in seconds.items()}
    line = {"games": games, "max_steps": max_steps, "weights": agent.total_weights, "capacity": side.capacity, "warmup": warmup, "repeats": repeats,
            "entries_found": _spread(found), "list_bytes": 32 * (1 + max(found)), "acc_bytes": 16 * agent.total_weights, **spread,
            "pack_first_over_apply": spread["pack_first_s"]["median"] / spread["apply_s"]["median"],
            "pack_over_apply": spread["pack_s"]["median"] / spread["apply_s"]["median"],
            "unpack_over_apply": spread["unpack_s"]["median"] / spread["apply_s"]["median"], "refused": stats.tolist()[1]}
    del agent, second, side
    torch.cuda.empty_cache()
    return {"exchange": line}


def _exchange_rounds(torch, dev, n_games, games, game0, max_steps, rounds):
    """(wall seconds of `rounds` rounds after one untimed, the agent): `n_games` games of a job of `games`, sharded where they are fewer"""
    import time
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    agent = NTupleTDAfterstateTFEGPU(dev, n_games, max_steps=max_steps, seed=0)
    if n_games != games:
        agent.set_shard(games, game0)
    agent.learn_batch()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(rounds):
        agent.learn_batch()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, agent


def _exchange_rank(rank, world, port, games, max_steps, rounds, out):
    import torch
    import torch.distributed as dist
    from pulselib_amd.agents import tfe_ntuple_ranks as ranks
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    ranks.init_ranks("gloo", rank, world)
    try:
        n_games, game0 = ranks.shard_of(games)
        wall, agent = _exchange_rounds(torch, torch.device("cuda:0"), n_games, games, game0, max_steps, rounds)
        out[rank] = {"wall_s": wall, "rounds": agent.exchange_summary()["rounds"][1:], "weights_nonzero": int((agent.weights_dev != 0).sum().item()),
                     "weights_sum": float(agent.weights_dev.double().sum().item())}
    finally:
        dist.destroy_process_group()


def exchange_ranks_line(torch, dev, games, max_steps, rounds, world):
    """one process on `games` games beside `world` gloo ranks on the same device and the same games: a rehearsal, not a scaling number"""
    import socket
    import torch.multiprocessing as mp
    wall, agent = _exchange_rounds(torch, dev, games, games, 0, max_steps, rounds)
    single = {"wall_s": wall, "weights_nonzero": int((agent.weights_dev != 0).sum().item()), "weights_sum": float(agent.weights_dev.double().sum().item())}
    del agent
    torch.cuda.empty_cache()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_exchange_rank, args=(world, port, games, max_steps, rounds, out), nprocs=world, join=True)
    got = [out[r] for r in range(world)]
    same = all(g["weights_nonzero"] == single["weights_nonzero"] and g["weights_sum"] == single["weights_sum"] for g in got)
    return {"exchange_ranks": {"rehearsal": "all ranks share device 0 over gloo (host tensors): says nothing about scaling", "games": games, "max_steps": max_steps,
                               "rounds": rounds, "world": world, "single_process": single, "ranks_wall_s": [g["wall_s"] for g in got],
                               "paths": [r["path"] for r in got[0]["rounds"]], "entries_per_rank": [r["entries"] for r in got[0]["rounds"]],
                               "bytes_per_round": [r["bytes"] for r in got[0]["rounds"]], "weights_equal_single_process": same}}


def lambda_line(agent, torch, lam, warmup, repeats):
    """the two learn launches on the games the agent last recorded (the agent's own lam is 0: learn() is the TD(0) launch)"""
    launches = (("learn", agent.learn), ("learn_lambda", lambda: agent.learn_lambda_launch(lam)))
    seconds = {name: [] for name, _ in launches}
    before = agent.stats()
    for i in range(warmup + repeats):
        for name, launch in launches:
            agent.acc.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            launch()
            ev[1].record()
            ev[1].synchronize()
            if i >= warmup:
                seconds[name].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    agent.acc.zero_()
    moves = (agent.stats()["learnt"] - before["learnt"]) // (2 * (warmup + repeats))
    td0, tdl = _spread(seconds["learn"]), _spread(seconds["learn_lambda"])
    return {"lambda": {"games": agent.n_games, "lambda": lam, "gamma": agent.gamma, "trained_rounds": agent.round, "max_steps": agent.max_steps,
                       "warmup": warmup, "repeats": repeats, "moves_learnt": moves, "learn_s": td0, "learn_lambda_s": tdl,
                       "overhead_s": tdl["median"] - td0["median"], "ratio": tdl["median"] / td0["median"], "walk_bytes": 17 * moves,
                       "atomics": 2 * agent.n_features * moves}}


def tc_line(agent, torch, lam, warmup, repeats):
    """the fixed-step and the temporal-coherence launches on the games the agent last recorded (the agent's own lam is 0 and its tc off:
    learn() and apply() are the TD(0) launch and the fixed-step apply)"""
    launches = [("learn", agent.learn, "apply", agent.apply), ("learn_tc", lambda: agent.learn_tc_launch(0.0), "apply_tc", agent.apply_tc_launch)]
    if lam:
        launches += [("learn_lambda", lambda: agent.learn_lambda_launch(lam), None, agent.apply),
                     ("learn_tc_lambda", lambda: agent.learn_tc_launch(lam), None, agent.apply_tc_launch)]
    agent.learn_tc_launch(0.0)                                              # untimed: allocates acc_abs, E, A and tc_stats
    weights, before = agent.weights_dev.clone(), agent.stats()
    seconds = {name: [] for row in launches for name in (row[0], row[2]) if name}
    for i in range(warmup + repeats):
        for learn_name, learn, apply_name, apply in launches:
            agent.acc.zero_()
            agent.acc_abs.zero_()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            learn()
            ev[1].record()
            apply()
            ev[2].record()
            ev[2].synchronize()
            if i >= warmup:
                seconds[learn_name].append(ev[0].elapsed_time(ev[1]) * 1e-3)
                if apply_name:
                    seconds[apply_name].append(ev[1].elapsed_time(ev[2]) * 1e-3)
    moves = (agent.stats()["learnt"] - before["learnt"]) // (len(launches) * (warmup + repeats))
    tc = agent.tc_summary()
    agent.weights_dev.copy_(weights)
    for t in (agent.acc, agent.acc_abs, agent.E, agent.A):
        t.zero_()
    out = {name + "_s": _spread(xs) for name, xs in seconds.items()}
    med = lambda name: out[name + "_s"]["median"]
    out.update(learn_ratio=med("learn_tc") / med("learn"), apply_ratio=med("apply_tc") / med("apply"),
               round_overhead_s=med("learn_tc") + med("apply_tc") - med("learn") - med("apply"))
    if lam:
        out.update(learn_lambda_ratio=med("learn_tc_lambda") / med("learn_lambda"))
    return {"tc": True, "games": agent.n_games, "lambda": lam or 0.0, "gamma": agent.gamma, "trained_rounds": agent.round, "max_steps": agent.max_steps,
            "warmup": warmup, "repeats": repeats, "moves_learnt": moves, "weights": agent.n_weights, "weights_moved_per_apply_tc": tc["moved"] // (
                (2 if lam else 1) * (warmup + repeats)), "atomics": 2 * agent.n_features * moves, "atomics_tc": 3 * agent.n_features * moves, **out}


def state_line(agent, torch, state, trained_rounds, warmup, repeats):
    agent.clear()
    for _ in range(trained_rounds if state == "trained" else 0):
        agent.learn_batch()
    times, moves = [], []
    for i in range(warmup + repeats):
        if state == "zero":
            agent.weights_dev.zero_()
        before = agent.stats()["moves"]                                     # (synchronises: outside the events)
        t = _timed_round(agent, torch)
        if i >= warmup:
            times.append(t)
            moves.append(agent.stats()["moves"] - before)
    ro, le, ap = (_spread([t[i] for t in times]) for i in range(3))
    m, F, W = statistics.mean(moves), agent.n_features, agent.n_weights
    agent.evaluate()                                                        # untimed: the evaluation kernel's code object
    evals = [_timed_evaluate(agent, torch) for _ in range(repeats)]
    ev_s, e = _spread([s for s, _ in evals]), evals[-1][1]
    st = agent.stats()
    return {"games": agent.n_games, "state": state, "tuples": [list(t) for t in agent.tuples], "features": F, "weights": W, "max_steps": agent.max_steps,
            "trained_rounds": trained_rounds if state == "trained" else 0, "warmup": warmup, "repeats": repeats,
            "rollout_s": ro, "learn_s": le, "apply_s": ap, "round_s": _spread([sum(t) for t in times]), "moves_per_round": m,
            "rollout_moves_per_s": m / ro["median"], "learn_moves_per_s": m / le["median"], "learn_atomics_per_s": 2 * F * m / le["median"],
            "apply_read_bytes_per_s": 20 * W / ap["median"], "mean_final_score_last_round": agent.total_score.double().mean().item(),
            "skipped": st["skipped"], "clamped": st["clamped"], "truncated": st["truncated"],
            "evaluate": {"seconds": ev_s, "moves": e["moves"], "moves_per_s": e["moves"] / ev_s["median"], "mean_score": e["mean_score"],
                         "std_score": e["std_score"], "mean_length": e["mean_length"], "truncated": e["truncated"]}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--states", nargs="+", default=["zero", "trained"], choices=["zero", "trained"])
    ap.add_argument("--trained-rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--search", action="store_true", help="one more line per B: the evaluation under search beside the one-ply one")
    ap.add_argument("--search-games", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--layers", type=int, default=1, choices=[1, 2], help="with --search, 2: the two-layer evaluation and its child count beside the other two")
    ap.add_argument("--deep-empty-max", type=int, nargs="+", metavar="E",
                    help="with --search --layers 2: one more line per B and E, the evaluation under the search two layers deep on boards with at most E empty cells beside one and two layers")
    ap.add_argument("--lambda", dest="lam", type=float, help="one more line per B: the TD(lambda) learn launch beside the TD(0) one, on the same games")
    ap.add_argument("--tc", action="store_true", help="one more line per B: the temporal-coherence learn and apply launches beside the fixed-step ones")
    ap.add_argument("--train-layers", type=int, choices=[1, 2], help="one more line per B: the recording launch under search beside the evaluation under it")
    ap.add_argument("--train-deep-empty-max", type=int, nargs="+", metavar="E",
                    help="with --train-layers 2: one more line per B and E, the recording launch at the adaptive depth beside its parents (E = 16) or the evaluation at E")
    ap.add_argument("--adaptive-regime", action="store_true", help="one line instead: backed rounds under one layer and at the adaptive depth, whole games and continued (DESIGN.md section 13.13)")
    ap.add_argument("--backed", action="store_true", help="with --train-layers: two more lines per B, the backed recording launch and the backed learner beside the parent's")
    ap.add_argument("--backed-regime", action="store_true", help="one line instead: twelve rounds and paired evaluations of the four agents of DESIGN.md section 13.6")
    ap.add_argument("--restart", type=float, metavar="F", help="two more lines per B: the restarted recording launch beside its three parents, and the pick launch at this fraction")
    ap.add_argument("--restart-min-length", type=int, default=64)
    ap.add_argument("--restart-regime", action="store_true", help="one line instead: twelve rounds and paired evaluations with and without restart (DESIGN.md section 13.7)")
    ap.add_argument("--stages", default="", metavar="TILES", help="one more line per B: every staged launch beside its unstaged sibling, stages at these tiles (512,2048), equal slices")
    ap.add_argument("--stage-regime", action="store_true", help="one line instead: twelve rounds and paired evaluations without stages, with --stages from round 0 and with one added half-way (DESIGN.md section 13.9)")
    ap.add_argument("--continue-games", action="store_true", help="one line per B instead: the continue pick launch beside the restart pick (DESIGN.md section 13.10)")
    ap.add_argument("--continue-regime", action="store_true", help="one line instead: twelve whole-game rounds beside continued rounds of --continue-max-steps moves to the same moves learnt")
    ap.add_argument("--continue-max-steps", type=int, default=64, metavar="K", help="with --continue-games / --continue-regime: the segment length")
    ap.add_argument("--continue-rounds", type=int, default=16, help="with --continue-games: the continued rounds played before the picks are timed")
    ap.add_argument("--exchange", action="store_true", help="two lines instead: the pack and unpack launches of the accumulator exchange beside the apply launch (DESIGN.md section 13.14)")
    ap.add_argument("--exchange-ranks", type=int, default=0, metavar="R", help="with --exchange: one more line, rounds on R gloo ranks sharing device 0 beside one process (a rehearsal)")
    ap.add_argument("--regime-rounds", type=int, default=12)
    ap.add_argument("--regime-eval-games", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfe_mc", "bench_tfe_ntuple.jsonl"))
    args = ap.parse_args(argv)
    if args.backed and not args.train_layers:
        ap.error("--backed needs --train-layers 1 or 2: the backed-up values are the search's")
    if args.train_deep_empty_max and args.train_layers != 2 and not args.adaptive_regime:
        ap.error("--train-deep-empty-max needs --train-layers 2: it says on which boards the roll-out's search looks two chance layers ahead")
    if args.train_deep_empty_max and not all(0 <= E <= 16 for E in args.train_deep_empty_max):
        ap.error("--train-deep-empty-max takes thresholds in 0..16")
    if args.deep_empty_max and not (args.search and args.layers == 2):
        ap.error("--deep-empty-max needs --search --layers 2: it says on which boards the search looks two chance layers ahead")
    if args.deep_empty_max and not all(0 <= E <= 16 for E in args.deep_empty_max):
        ap.error("--deep-empty-max takes thresholds in 0..16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfe_ntuple needs the MI355X: no timing is taken on a CPU")
    from pulselib_amd.agents import NTupleTDAfterstateTFEGPU
    from pulselib_amd.agents.tfe_ntuple_td_gpu import DEFAULT_TUPLES, tuple_offsets
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.exchange:
        games = args.games[0] if "--games" in (sys.argv if argv is None else argv) else 4096
        lines = [exchange_line(torch, dev, games, ms, args.warmup, args.repeats) for ms in (64, args.max_steps)]
        if args.exchange_ranks > 1:
            lines.append(exchange_ranks_line(torch, dev, games, 64, args.regime_rounds, args.exchange_ranks))
        for line in lines:
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        return
    if args.adaptive_regime:
        line = adaptive_regime_line(torch, dev, args.games[0], args.regime_rounds, args.regime_eval_games, args.max_steps, args.continue_max_steps,
                                    (args.train_deep_empty_max or [3])[0])
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        return
    if args.backed_regime:
        line = backed_regime_line(torch, dev, args.games[0], args.regime_rounds, args.regime_eval_games, args.max_steps)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        return
    stage_tiles = tuple(int(t) for t in args.stages.split(",") if t)
    if args.stage_regime:
        line = stage_regime_line(torch, dev, args.games[0], args.regime_rounds, args.regime_eval_games, args.max_steps, stage_tiles or None)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        return
    if args.restart_regime:
        line = restart_regime_line(torch, dev, args.games[0], args.regime_rounds, args.regime_eval_games, args.max_steps,
                                   0.5 if args.restart is None else args.restart, args.restart_min_length)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        return
    if args.continue_regime or args.continue_games:
        lines = [continue_regime_line(torch, dev, args.games[0], args.regime_rounds, args.regime_eval_games, args.max_steps, args.continue_max_steps)] \
            if args.continue_regime else [continue_pick_line(torch, dev, g, args.continue_max_steps, args.continue_rounds, args.warmup, args.repeats) for g in args.games]
        for line in lines:
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")
        return
    for games in args.games:
        per_move = 33 if args.backed or args.restart or args.train_deep_empty_max else 17 if args.lam is None else 25
        need = (48 if args.tc else 20) * tuple_offsets(DEFAULT_TUPLES)[1] + per_move * games * args.max_steps + 64 * games
        if stage_tiles:                                                     # a second agent: the staged weights and records of its own
            need = 2 * 33 * games * args.max_steps + (48 if args.tc else 20) * (len(stage_tiles) + 2) * tuple_offsets(DEFAULT_TUPLES)[1] + 128 * games
        free = torch.cuda.mem_get_info(dev)[0]
        if need > 0.9 * free:
            lines = [{"games": games, "skipped": f"needs {need} bytes of device memory, {free} are free"}]
        else:
            agent = NTupleTDAfterstateTFEGPU(dev, games, max_steps=args.max_steps, seed=0)
            lines = [state_line(agent, torch, s, args.trained_rounds, args.warmup, args.repeats) for s in args.states]
            if args.search:                                                 # on the weights the last state left
                lines += [search_line(agent, torch, g, args.repeats, args.layers) for g in args.search_games]
            if args.deep_empty_max:                                         # likewise
                lines += [line for g in args.search_games for line in adaptive_lines(agent, torch, g, args.deep_empty_max, args.repeats)]
            if args.lam is not None:                                        # on the games the last timed round recorded
                lines.append(lambda_line(agent, torch, args.lam, args.warmup, args.repeats))
            if args.tc:                                                     # likewise
                lines.append(tc_line(agent, torch, args.lam, args.warmup, args.repeats))
            if args.train_deep_empty_max:                                   # on the weights the last state left; instead of the line of section 13.5
                lines += adaptive_rollout_lines(agent, torch, args.train_deep_empty_max, args.warmup, args.repeats)
            elif args.train_layers:                                         # on the weights the last state left
                lines.append(train_rollout_line(agent, torch, args.train_layers, args.warmup, args.repeats))
            if args.backed:                                                 # likewise, then on the records of its own last launch
                lines += backed_lines(agent, torch, args.train_layers, args.lam or 0.0, args.warmup, args.repeats)
            if args.restart:                                                # on the weights the last state left
                lines += restart_lines(agent, torch, args.restart, args.restart_min_length, args.warmup, args.repeats)
            if stage_tiles:                                                 # likewise
                lines += staged_lines(agent, torch, dev, stage_tiles, 0.5 if args.lam is None else args.lam, args.warmup, args.repeats)
            del agent
            torch.cuda.empty_cache()
        for line in lines:
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
