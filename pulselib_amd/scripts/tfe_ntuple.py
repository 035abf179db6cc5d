"""An n-tuple network for 2048 on the 4 x 4 board, trained by batch TD(0) on afterstates with the whole loop on the device
(agents/tfe_ntuple_td_gpu.py; which flags go together: check_options of agents/tfe_ntuple_host.py, section 13.12): every round is a roll-out launch of `--tables` whole games under the network,
a learn launch of one lane per recorded move and an apply launch over the weights.  Defaults: the network of two rows and two 2 x 3
rectangles over the board's eight images, gamma 1, epsilon 0, alpha 1.  Every `--eval-every` rounds (default: every round) it
prints, from ONE evaluation launch of `--eval-games` games under the greedy policy on the same boards every time: the mean final
score and its standard error, the mean length and the histogram of the largest tile.  `--save PATH` writes the non-zero weights and
the run's state at the end, `--resume PATH` continues such a run for `--rounds` more rounds.  `--search`: every evaluation also runs
under expectimax search one chance layer deep (section 13.1) on the same boards, and both means are printed; `--resume PATH --rounds 0
--search` plays a saved network; `--search --layers 2` searches two chance layers deep (section 13.4), with `--deep-empty-max E` only on the boards with at most E empty cells and one layer on the others (section 13.11; the line says what share of the moves went deep; not with `--stages`).  `--lambda L` (0 < L <= 1) learns by TD(lambda) (section 13.2): the learn launch walks every game
backwards first and adds lambda-differences; the run's first line names it, and `--resume` takes it from the file.  `--tc` learns with temporal-coherence
step sizes (section 13.3): every weight moves by rho = |E| / A of the step, from the running sums of its errors; the round's mean rho
is printed beside the round's counters, and `--resume` takes `tc` from the file too.  `--train-layers L` (1 or 2; section 13.5) plays the
rounds' own games under expectimax search L chance layers deep, recorded and learnt from as before; every round's line carries the mean
score and length of the games it trained on; no checkpoint holds the option, so `--resume` needs it given again.  `--backed` (with
`--train-layers 1` or `2`; section 13.6) also records the value the search backed up for every move's board and learns towards it:
a move's difference is backed[t + 1] - V_t, under the run's `--lambda` and `--tc`; not saved either.  `--restart F` (0 < F < 1;
section 13.7; not with `--train-layers 2`) starts every game of a round on the board its predecessor of the round before stood on at
the fraction F of its length, where that game had at least `--restart-min-length` moves: every round's line says how many of its games
were restarted and from what mean depth -- a restarted game's score counts from its start board and is not comparable with a whole
game's; the evaluations stay from reset.  Not saved either: a resumed run's first round starts at the reset boards.  `--stages 512,2048`
(section 13.9) keeps one weight set per tile stage -- a board reads and learns in the set of the largest of those tiles it has reached --
and `--add-stage ROUND:TILE` splits a stage at TILE before round ROUND, the new set starting as a copy (weight promotion); not with
`--train-layers 2` or `--search --layers 2`; the file holds the stages, and `--resume` takes them from it.  `--continue-games` with
`--max-steps K` (K >= 2, small: 64; section 13.10; not with `--restart` nor `--train-layers 2`) plays K moves of every game per round
and takes the cut games up again in the next round under the new weights, so the weights move every K moves of a game instead of once
per generation of games; the evaluations are capped at 4,096 moves, not at K, and every round's line says how many whole games
finished since the last line, their mean score and length, and how many games the round's pick continued: the training curve of
complete games.  Not saved either: a resumed run's games begin at their resets.  `--train-layers 2 --train-deep-empty-max E` (E in
0..16; section 13.13; not with `--stages`) plays the rounds' own games under the search whose depth the board chooses: two chance
layers where the board a move is made from has at most E empty cells and one elsewhere, recorded and learnt from as before; it goes
with `--backed`, with `--continue-games --max-steps K` and with `--restart F`, which `--train-layers 2` alone does not; every round's
line says what share of the training moves since the last line went deep.  Not saved either.  `--ranks R` (section 13.14) plays
every round on R ranks, one fresh process and one device each (or run the module under torch.distributed.run, which sets RANK and
WORLD_SIZE): `--tables` and `--eval-games` are the job's counts, every rank plays its share of the same boards, the ranks' accumulators
are summed between the learn and the apply launch (a sparse list of the touched cells; one host read per round), and the weights
stay identical on all ranks and equal to those of one process -- exactly.  Rank 0 prints and saves; the training scores of a line are
rank 0's share, every other number is the job's.  `--ranks-one-device` puts all ranks on device 0 over gloo: a rehearsal of the
protocol, not of its speed.  `--resume` with `--ranks` takes the file's weights and round; the file's n_games is the saving rank's share."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import torch

from ..agents import NTupleTDAfterstateTFEGPU
from ..agents.tfe_ntuple_host import check_options

CONTINUE_EVAL_MAX_STEPS = 4096                                             # --continue-games: the evaluations' cap (max_steps is the segment's length)


def _promotions(add_stage, first, rounds) -> dict:
    """{round: the tile a stage is split at before it} of --add-stage's (round, tile) pairs; ValueError for a round named twice or
    outside the rounds first .. first + rounds - 1 this run plays: neither is passed over in silence."""
    add_stage = tuple((int(r), int(tile)) for r, tile in add_stage)
    promotions = dict(add_stage)
    if len(promotions) != len(add_stage):
        raise ValueError("--add-stage names a round twice: one stage is split before a round")
    outside = sorted(r for r in promotions if not first <= r < first + rounds)
    if outside:
        raise ValueError(f"--add-stage rounds {outside} are outside the rounds this run plays, {first}..{first + rounds - 1}")
    return promotions


def run(device, rounds, tables=65536, alpha=1.0, epsilon=0.0, gamma=1.0, seed=0, max_steps=4096, eval_every=1, eval_games=None, save=None,
        resume=None, out=print, search=False, lam=0.0, tc=False, layers=1, train_layers=0, backed=False, restart=0.0, restart_min_length=64, stages=(), add_stage=(),
        continue_games=False, deep_empty_max=None, train_deep_empty_max=None, shard=False):
    check_options(train_layers, backed, restart, continue_games, max_steps, bool(stages or add_stage), search=search, layers=layers,
                  deep_empty_max=deep_empty_max, rollout_deep_empty_max=train_deep_empty_max, script=True)     # (refused before a device is asked for)
    job_tables, game0 = tables, 0
    if shard:                                                               # (torch.distributed is initialised: main's _join_ranks)
        from ..agents.tfe_ntuple_ranks import shard_of
        tables, game0 = shard_of(job_tables)
    if resume:
        agent = NTupleTDAfterstateTFEGPU.load(resume, device, n_games=tables if shard else None)
        want = dict(n_games=tables, alpha=float(alpha), epsilon=float(epsilon), gamma=float(gamma), max_steps=max_steps, seed=seed)
        differ = {k: (getattr(agent, k), v) for k, v in want.items() if getattr(agent, k) != v}
        if differ:
            raise ValueError(f"{resume} continues another run: (saved, asked) {differ}")
    else:
        _promotions(add_stage, 0, rounds)                                   # (refused before a device is asked for)
        agent = NTupleTDAfterstateTFEGPU(device, tables, gamma=gamma, epsilon=epsilon, alpha=alpha, max_steps=max_steps, seed=seed, lam=lam, tc=tc,
                                         stage_tiles=tuple(stages))
    if shard:
        agent.set_shard(job_tables, game0)
    promotions = _promotions(add_stage, agent.round, rounds)
    agent.rollout_layers, agent.backed_targets = train_layers, bool(backed)  # (no checkpoint holds them: given again on --resume)
    agent.rollout_deep_empty_max = train_deep_empty_max
    agent.restart_fraction, agent.restart_min_length = float(restart), int(restart_min_length)
    if continue_games:                                                      # (not saved: given again on --resume; the games begin at their resets)
        agent.continue_games, agent.eval_max_steps = True, CONTINUE_EVAL_MAX_STEPS
    out(f"{f'rank 0 of a job of {job_tables} games per round: ' if shard else ''}{agent.n_games} games per round from round {agent.round}: alpha {agent.alpha}, epsilon {agent.epsilon}, gamma {agent.gamma}, "
        f"lambda {agent.lam}, tc {agent.tc}, max_steps {agent.max_steps}, seed {agent.seed}, roll-out under {agent.rollout_layers} chance layers of search"
        f"{'' if train_deep_empty_max is None else f' on boards with at most {train_deep_empty_max} empty cells and one on the others'}"
        f"{', learning towards the search-backed values' if agent.backed_targets else ''}"
        f"{f', games restarted at {agent.restart_fraction} of games of {agent.restart_min_length} moves or more' if agent.restart_fraction else ''}"
        f"{f', weight sets by stage from tiles {agent.stage_tiles}' if agent.stage_tiles else ''}"
        f"{f', games continued across rounds in segments of {agent.max_steps} moves, evaluations capped at {agent.eval_max_steps}' if agent.continue_games else ''}")
    first, moves_before, t0 = agent.round, agent.stats()["moves"], time.perf_counter()

    def under_search():
        if not search:
            return ""
        e = agent.evaluate_search(n_games=eval_games, layers=layers, deep_empty_max=deep_empty_max)
        depth = "" if deep_empty_max is None else (f" on boards with at most {deep_empty_max} empty cells and one on the others "
                                                   f"(deep share {e['moves_deep'] / max(e['moves'], 1):.4f} of {e['moves']} moves)")
        return (f"; under search{'' if layers == 1 else f' of {layers} chance layers'}{depth}: Avg final score: {e['mean_score']:.1f} +- {e['std_score'] / e['games'] ** .5:.1f}, Highest: {e['max_score']}, "
                f"Avg length: {e['mean_length']:.1f}, cut {e['truncated']}, largest tile 2^k: {e['max_tile_hist']}")

    def evaluation():
        e = agent.evaluate(n_games=eval_games)                              # (synchronises)
        return (f"greedy policy over {e['games']} games: Avg final score: {e['mean_score']:.1f} +- {e['std_score'] / e['games'] ** .5:.1f}, "
                f"Highest: {e['max_score']}, Avg length: {e['mean_length']:.1f}, cut {e['truncated']}, largest tile 2^k: {e['max_tile_hist']}")

    if not rounds and search:
        out(f"After {agent.round} rounds: {evaluation()}{under_search()}")
    restarted = dict(picked=0, mean_depth=0.0)                            # of the round being played: what the round before picked
    for r in range(first, first + rounds):
        if r in promotions:
            agent.add_stage(promotions[r])
            out(f"Round {r}: a stage split at tile {promotions[r]}: stages from tiles {agent.stage_tiles}")
        agent.learn_batch()
        began, restarted = restarted, (agent.restart_summary() if agent.restart_fraction else restarted)     # (synchronises)
        if eval_every and ((r + 1) % eval_every == 0 or r + 1 == first + rounds):
            line = evaluation()
            st, now = agent.stats(), time.perf_counter()
            again = f"restarted {began['picked']} games from mean depth {began['mean_depth']:.1f}, " if agent.restart_fraction else ""
            rho = f", mean rho {agent.tc_summary()['mean_rho']:.4f}" if agent.tc else ""       # (of the applies since the last line)
            if train_deep_empty_max is not None:                            # (of the roll-outs since the last line; synchronises)
                d = agent.rollout_depth_summary()
                rho += f", deep share {d['moves_deep'] / max(d['moves_deep'] + d['moves_shallow'], 1):.4f} of {d['moves_deep'] + d['moves_shallow']} training moves"
            if agent.continue_games:                                        # (the whole games that ended since the last line; synchronises)
                done = agent.finished_summary()
                again = (f"whole games finished {done['games']}: Avg final score {done['mean_score']:.1f}, Avg length {done['mean_length']:.1f}, "
                         f"games continued {done['continued']}; per segment: ")
            out(f"Round {r}: {line}; "
                f"training: {again if agent.continue_games else ''}Avg final score {agent.total_score.double().mean().item():.1f}, Avg length {agent.lengths.double().mean().item():.1f}, {'' if agent.continue_games else again}moves/sec {(st['moves'] - moves_before) / (now - t0):.0f}, "
                f"skipped {st['skipped']}, clamped {st['clamped']}{rho}{under_search()}")
            if train_deep_empty_max is not None:
                agent.depth_stats.zero_()                                   # (an adaptive evaluation leaves its own moves there)
            moves_before, t0 = st["moves"], time.perf_counter()
    if save:
        agent.save(save)
    return agent


def _spawn_ranks(argv, ranks) -> int:
    """`ranks` fresh processes of this module with `argv`, rank r with RANK = LOCAL_RANK = r; the largest exit status."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    children = [subprocess.Popen([sys.executable, "-m", "pulselib_amd.scripts.tfe_ntuple"] + list(argv), env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
                for r in range(ranks)]
    return max(abs(c.wait()) for c in children)


def _join_ranks(one_device):
    """This process as the rank RANK of WORLD_SIZE (set by _spawn_ranks or torch.distributed.run): the group initialised -- gloo with
    all ranks on device 0, else nccl (RCCL) with rank r on device LOCAL_RANK -- and (the device, the rank)."""
    from ..agents.tfe_ntuple_ranks import init_ranks
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = torch.device("cuda", 0 if one_device else int(os.environ.get("LOCAL_RANK", rank)))
    torch.cuda.set_device(device)
    init_ranks("gloo" if one_device else "nccl", rank, world)
    return device, rank


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--ranks", type=int, default=1, metavar="R", help="play every round on R ranks, one process and one device each; --tables is the job's count")
    ap.add_argument("--ranks-one-device", action="store_true", help="with --ranks: all ranks on device 0 over gloo (a rehearsal of the protocol)")
    ap.add_argument("--tables", type=int, default=65536, help="games per round (one update of the weights per round)")
    ap.add_argument("--rounds", type=int, default=16)
    ap.add_argument("--alpha", type=float, default=1.0, help="a weight moves by alpha / F of the mean temporal difference of its visits")
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.0, metavar="L",
                    help="TD(lambda): credit decays by gamma * L per move back along the game (0: TD(0)); --resume takes it from the file")
    ap.add_argument("--tc", action="store_true", help="temporal-coherence step sizes: a weight moves by |E| / A of the step; --resume takes it from the file")
    ap.add_argument("--max-steps", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-every", type=int, default=1, help="rounds between evaluations of the greedy policy (0: never)")
    ap.add_argument("--eval-games", type=int, help="games per evaluation (default: --tables)")
    ap.add_argument("--save", metavar="PATH", help="write the non-zero weights and the run's state to this .npz at the end")
    ap.add_argument("--resume", metavar="PATH", help="continue the run saved there (the same --tables, --alpha, --epsilon, --gamma, --max-steps, --seed)")
    ap.add_argument("--search", action="store_true", help="every evaluation also under expectimax search, one chance layer deep")
    ap.add_argument("--layers", type=int, default=1, choices=[1, 2], help="with --search: the chance layers the search looks ahead")
    ap.add_argument("--deep-empty-max", type=int, metavar="E",
                    help="with --search --layers 2: two chance layers only on boards with at most E empty cells (0..16), one on the others; not with --stages")
    ap.add_argument("--train-layers", type=int, default=0, choices=[0, 1, 2],
                    help="the chance layers of search the rounds' own games are played under (0: the one-ply roll-out); not saved: give it again with --resume")
    ap.add_argument("--train-deep-empty-max", type=int, metavar="E",
                    help="with --train-layers 2: the rounds' games search two chance layers only on boards with at most E empty cells (0..16), one on the "
                         "others; goes with --backed, --continue-games and --restart; not with --stages; not saved")
    ap.add_argument("--backed", action="store_true",
                    help="with --train-layers 1 or 2: learn towards the value the search backed up instead of r + gamma * V of the next record; not saved")
    ap.add_argument("--restart", type=float, default=0.0, metavar="F",
                    help="start every game on the board its predecessor stood on at this fraction of its length (0: off; not with --train-layers 2); not saved")
    ap.add_argument("--restart-min-length", type=int, default=64, metavar="N", help="with --restart: only games of at least N moves are restarted from")
    ap.add_argument("--continue-games", action="store_true",
                    help="with a small --max-steps K: a game cut after K moves is taken up again by the next round under the new weights "
                         "(not with --restart nor --train-layers 2); evaluations are capped at 4096 moves; not saved")
    ap.add_argument("--stages", default="", metavar="TILES", help="weight sets by tile stage: up to three increasing tiles, e.g. 512,2048; --resume takes them from the file")
    ap.add_argument("--add-stage", action="append", default=[], metavar="ROUND:TILE", help="split a stage at TILE before round ROUND (weight promotion); repeatable")
    args = ap.parse_args(argv)
    try:
        stages = tuple(int(t) for t in args.stages.split(",") if t)
        add_stage = tuple(tuple(int(x) for x in item.split(":")) for item in args.add_stage)
        if any(len(item) != 2 for item in add_stage):
            raise ValueError
    except ValueError:
        ap.error("--stages takes tiles as 512,2048 and --add-stage ROUND:TILE")
    if len({r for r, _ in add_stage}) != len(add_stage):
        ap.error("--add-stage names a round twice: one stage is split before a round")
    if args.deep_empty_max is not None:
        if not 0 <= args.deep_empty_max <= 16:
            ap.error("--deep-empty-max must be in 0..16")
    if args.train_deep_empty_max is not None:
        if not 0 <= args.train_deep_empty_max <= 16:
            ap.error("--train-deep-empty-max must be in 0..16")
    try:                                                                    # (run()'s refusals, as the command line's)
        check_options(args.train_layers, args.backed, args.restart, args.continue_games, args.max_steps, bool(stages or add_stage),
                      search=args.search, layers=args.layers, deep_empty_max=args.deep_empty_max, rollout_deep_empty_max=args.train_deep_empty_max,
                      script=True)
    except ValueError as refused:
        ap.error(str(refused))
    device, rank, sharded = torch.device("cuda"), 0, "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1
    if args.ranks < 1 or (args.ranks_one_device and args.ranks < 2 and not sharded):
        ap.error("--ranks must be positive, and --ranks-one-device needs --ranks 2 or more")
    if args.ranks > 1 and not sharded:                                      # the parent: one fresh process per rank, and nothing else
        sys.exit(_spawn_ranks(sys.argv[1:] if argv is None else argv, args.ranks))
    if sharded:
        device, rank = _join_ranks(args.ranks_one_device)
    quiet = (lambda *a: None) if rank else print                            # rank 0 prints and saves
    agent = run(device, args.rounds, args.tables, args.alpha, args.epsilon, args.gamma, args.seed, args.max_steps, args.eval_every,
                args.eval_games, None if rank else args.save, args.resume, out=quiet, shard=sharded, search=args.search, lam=args.lam, tc=args.tc, layers=args.layers, train_layers=args.train_layers, backed=args.backed,
                restart=args.restart, restart_min_length=args.restart_min_length, stages=stages, add_stage=add_stage,
                continue_games=args.continue_games, deep_empty_max=args.deep_empty_max, train_deep_empty_max=args.train_deep_empty_max)
    st = agent.stats()
    if sharded:
        torch.distributed.destroy_process_group()
    if rank:
        return
    print(f"{agent.round * args.tables} games in {agent.round} rounds, {st['moves']} moves, alpha {args.alpha}, epsilon {args.epsilon}: "
          f"{int((agent.weights_dev != 0).sum().item())} of {agent.total_weights} weights are not zero")


if __name__ == "__main__":
    main()
