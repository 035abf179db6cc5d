"""2048 on 4 x 4: the device agent of the n-tuple network, trained by batch TD(0) -- or, with `lam`, TD(lambda) -- on afterstates
(DESIGN.md sections 13 and 13.2; csrc/tfe_ntuple.hip, csrc/tfe_ntuple_lambda.hip).  What the launches compute is stated in
tfe_ntuple_host.py, the file an agent saves in tfe_ntuple_checkpoint.py; every public name of both is a name of this module too.

A round is three launches and nothing read back in between: `pulse_tfe_nt_rollout` plays `n_games` whole games, one lane each, greedily
(or epsilon-greedily) on reward + gamma * V among the moves that change the board, and records per move the afterstate's key, its V and
one byte; `pulse_tfe_nt_learn` runs one lane per recorded move and adds the temporal difference as a fixed-point integer into {sum, cnt}
of every weight the afterstate reads; `pulse_tfe_nt_apply` moves every visited weight by alpha / F of the MEAN of its adds and zeroes the
accumulators.  `pulse_tfe_nt_evaluate` plays games without a trajectory and reduces the scores in the launch.  The opt-ins, each the
agent as it was while it is off:
  search (sections 13.1, 13.4, 13.11): `pulse_tfe_nt_search` and `pulse_tfe_nt_evaluate_search` play under expectimax search one chance
    layer deep, 32 lanes per board; with `layers=2` the `..._deep` entry points search two, 256 lanes per board; with `layers=2,
    deep_empty_max=E` the `..._adaptive` ones search two on the boards with at most E empty cells and one on the others;
  `lam` > 0 (13.2): the learn launch is `pulse_tfe_nt_learn_lambda`: one lane per game walks the recorded game backwards and leaves the
    lambda-differences in `deltas`, and the same one-lane-per-move adds follow with them;
  `tc` (13.3; csrc/tfe_ntuple_tc.hip): every weight has a step size of its own, rho = |E| / A: `pulse_tfe_nt_learn_tc` also adds |d|
    into a third accumulator, and apply is `pulse_tfe_nt_apply_tc`;
  `rollout_layers` = 1 or 2 (13.5): the round's games are played under that search, `pulse_tfe_nt_rollout_search`, and recorded alike;
  `backed_targets` (13.6; csrc/tfe_ntuple_backed.hip): a round under search also records the value the search backed up for every
    move's board (`pulse_tfe_nt_rollout_backed`), and `pulse_tfe_nt_learn_backed` learns towards backed[t + 1] - V_t;
  `restart_fraction` > 0 (13.7; csrc/tfe_ntuple_restart.hip): `learn_batch` ends with `pulse_tfe_nt_restart_pick`, which writes into
    `start` the board every long enough game stood on at that fraction of its length; the next round begins there
    (`pulse_tfe_nt_rollout_from`);
  `stage_tiles` (13.9; csrc/tfe_ntuple_staged.hip): S = len(stage_tiles) + 1 copies of the tables, a board reading and learning in the
    copy of its stage, through the four `pulse_tfe_nt_*_staged` entry points and one apply launch per stage; `add_stage` splits one;
  `continue_games` (13.10; csrc/tfe_ntuple_continue.hip): with a small `max_steps` = K a round plays K moves of every game, and
    `pulse_tfe_nt_continue_pick` puts the cut games' boards into `start`, their scores so far into the carries and the ended games
    into `finished`; `eval_max_steps` gives the evaluations a cap of their own;
  `rollout_deep_empty_max` = E (13.13; csrc/tfe_ntuple_search_rollout.hip): with `rollout_layers` 2 the round's games are played and
    recorded by `pulse_tfe_nt_rollout_adaptive`, two layers deep on the boards with at most E empty cells and one on the others, with
    the backed values and from `start` where those are on;
  `set_shard` (13.14; csrc/tfe_ntuple_exchange.hip, tfe_ntuple_ranks.py): the agent plays a rank's share of the job's games, and
    `learn_batch` sums the ranks' accumulators between learn and apply (`exchange`: `pulse_tfe_nt_acc_pack`, an all-gather of the
    lists, `pulse_tfe_nt_acc_unpack`), so every rank applies what one process would have applied.
Which of them go together is `check_options`' to say (13.12), and the agent asks it before it touches anything."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native
from .tfe_common import (AGENT_KEY, EVAL_BINS, TIE_KEY, _TFEGamesGPU, greedy_scan_many_on_host, philox_many_on_host,  # noqa: F401 (re-exported)
                         rewards_of_scores, transforms_on_host, unpack_steps)
from .tfe_ntuple_checkpoint import *                                       # noqa: F401,F403 (re-exported, as the host's names are)
from .tfe_ntuple_host import *                                             # noqa: F401,F403


class NTupleTDAfterstateTFEGPU(_TFEGamesGPU):
    """`learn_batch` = `rollout` + `learn` + `apply` + `round += 1`: three launches and no synchronisation.  Everything that reads
    back (`weights`, `stats`, `trajectory`, `evaluate`, the per-game arrays' `.cpu()`) synchronises.  Round r plays the boards
    board_id0 + r * n_games + g, so no two rounds replay the same spawns.  `lam` > 0: `learn` is the TD(lambda) launch and the agent
    holds `deltas`, float64 in the shape of `values`; `lam` = 0 (the default) allocates nothing more and learns by TD(0).  `tc`:
    temporal-coherence step sizes (section 13.3): `learn` is pulse_tfe_nt_learn_tc under the agent's `lam`, `apply` is
    pulse_tfe_nt_apply_tc, and the agent holds `acc_abs`, `E`, `A` and `tc_stats`; without it (the default) none of them exists.
    `rollout_layers` (an attribute, 0 by default; section 13.5): 1 or 2 and `rollout`, so `learn_batch`, plays its games under
    expectimax search that many chance layers deep and records them as before; it is how rounds are played, not part of the network,
    so no checkpoint holds it.  `backed_targets` (an attribute, False by default; section 13.6): with `rollout_layers` 1 or 2, `rollout`
    also records the search's backed-up value of every move's board in `backed` (float64 in the shape of `values`, allocated at the
    first such launch) and `learn` is pulse_tfe_nt_learn_backed under the agent's `lam` and `tc`; it says how rounds are learnt, so
    no checkpoint holds it either.  `restart_fraction` (an attribute, 0.0 by default: off; section 13.7): in (0, 1) and `learn_batch`
    ends with the pick launch, which fills `start` (uint64[n_games], allocated at first use, as `restart_stats` int64[2] is) from the
    games of at least `restart_min_length` moves (an attribute, 64 by default: a starting point, not tuned), and `rollout` starts the
    next round's games there; with `rollout_layers` 2 it is refused.  No checkpoint holds either, and `start` is not saved: a loaded
    agent's next round starts at the reset boards.  `stage_tiles` (section 13.9; () by default: the agent as it was, launches, allocations
    and checkpoint files): up to three tiles, powers of two, strictly increasing, at which the stages 1, 2, ... begin.  `weights_dev`,
    `acc` and the TC state then hold S * W words, stage s in [s * W, (s + 1) * W) with W = `n_weights`; rollout, learn, evaluate,
    evaluate_search and search go through the `pulse_tfe_nt_*_staged` entry points under the agent's `lam`, `tc`, `rollout_layers` 0 or
    1, `backed_targets` and `restart_fraction`, and apply is one launch per stage; two chance layers are refused (ValueError, before
    anything is touched).  `tuples` carries the stage tiles (with_stages), so the host mirrors handed `agent.tuples` read by stage.
    `continue_games` (an attribute, False by default: the agent as it was; section 13.10): on an agent built with a small `max_steps`
    = K >= 2, a game a round cuts at K moves is taken up again by the next round instead of being reset: `learn_batch` ends with the
    continue pick, a fourth launch, which fills `start` with the board the cut move was made on, and `rollout` plays from `start`
    (rollout_from_launch, or the staged launch) at `rollout_layers` 0 or 1 with `backed_targets`, `lam`, `tc` and `stage_tiles` as
    they are; not with `restart_fraction` > 0 nor two layers (ValueError before anything is touched).  `carry_score` int64[n_games]
    and `carry_moves` int32[n_games] hold the games so far, `finished` int64[24] the whole games that ended (`finished_summary`);
    the three are allocated by the first continue launch.  `total_score`, `lengths` and stats() stay per segment.  A lambda-walk ends
    at the segment's cut.  No checkpoint holds any of it: a loaded agent's games begin at their resets.  `eval_max_steps` (an
    attribute, None by default: the agent's `max_steps`): the cap of evaluate_launch's games, so of evaluate and evaluate_search, any
    value in 1..65,535 -- the evaluation launches hold no per-move buffers.
    `rollout_deep_empty_max` (an attribute, None by default: the agent as it was; section 13.13): an int E in 0..16 and, with
    `rollout_layers` 2, `rollout` plays the round's games under the search whose depth the board chooses -- two chance layers where
    the board a move is made from has at most E empty cells, one elsewhere (rollout_adaptive_launch) -- and records them as before,
    with `backed` if `backed_targets` and from `start` once a restart or continue pick has filled it: with E set, two layers go with
    `restart_fraction` > 0 and with `continue_games`.  Any other `rollout_layers` and `stage_tiles` are refused (ValueError before
    anything is touched).  The launch adds the moves at each depth to `depth_stats` (rollout_depth_summary).  The learners, the apply
    and the pick launches read the records as they are.  It says how rounds are played, so no checkpoint holds it.
    `set_shard` (a method; no shard by default: the agent as it was; section 13.14): the agent's `n_games` games are the games game0 ..
    game0 + n_games - 1 of a job of n_games_total, played by the ranks of a torch.distributed group; `learn_batch` calls `exchange`
    between learn() and apply(), after which `acc` (and `acc_abs`) hold the sum over the ranks, and the apply launch runs replicated:
    weights, E, A and tc_stats are identical on all ranks and equal, bit for bit, those of one process on n_games_total games.  It
    goes with every other option.  stats(), finished_summary(), restart_summary()'s counters, rollout_depth_summary(), evaluate and
    evaluate_search -- its moves_deep / moves_shallow too -- are job-wide then: summed over the ranks (Shard.reduce).  It says how rounds are played, so no checkpoint holds it: save() is valid from any rank, and load() followed by
    set_shard resumes."""
    STATS, EVAL_SUMMARY = STATS, EVAL_SUMMARY
    _shard = None                                                          # set_shard's; None: one process plays the rounds
    continue_games = False                                                 # set on the agent; checked at the launch
    eval_max_steps = None                                                  # set on the agent; None: the agent's max_steps
    carry_score = carry_moves = finished = None                            # allocated by the first continue launch
    restart_fraction = 0.0                                                 # set on the agent; checked at the launch (check_restart_fraction)
    restart_min_length = 64                                                # set on the agent; checked by the pick launch
    start = restart_stats = None                                           # allocated by the first restart launch
    rollout_layers = 0                                                     # set on the agent; checked at the launch (check_rollout_layers)
    rollout_deep_empty_max = None                                          # set on the agent; checked at the launch, with rollout_layers
    backed_targets = False                                                 # set on the agent; checked at the launch, with rollout_layers
    stage_tiles = ()                                                       # __init__'s stage_tiles, or those `tuples` carry; add_stage grows it

    def __init__(self, device, n_games, tuples=DEFAULT_TUPLES, symmetric=True, gamma=1.0, epsilon=0.0, alpha=1.0, max_steps=4096, seed=0,
                 board_id0=0, lam=0.0, tc=False, *, stage_tiles=()):
        import torch
        self.stage_tiles = check_stage_tiles(tuple(stage_tiles) or stage_tiles_of(tuples))          # (refused before a device is asked for)
        self.lam, self.tc = check_lam(lam), bool(tc)
        super().__init__(device, n_games, 4, max_steps, gamma, epsilon, seed, board_id0)
        self.tuples, self.symmetric, self.alpha = with_stages(tuples, self.stage_tiles), bool(symmetric), float(alpha)
        self.n_features = len(self.tuples) * (8 if self.symmetric else 1)
        if not 0.0 < self.alpha <= self.n_features:
            raise ValueError("alpha must be in (0, F]: the apply launch takes step = alpha / F in (0, 1]")
        self.offsets, self.n_weights = tuple_offsets(self.tuples)
        self.weights_dev = torch.zeros(self.total_weights, dtype=torch.float32, device=self.device)
        self.acc = torch.zeros((self.total_weights, 2), dtype=torch.int64, device=self.device)        # {sum, cnt}; torch allocations are 16-byte aligned
        self.values = torch.zeros((self.max_steps, self.n_games), dtype=torch.float64, device=self.device)
        self.deltas = torch.zeros_like(self.values) if self.lam > 0.0 else None
        self.acc_abs = self.E = self.A = self.tc_stats = self.backed = None
        if self.tc:
            self._tc_state()

    # ------------------------------------------------------------------ weight sets by tile stage
    @property
    def n_stages(self) -> int:
        return len(self.stage_tiles) + 1

    @property
    def total_weights(self) -> int:
        """The weights of all stages: n_stages * n_weights (n_weights is one stage's, what the library's network struct holds)."""
        return self.n_stages * self.n_weights

    def _stages(self):
        """PulseTfeNtStages of the agent's stage tiles: threshold[s - 1] = log2 of the tile at which stage s begins."""
        st = _native.TfeNtStages()
        st.n_stages = self.n_stages
        for i, tile in enumerate(self.stage_tiles):
            st.threshold[i] = tile.bit_length() - 1
        return st

    def add_stage(self, tile):
        """Weight promotion: the stage that holds `tile` is split at it.  The new, upper stage's weights -- with tc its E and A too --
        start as a copy of the stage it is split from, and its accumulators are zero, so V of every board is what it was right after
        the call; from then on the boards whose largest tile has reached `tile` learn apart.  ValueError if `tile` is no stage tile,
        begins a stage already, or the agent has MAX_STAGES stages.  Reallocates `weights_dev`, `acc` and the TC state."""
        import torch
        tiles, new = split_stage_tiles(self.stage_tiles, tile, whose="agent")
        source = [s if s < new else s - 1 for s in range(len(tiles) + 1)]
        W = self.n_weights

        def grown(t, copy):
            rows = t.reshape(self.n_stages, -1)
            out = torch.stack([rows[src] if copy or s != new else torch.zeros_like(rows[src]) for s, src in enumerate(source)])
            return out.reshape((len(source) * W,) + tuple(t.shape[1:])).contiguous()
        self.weights_dev, self.acc = grown(self.weights_dev, True), grown(self.acc, False)
        if self.acc_abs is not None:
            self.acc_abs, self.E, self.A = grown(self.acc_abs, False), grown(self.E, True), grown(self.A, True)
        self.stage_tiles = tiles
        self.tuples = with_stages(self.tuples, tiles)
        return self

    def rollout_staged_launch(self, layers, backed=False):
        """pulse_tfe_nt_rollout_staged alone: rollout_from_launch's games (layers 0 or 1, `backed` with 1) with V read by stage, begun
        on the boards of `start` where usable."""
        if layers == 2:                                                     # (in the search's words; any other depth in check_from_layers')
            self._search_options(layers)
        args = self._from_args(layers, backed)
        return self._launch("pulse_tfe_nt_rollout_staged", self._rollout_struct(), C.byref(self._stages()), *args)

    def learn_staged_launch(self, lam, backed=False, tc=False):
        """pulse_tfe_nt_learn_staged alone on the games last played: learn()'s adds (lam == 0 without backed: no deltas), the walk of
        learn_lambda_launch (lam > 0) or of learn_backed_launch (backed) into `deltas` first, with tc |d| into `acc_abs` as well; every
        move's adds go to the stage of its afterstate.  Allocates what the agent lacks of `deltas` and the TC state."""
        o = self._learner(_native.TfeNtLearnBacked, lam, deltas=backed or check_lam(lam) > 0.0, acc_abs=tc, backed=backed)
        return self._launch("pulse_tfe_nt_learn_staged", o, C.byref(self._stages()))

    def _apply_staged(self):
        """pulse_tfe_nt_apply, or with tc pulse_tfe_nt_apply_tc, once per stage on that stage's slice of weights, acc, acc_abs, E and A."""
        for s in range(self.n_stages):
            self._launch(*self._apply_struct(s, self.tc))
        return self

    def _apply_struct(self, stage, tc):
        """(entry point, its struct): pulse_tfe_nt_apply, or with tc pulse_tfe_nt_apply_tc, on stage `stage`'s slices."""
        at = stage * self.n_weights
        o = _native.TfeNtApplyTc() if tc else _native.TfeNtApply()
        self._net(o.net)
        o.net.weights = self.weights_dev[at:].data_ptr()
        o.step, o.acc = self.alpha / self.n_features, self.acc[at:].data_ptr()
        if tc:
            o.acc_abs, o.e, o.a, o.tc_stats = self.acc_abs[at:].data_ptr(), self.E[at:].data_ptr(), self.A[at:].data_ptr(), self.tc_stats.data_ptr()
        return "pulse_tfe_nt_apply_tc" if tc else "pulse_tfe_nt_apply", o

    # ------------------------------------------------------------------ the launches
    def _net(self, net):
        net.n, net.n_tuples, net.symmetric = self.n, len(self.tuples), int(self.symmetric)
        for t, cells in enumerate(self.tuples):
            net.tuple_len[t] = len(cells)
            for i, c in enumerate(cells):
                net.cells[t][i] = c
        net.n_weights, net.weights = self.n_weights, self.weights_dev.data_ptr()

    def _rollout_struct(self):
        o = self._draws(_native.TfeNtRollout(), self.round_board_id0())
        self._net(o.net)
        o.n_games, o.max_steps, o.gamma, o.epsilon = self.n_games, self.max_steps, self.gamma, self.epsilon
        o.keys, o.values, o.steps, o.lengths = self.keys.data_ptr(), self.values.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr()
        o.total_score, o.episode_reward, o.stats = self.total_score.data_ptr(), self.episode_reward.data_ptr(), self.counters.data_ptr()
        return o

    def rollout(self, layers=None):
        """One launch: n_games games under the weights as they stand (round `self.round`), into keys / values / steps / lengths /
        scores.  layers (None: the agent's `rollout_layers`) = 0: pulse_tfe_nt_rollout, greedy on reward + gamma * V; 1 or 2:
        rollout_search_launch, greedy on the q of the search that deep.  ValueError for any other.  With `backed_targets` the depth
        must be 1 or 2 (ValueError otherwise, before anything is touched) and the launch is rollout_backed_launch.  With
        `restart_fraction` > 0 the depth must be 0 or 1 (ValueError otherwise, before anything is touched), and once a pick has filled
        `start` the launch is rollout_from_launch at that depth, with the backed values if `backed_targets`.  With `stage_tiles` the
        depth must be 0 or 1 and the launch is rollout_staged_launch, from `start` (zeroed here while restart_fraction is 0 and
        `continue_games` is off).  With `continue_games` the depth must be 0 or 1, restart_fraction 0 and max_steps at least 2
        (ValueError otherwise, before anything is touched), and once a continue pick has filled `start` the launch is
        rollout_from_launch at that depth, with the backed values if `backed_targets`.  With `rollout_deep_empty_max` the depth
        must be 2 and the agent without stages (ValueError otherwise, before anything is touched), and the launch is
        rollout_adaptive_launch at that threshold, with the backed values if `backed_targets` and from `start` once a pick has filled it."""
        layers, from_start, _, _ = check_options(self.rollout_layers if layers is None else layers, self.backed_targets, self.restart_fraction,
                                                 self.continue_games, self.max_steps if self.continue_games else None, bool(self.stage_tiles),
                                                 rollout_deep_empty_max=self.rollout_deep_empty_max)
        if self.rollout_deep_empty_max is not None:                         # (two layers, no stages: check_options has seen to it)
            return self.rollout_adaptive_launch(self.rollout_deep_empty_max, backed=bool(self.backed_targets),
                                                from_start=from_start and self.start is not None)
        if self.stage_tiles:                                                # one entry point: from `start`, all zero while restarts are off
            self._restart_state()
            if not from_start:
                self.start.zero_()
            return self.rollout_staged_launch(layers, backed=bool(self.backed_targets))
        if from_start and self.start is not None:                           # (a pick has run: restarted and continued rounds alike)
            return self.rollout_from_launch(layers, backed=bool(self.backed_targets))
        if self.backed_targets:
            return self.rollout_backed_launch(layers)
        if layers:
            return self.rollout_search_launch(layers)
        return self._launch("pulse_tfe_nt_rollout", self._rollout_struct())

    def _restart_state(self):
        """`start` and `restart_stats`, zeroed, where the agent has none yet."""
        import torch
        if self.start is None:
            self.start = torch.zeros(self.n_games, dtype=torch.int64, device=self.device)             # (uint64 words)
            self.restart_stats = torch.zeros(2, dtype=torch.int64, device=self.device)

    # ------------------------------------------------------------------ games continued across rounds
    def _continue_state(self):
        """`carry_score`, `carry_moves` and `finished`, zeroed, where the agent has none yet; `start` too (_restart_state)."""
        import torch
        self._restart_state()
        if self.carry_score is None:
            self.carry_score = torch.zeros(self.n_games, dtype=torch.int64, device=self.device)
            self.carry_moves = torch.zeros(self.n_games, dtype=torch.int32, device=self.device)
            self.finished = torch.zeros(len(FINISHED_SUMMARY) + EVAL_BINS, dtype=torch.int64, device=self.device)

    def continue_pick_launch(self):
        """pulse_tfe_nt_continue_pick alone on the games last recorded (under this round's seed and boards), whatever the agent's
        `continue_games`: per game cut at `max_steps`, `start` becomes the board its last move was made on and the carries take the
        segment without that move; every other game is added whole to `finished`, and its `start` and carries become 0.  ValueError
        if max_steps < 2."""
        check_options(continue_games=True, max_steps=self.max_steps)
        self._continue_state()
        o = _native.TfeNtContinuePick()
        o.n_games, o.max_steps, o.env_seed, o.board_id0 = self.n_games, self.max_steps, self.env_seed, self.round_board_id0()
        o.keys, o.steps, o.lengths, o.total_score = self.keys.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr(), self.total_score.data_ptr()
        o.start, o.carry_score, o.carry_moves, o.finished = self.start.data_ptr(), self.carry_score.data_ptr(), self.carry_moves.data_ptr(), self.finished.data_ptr()
        return self._launch("pulse_tfe_nt_continue_pick", o)

    def finished_summary(self, clear=True) -> dict:
        """finished_summary_on_host of `finished` (synchronises): the whole games that ended since the words were last zeroed, the
        games continued by the pick launches since and the finished games that had been continued.  clear: `finished` is zeroed.
        With a shard the words are reduced over the ranks (sums, word 4 a maximum): the job's games."""
        if self.finished is None:
            raise ValueError("no continue launch has run: the agent holds no finished")
        words = self.finished.cpu().tolist()
        out = finished_summary_on_host(words if self._shard is None else self._shard.reduce(words, max_at=(4,)))        # (with a shard: job-wide)
        if clear:
            self.finished.zero_()
        return out

    def _per_move(self, name):
        """The agent's `deltas` or `backed` (`name`): float64 in the shape of `values`, allocated zeroed where the agent has none yet."""
        import torch
        if getattr(self, name) is None:
            setattr(self, name, torch.zeros_like(self.values))
        return getattr(self, name)

    def _from_args(self, layers, backed):
        """What rollout_from_launch and rollout_staged_launch pass beside the struct: (layers (check_from_layers), `backed` or None,
        `start`), `start` and `backed` allocated where the agent has none."""
        layers = check_from_layers(layers, backed)
        self._restart_state()
        return layers, self._per_move("backed").data_ptr() if backed else None, self.start.data_ptr()

    def rollout_from_launch(self, layers, backed=False):
        """pulse_tfe_nt_rollout_from alone, whatever the agent's attributes: rollout()'s games at `layers` = 0 (one ply) or 1 (one-layer
        search; ValueError for any other), each begun on the board in `start` where that board is usable and at its reset otherwise
        (`start` is 0 there afterwards).  backed: rollout_backed_launch's `backed` too (layers must be 1).  A `start` no pick has
        filled is all zero: the launch plays its sibling's games."""
        args = self._from_args(layers, backed)
        return self._launch("pulse_tfe_nt_rollout_from", self._rollout_struct(), *args)

    def restart_pick_launch(self, fraction=None, min_length=None):
        """pulse_tfe_nt_restart_pick alone on the games last recorded (under this round's seed and boards): `start` becomes, per game
        of at least `min_length` moves, the board it stood on before move floor(L * fraction), and 0 for the others; `restart_stats`
        has the boards picked and their depths added.  fraction, min_length: None for the agent's attributes."""
        fraction = check_restart_fraction(self.restart_fraction if fraction is None else fraction)
        if not fraction > 0.0:
            raise ValueError("the pick needs a fraction in (0, 1): restart_fraction is 0 (off)")
        self._restart_state()
        o = _native.TfeNtRestartPick()
        o.n_games, o.max_steps, o.env_seed, o.board_id0 = self.n_games, self.max_steps, self.env_seed, self.round_board_id0()
        o.fraction, o.min_length = fraction, int(self.restart_min_length if min_length is None else min_length)
        o.keys, o.lengths, o.start, o.picked = self.keys.data_ptr(), self.lengths.data_ptr(), self.start.data_ptr(), self.restart_stats.data_ptr()
        return self._launch("pulse_tfe_nt_restart_pick", o)

    def restart_summary(self) -> dict:
        """{"picked", "mean_depth", "started"} (restart_summary_on_host; synchronises): the boards the pick launches since the last call
        picked and the mean of their t*, and the non-zero entries of `start` as it stands -- after a pick the games that will be
        restarted, after a roll-out those that were.  `restart_stats` is zeroed."""
        if self.start is None:
            raise ValueError("no restart launch has run: the agent holds no start")
        out = restart_summary_on_host(self.restart_stats.cpu().tolist(), self.start.cpu().numpy())
        if self._shard is not None:                                         # job-wide: the three counters summed over the ranks
            picked, total, started = self._shard.reduce([out["picked"], self.restart_stats[1].item(), out["started"]])
            out = dict(picked=picked, mean_depth=total / picked if picked else 0.0, started=started)
        self.restart_stats.zero_()
        return out

    def rollout_search_launch(self, layers):
        """pulse_tfe_nt_rollout_search alone, whatever the agent's `rollout_layers`: the roll-out's games, draws and records with the
        greedy action taken on the q of expectimax search `layers` chance layers deep (1 or 2; ValueError for any other).  `values`
        holds the network's V of the chosen afterstates, so the learners read the records as they read rollout()'s."""
        layers = check_layers(layers)
        return self._launch("pulse_tfe_nt_rollout_search", self._rollout_struct(), layers)

    def rollout_adaptive_launch(self, deep_empty_max, backed=False, from_start=False):
        """pulse_tfe_nt_rollout_adaptive alone, whatever the agent's attributes: rollout_search_launch's games and records at two
        layers on the boards with at most `deep_empty_max` (0..16; ValueError otherwise) empty cells and at one layer on the others.
        backed: rollout_backed_launch's `backed` too, of the q at the depth the board chose.  from_start: the games begin on the
        boards of `start` where usable, as rollout_from_launch's do.  The moves at each depth are ADDED to `depth_stats`.  Allocates
        `backed`, `start` and `depth_stats` where the agent has none, and zeroes nothing."""
        deep_empty_max = check_deep_empty_max(deep_empty_max)
        if deep_empty_max is None:
            raise ValueError("deep_empty_max must be None or an int in 0..16")
        if from_start:
            self._restart_state()
        return self._launch("pulse_tfe_nt_rollout_adaptive", self._rollout_struct(), deep_empty_max,
                            self._per_move("backed").data_ptr() if backed else None, self.start.data_ptr() if from_start else None,
                            self._depth_words().data_ptr())

    def rollout_depth_summary(self, clear=True) -> dict:
        """{"moves_deep", "moves_shallow"} (synchronises): the moves the adaptive launches since the words were last zeroed searched
        two layers and one layer deep -- rollout_adaptive_launch's and the adaptive evaluations' alike.  clear: `depth_stats` is zeroed.
        With a shard the two words are summed over the ranks: the job's moves.  ValueError if no adaptive launch has run."""
        if self.depth_stats is None:
            raise ValueError("no adaptive launch has run: the agent holds no depth_stats")
        deep, shallow = self._depth_read()
        if clear:
            self.depth_stats.zero_()
        return dict(moves_deep=deep, moves_shallow=shallow)

    def _depth_read(self) -> list:
        """`depth_stats` on the host (synchronises); with a shard summed over the ranks, as stats() is (job-wide)."""
        words = self.depth_stats.cpu().tolist()
        return words if self._shard is None else self._shard.reduce(words)

    def rollout_backed_launch(self, layers):
        """pulse_tfe_nt_rollout_backed alone, whatever the agent's `rollout_layers` and `backed_targets`: rollout_search_launch's games
        and records, and in `backed` (allocated here if the agent has none) per move the largest q of the search over the moves that
        change the board."""
        layers = check_layers(layers)
        return self._launch("pulse_tfe_nt_rollout_backed", self._rollout_struct(), layers, self._per_move("backed").data_ptr())

    def _moves(self, o):
        """The network and the fields the two learners' structs share."""
        self._net(o.net)
        o.n_games, o.max_steps, o.gamma = self.n_games, self.max_steps, self.gamma
        o.keys, o.values, o.steps, o.lengths = self.keys.data_ptr(), self.values.data_ptr(), self.steps.data_ptr(), self.lengths.data_ptr()
        o.acc, o.stats = self.acc.data_ptr(), self.counters.data_ptr()
        return o

    def _tc_state(self):
        """The third accumulator, E, A and tc_stats, zeroed, where the agent has none yet."""
        import torch
        if self.acc_abs is None:
            self.acc_abs = torch.zeros(self.total_weights, dtype=torch.int64, device=self.device)
            self.E = torch.zeros(self.total_weights, dtype=torch.float64, device=self.device)
            self.A = torch.zeros(self.total_weights, dtype=torch.float64, device=self.device)
            self.tc_stats = torch.zeros(4, dtype=torch.int64, device=self.device)

    def _learner(self, struct, lam, deltas=False, acc_abs=False, backed=False):
        """A learner's struct (`struct`, its class) filled: the moves, `lam` (check_lam) and, of `deltas`, `acc_abs` and `backed`, those
        asked for.  `deltas` and the TC state are allocated where the agent has none; `backed` is a roll-out's to make (ValueError)."""
        lam = check_lam(lam)
        if backed and self.backed is None:
            raise ValueError("no roll-out with backed values has run: the agent holds no backed")
        o = self._moves(struct())
        o.lam = lam
        if deltas:
            o.deltas = self._per_move("deltas").data_ptr()
        if backed:
            o.backed = self.backed.data_ptr()
        if acc_abs:
            self._tc_state()
            o.acc_abs = self.acc_abs.data_ptr()
        return o

    def learn(self):
        """The temporal differences of the games last played, into the accumulators: one launch, or with lam > 0
        learn_lambda_launch's two; with tc, learn_tc_launch's; with backed_targets, learn_backed_launch's; with stage_tiles,
        learn_staged_launch's under the same three."""
        if self.stage_tiles:
            return self.learn_staged_launch(self.lam, backed=bool(self.backed_targets), tc=self.tc)
        if self.backed_targets:
            return self.learn_backed_launch(self.lam)
        if self.tc:
            return self.learn_tc_launch(self.lam)
        if self.lam > 0.0:
            return self.learn_lambda_launch(self.lam)
        return self._launch("pulse_tfe_nt_learn", self._moves(_native.TfeNtLearn()))

    def learn_lambda_launch(self, lam):
        """pulse_tfe_nt_learn_lambda on the games last played, whatever the agent's own `lam`: the backward walk into `deltas`
        (allocated here if the agent has none) and the adds of the lambda-differences into the accumulators."""
        o = self._learner(_native.TfeNtLearnLambda, lam, deltas=True)
        return self._launch("pulse_tfe_nt_learn_lambda", o)

    def learn_tc_launch(self, lam):
        """pulse_tfe_nt_learn_tc on the games last played, whatever the agent's own `lam` and `tc`: the adds of learn() (lam == 0: one
        launch, no deltas) or of learn_lambda_launch (lam > 0: the walk into `deltas`, then the adds), with |d| into `acc_abs` as
        well.  Allocates the TC state, and for lam > 0 `deltas`, if the agent has none."""
        o = self._learner(_native.TfeNtLearnTc, lam, deltas=check_lam(lam) > 0.0, acc_abs=True)
        return self._launch("pulse_tfe_nt_learn_tc", o)

    def learn_backed_launch(self, lam):
        """pulse_tfe_nt_learn_backed on the games rollout_backed_launch last recorded, whatever the agent's own `lam` and
        `backed_targets`: the backward walk of backed[t + 1] - V_t into `deltas` (allocated here if the agent has none) and the adds
        of what it left -- with the agent's `tc` into `acc_abs` as well.  ValueError if no such roll-out has run."""
        o = self._learner(_native.TfeNtLearnBacked, lam, deltas=True, acc_abs=self.tc, backed=True)
        return self._launch("pulse_tfe_nt_learn_backed", o)

    def apply_tc_launch(self):
        """pulse_tfe_nt_apply_tc: every visited weight moves by (alpha / F) * rho of the mean of its adds, rho = |E| / A as they stood;
        E and A take the round's means, the three accumulator words are zero afterwards and tc_stats has the round added."""
        self._tc_state()
        return self._launch(*self._apply_struct(0, True))

    def apply(self):
        """One launch: every visited weight moves by alpha / F of the mean of its adds; the accumulators are zero afterwards.  With
        tc, apply_tc_launch.  With stage_tiles, either once per stage on that stage's slices."""
        if self.stage_tiles:
            return self._apply_staged()
        if self.tc:
            return self.apply_tc_launch()
        return self._launch(*self._apply_struct(0, False))

    def learn_batch(self):
        self.rollout()
        self.learn()
        if self._shard is not None:                                         # the ranks' accumulators summed: apply runs replicated
            self.exchange()
        self.apply()
        if self.continue_games:                                             # the cut games' boards for the next round, the ended games into `finished`
            self.continue_pick_launch()
        elif self.restart_fraction > 0.0:                                  # the next round's start boards, from this round's records
            self.restart_pick_launch()
        self.round += 1
        return self

    # ------------------------------------------------------------------ rank-parallel rounds (tfe_ntuple_ranks.py)
    def set_shard(self, n_games_total, game0, group=None, exchange_capacity=None):
        """The agent's games become the games game0 .. game0 + n_games - 1 of a job of `n_games_total` (its own `n_games` is its local
        count; tfe_ntuple_ranks.shard_of gives the split of sharding.shard_tables, so uneven splits work).  group: the
        torch.distributed group of the job's ranks (None: the default group, or without torch.distributed a world of one).
        exchange_capacity: the entries the rank's list has room for (None: min(total_weights, n_games * max_steps * F), which a round
        cannot overflow; a round that finds more on any rank is exchanged by a dense all-reduce, as exactly).  ValueError if the
        games do not lie inside the job's."""
        from .tfe_ntuple_ranks import Shard
        self._shard = Shard(self, n_games_total, game0, group, exchange_capacity)
        return self

    def round_board_id0(self, round=None) -> int:
        if self._shard is None:
            return super().round_board_id0(round)
        return self._shard.round_board_id0(self.board_id0, self.round if round is None else round)

    def exchange(self) -> dict:
        """Between learn() and apply(): `acc` (and `acc_abs`) become the sum over the ranks (tfe_ntuple_ranks.exchange_round): the
        pack launch, an all-gather of the 4-word headers READ ON THE HOST -- the one host read per round this mode costs -- and then
        the lists all-gathered and every other rank's added by the unpack launch, or, where a rank found more than its list holds, a
        dense all-reduce.  Returns the round's record (exchange_summary)."""
        if self._shard is None:
            raise ValueError("no shard is set: the agent holds no exchange (set_shard)")
        return self._shard.exchange(self.round)

    def exchange_summary(self, clear=True) -> dict:
        """{"rounds", "added", "refused"} (synchronises): per exchange since the last clear {"round", "path" ("sparse" or "dense"),
        "entries" (found, per rank), "bytes" (what this rank's collectives gathered or reduced)}, and the entries the unpack launches
        added and refused."""
        if self._shard is None:
            raise ValueError("no shard is set: the agent holds no exchange (set_shard)")
        return self._shard.summary(clear)

    def stats(self) -> dict:
        """The counters by name; with a shard summed over the ranks (job-wide)."""
        if self._shard is None:
            return super().stats()
        return dict(zip(self.STATS, self._shard.reduce(self.counters.cpu().tolist())))

    def _evaluate_with(self, launch, n_games, epsilon, board_id0, per_game) -> dict:
        """With a shard `n_games` (default: the job's) is the job-wide count: the rank plays its share of the boards board_id0 + g
        (sharding.shard_tables) and the counters are reduced over the ranks -- sums, word 4 (max_score) a maximum -- so mean and
        standard error are the single process's.  per_game: the arrays are those of the rank's OWN share."""
        if self._shard is None:
            return super()._evaluate_with(launch, n_games, epsilon, board_id0, per_game)
        total = self._shard.n_games_total if n_games is None else int(n_games)
        n, first = self._shard.eval_shard(total, self.eval_board_id0() if board_id0 is None else int(board_id0))
        self.eval_counters(clear=True)
        arrays = self._evaluate_launch_with(launch, n, epsilon, first, per_game) if n else None
        out = eval_summary_on_host(self._shard.reduce(self._eval.cpu().tolist(), max_at=(4,)))
        if per_game:
            out["total_score"] = arrays[0].cpu().numpy() if n else np.zeros(0, dtype=np.int64)
            out["lengths"] = arrays[1].cpu().numpy() if n else np.zeros(0, dtype=np.int32)
        return out

    # ------------------------------------------------------------------ evaluation
    def _eval_struct(self):
        o = _native.TfeNtEval()
        self._net(o.net)
        o.gamma = self.gamma
        return o

    def _entry(self, name, *args):
        """An evaluation's launch, as evaluate_launch's body takes it: entry point `name` on the filled struct, `args` beside it."""
        return lambda o: self._launch(name, o, *args)

    def _eval_launch(self, o):
        """The evaluation one ply deep."""
        return self._search_eval_launch(0, None)(o)

    # ------------------------------------------------------------------ expectimax search (DESIGN.md sections 13.1, 13.4 and 13.11)
    depth_stats = None                                                     # int64[2] on the device, from the first adaptive launch: moves two layers deep, one layer deep

    def _search_options(self, layers, deep_empty_max=None):
        """(layers, deep_empty_max) as ints (deep_empty_max: or None), or check_options' ValueError of what the search refuses: a depth
        other than 1 or 2, a threshold other than None or 0..16, a threshold without two layers, two layers on an agent with stage_tiles"""
        return check_options(staged=bool(self.stage_tiles), search=True, layers=layers, deep_empty_max=deep_empty_max)[2:]

    def _depth_words(self):
        import torch
        if self.depth_stats is None:
            self.depth_stats = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self.depth_stats

    def _search_eval_launch(self, layers, deep_empty_max):
        """The launch of an evaluation `layers` chance layers deep (0: one ply; _search_options' values): on stages the one staged entry
        point with the depth beside the struct; else pulse_tfe_nt_evaluate, at one layer pulse_tfe_nt_evaluate_search, at two
        pulse_tfe_nt_evaluate_search_deep with the depth; with deep_empty_max (and two layers) pulse_tfe_nt_evaluate_search_adaptive
        with the threshold and the agent's `depth_stats`."""
        if self.stage_tiles:
            return self._entry("pulse_tfe_nt_evaluate_staged", C.byref(self._stages()), layers)
        if layers < 2:
            return self._entry("pulse_tfe_nt_evaluate_search" if layers else "pulse_tfe_nt_evaluate")
        if deep_empty_max is None:
            return self._entry("pulse_tfe_nt_evaluate_search_deep", layers)
        return self._entry("pulse_tfe_nt_evaluate_search_adaptive", deep_empty_max, self._depth_words().data_ptr())

    def _search_struct(self, boards, q, action, candidates):
        o = _native.TfeNtSearch()
        self._net(o.net)
        o.n_boards, o.gamma, o.tie_seed, o.round = boards.numel(), self.gamma, self.tie_seed, self.round
        o.boards, o.q, o.action, o.candidates = boards.data_ptr(), q.data_ptr(), action.data_ptr(), candidates.data_ptr()
        return o

    def search_launch(self, boards, q, action, candidates, layers=1, deep_empty_max=None):
        """The launch of search() alone on device tensors: boards int64[N] (the keys' words), q float64[N, 4], action int8[N],
        candidates uint8[N].  layers = 1: pulse_tfe_nt_search; layers = 2: pulse_tfe_nt_search_deep (ValueError for any other); with
        layers = 2 and deep_empty_max = 0..16: pulse_tfe_nt_search_adaptive, two layers on the boards with at most that many empty
        cells and one layer on the others."""
        layers, deep_empty_max = self._search_options(layers, deep_empty_max)
        o = self._search_struct(boards, q, action, candidates)
        if self.stage_tiles:
            return self._launch("pulse_tfe_nt_search_staged", o, C.byref(self._stages()))
        if layers == 1:
            return self._launch("pulse_tfe_nt_search", o)
        if deep_empty_max is not None:
            return self._launch("pulse_tfe_nt_search_adaptive", o, deep_empty_max)
        return self._launch("pulse_tfe_nt_search_deep", o, layers)

    def search(self, keys, layers=1, deep_empty_max=None) -> dict:
        """One launch and one read-back: q float64[N, 4] of the packed boards `keys` under `layers` chance layers of search (1 or 2), the
        greedy action int8[N] (-1: the board is over) and the candidates uint8[N] (bit a: move a changes the board); search_nt_on_host
        on the device, with deep_empty_max search_adaptive_nt_on_host."""
        import torch
        layers, deep_empty_max = self._search_options(layers, deep_empty_max)
        keys = np.array(keys, dtype=np.uint64).reshape(-1)                       # (a copy: torch takes no read-only array)
        boards = torch.from_numpy(keys.view(np.int64)).to(self.device)
        q = torch.zeros((len(keys), 4), dtype=torch.float64, device=self.device)
        action, candidates = torch.zeros(len(keys), dtype=torch.int8, device=self.device), torch.zeros(len(keys), dtype=torch.uint8, device=self.device)
        self.search_launch(boards, q, action, candidates, layers, deep_empty_max)
        return dict(q=q.cpu().numpy(), action=action.cpu().numpy(), candidates=candidates.cpu().numpy())

    def evaluate_search_launch(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False, layers=1, deep_empty_max=None):
        """evaluate_launch() under the search policy of `layers` chance layers (1 or 2); with layers = 2 and deep_empty_max = 0..16 under
        the adaptive search, which also ADDS the moves at each depth to `depth_stats` (int64[2]: two layers, one layer)."""
        launch = self._search_eval_launch(*self._search_options(layers, deep_empty_max))
        return self._evaluate_launch_with(launch, n_games, epsilon, board_id0, per_game)

    def evaluate_search(self, n_games=None, epsilon=0.0, board_id0=None, per_game=False, layers=1, deep_empty_max=None) -> dict:
        """evaluate() under the search policy of `layers` chance layers (1 or 2): the same default boards, so the policies are paired on
        the spawns each game starts from.  With layers = 2 and deep_empty_max = 0..16 the search is two layers deep on the boards with at
        most that many empty cells and one layer deep on the others (section 13.11), and the dict also has moves_deep / moves_shallow."""
        layers, deep_empty_max = self._search_options(layers, deep_empty_max)
        if deep_empty_max is not None:
            self._depth_words().zero_()
        out = self._evaluate_with(self._search_eval_launch(layers, deep_empty_max), n_games, epsilon, board_id0, per_game)
        if deep_empty_max is not None:
            out["moves_deep"], out["moves_shallow"] = self._depth_read()   # (with a shard: job-wide, as the summary is)
        return out

    # ------------------------------------------------------------------ read-back (the only syncs) and the checkpoint
    def weights(self) -> np.ndarray:
        """float32[n_weights] on the host; with stage_tiles float32[n_stages * n_weights], stage s at [s * n_weights, (s + 1) * n_weights)."""
        return self.weights_dev.cpu().numpy()

    def trajectory(self):
        """(keys uint64[T, B], values float64[T, B], steps uint8[T, B], lengths int32[B]) of the last batch, T = the longest game; rows
        at and beyond a game's length hold whatever the buffers held before."""
        T, lengths = self._played()
        return self.keys[:T].cpu().numpy().view(np.uint64), self.values[:T].cpu().numpy(), self.steps[:T].cpu().numpy(), lengths

    def trajectory_deltas(self) -> np.ndarray:
        """float64[T, B]: the lambda-differences of the last TD(lambda) learn launch, T = the longest game; rows at and beyond a game's
        length hold whatever `deltas` held before."""
        if self.deltas is None:
            raise ValueError("no TD(lambda) launch has run: the agent holds no deltas")
        T, _ = self._played()
        return self.deltas[:T].cpu().numpy()

    def trajectory_backed(self) -> np.ndarray:
        """float64[T, B]: the search's backed-up values of the last rollout_backed_launch, T = the longest game; rows at and beyond a
        game's length hold whatever `backed` held before."""
        if self.backed is None:
            raise ValueError("no roll-out with backed values has run: the agent holds no backed")
        T, _ = self._played()
        return self.backed[:T].cpu().numpy()

    def coherence(self):
        """(E, A), float64[n_weights] each, on the host."""
        if self.E is None:
            raise ValueError("no temporal-coherence launch has run: the agent holds no E and A")
        return self.E.cpu().numpy(), self.A.cpu().numpy()

    def tc_summary(self) -> dict:
        """{"moved", "mean_rho"} of the apply_tc launches since the last call (tc_summary_on_host; synchronises), and tc_stats zeroed."""
        if self.tc_stats is None:
            raise ValueError("no temporal-coherence launch has run: the agent holds no tc_stats")
        out = tc_summary_on_host(self.tc_stats.cpu().tolist())
        self.tc_stats.zero_()
        return out

    def save(self, path):
        """The non-zero weights and what a continued run needs as an .npz (write_checkpoint); with tc, E and A too.  `rollout_layers`,
        `backed_targets`, `restart_fraction`, `restart_min_length`, `continue_games`, `eval_max_steps` and `rollout_deep_empty_max` are not saved: they say how
        rounds are played, learnt and evaluated, not what the network is; nor are `start` and the carries of continued games."""
        write_checkpoint(path, self.weights(), self.tuples, symmetric=int(self.symmetric), gamma=self.gamma, epsilon=self.epsilon, alpha=self.alpha,
                         max_steps=self.max_steps, seed=self.seed, board_id0=self.board_id0, round=self.round, n_games=self.n_games, lam=self.lam,
                         tc=self.coherence() if self.tc else None, stage_tiles=self.stage_tiles)

    @classmethod
    def load(cls, path, device, n_games=None):
        """The agent save() wrote: weights, round, seeds, lam, tc and with it E and A restored.  With the saved n_games it continues the run the saved agent would
        have continued (another n_games plays other boards: round r starts at board_id0 + r * n_games).  `rollout_layers` is 0, whatever the saved
        agent played under, `backed_targets` False, `restart_fraction` 0.0 and `continue_games` False with no `start` and no carries:
        set them again to continue such rounds; a loaded agent's games begin at their resets."""
        import torch
        f = read_checkpoint(path)
        agent = cls(device, f["n_games"] if n_games is None else n_games, tuples=f["tuples"], symmetric=f["symmetric"], gamma=f["gamma"],
                    epsilon=f["epsilon"], alpha=f["alpha"], max_steps=f["max_steps"], seed=f["seed"], board_id0=f["board_id0"], lam=f["lam"], tc=f["tc"],
                    stage_tiles=f["stage_tiles"])
        agent.weights_dev.copy_(torch.from_numpy(weights_of_checkpoint(f)))
        if f["tc"]:
            E, A = coherence_of_checkpoint(f)
            agent.E.copy_(torch.from_numpy(E))
            agent.A.copy_(torch.from_numpy(A))
        agent.round = f["round"]
        return agent

    def clear(self):
        """The empty network, zeroed accumulators and counters, round 0."""
        self.weights_dev.zero_()
        self.acc.zero_()
        self.counters.zero_()
        for t in (self.acc_abs, self.E, self.A, self.tc_stats, self.start, self.restart_stats, self.carry_score, self.carry_moves, self.finished):
            if t is not None:
                t.zero_()
        self.round = 0
        return self
