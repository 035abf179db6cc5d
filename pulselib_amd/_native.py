"""ctypes binding of libpulse_hip.so (include/pulse_env.h).

The library is the product: if it is missing or does not load, importing this module's `lib()`
raises -- there is no PyTorch/CPU fallback for any environment step.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_SO = Path(os.environ["PULSE_LIB"]) if os.environ.get("PULSE_LIB") else _PKG / "libpulse_hip.so"     # PULSE_LIB: A/B of builds (tools/ab_bench.py)
_CSRC = _PKG / "csrc"
_LIB: C.CDLL | None = None

HANDRANKS_LEN = 32487834
STATS_SLOTS, STATS_STRIDE = 256, 16          # PulsePokerResetOpts.stats_out layout (include/pulse_env.h)
MAX_SEATS = 16

# phase bits (include/pulse_env.h)
PH_CAPTURE, PH_EQUITY, PH_EXECUTE, PH_ADVANCE = 0x001, 0x002, 0x004, 0x008
PH_FOLDWIN, PH_SHOWDOWN, PH_CLEARDONE, PH_REWARD, PH_OBS = 0x010, 0x020, 0x040, 0x080, 0x100
PH_STEP = 0x1FF

# PulsePokerView.flags: kernel variants selectable per view (include/pulse_env.h)
VIEW_NO_OBS_STAGING, VIEW_NO_CHUNK, VIEW_FOUR_LANES, VIEW_NO_PAIRS, VIEW_NO_LONG_LAUNCHES = 0x1, 0x2, 0x4, 0x8, 0x10

AGENT_EXTERNAL, AGENT_RANDOM, AGENT_HEURISTIC_HANDS, AGENT_TIGHT_AGGRESSIVE, AGENT_LOOSE_PASSIVE, AGENT_SMALL_BALL = range(6)


class PulseError(RuntimeError):
    pass


class PokerView(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("n_games", "n_players", "active_players", "max_players", "obs_size", "hand_ranks_len",
                                  "flags", "reserved0")]
        + [(n, C.c_void_p) for n in (
            "hand_ranks",
            "pots", "stages", "deck_positions", "button", "sb", "bb", "idx", "highest", "agg", "acted",
            "last_raise_size", "prev_stacks", "prev_invested",
            "is_done", "is_done_out", "equity_dirty",
            "stacks", "current_round_bet", "total_invested", "status",
            "hands", "board", "decks", "equities", "obs",
            "w1", "w2", "K", "alpha",
            "pre_board", "pre_hands", "pre_eq", "pre_rank")]
    )


class PokerResetOpts(C.Structure):
    _fields_ = [("first", C.c_int32), ("starting_bbs", C.c_int32), ("max_bbs", C.c_int32), ("rotation", C.c_int32),
                ("seed", C.c_uint64), ("episode", C.c_uint64), ("table_id0", C.c_uint64),
                ("prefixed_decks", C.c_void_p), ("decks_out", C.c_void_p),
                ("shuffle_key_bits", C.c_int32), ("reserved0", C.c_int32), ("stats_rewards", C.c_void_p), ("stats_out", C.c_void_p)]


class QNet(C.Structure):
    _fields_ = [("state_dim", C.c_int32), ("n_actions", C.c_int32)] + [(n, C.c_void_p) for n in (
        "w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4", "w5", "b5")]


class QNetTrain(C.Structure):
    _fields_ = [("net", QNet), ("target", QNet)] + [(n, C.c_void_p) for n in (
        "params", "target_params", "grad", "exp_avg", "exp_avg_sq", "step", "stats", "report", "partials")] + [(n, C.c_float) for n in (
            "lr", "weight_decay", "beta1", "beta2", "eps", "max_grad_norm", "gamma", "dropout_p")] + [
        ("update_freq", C.c_int32), ("max_blocks", C.c_int32), ("select_scratch", C.c_void_p), ("select_words", C.c_int64), ("select_from_act", C.c_int32),
        ("separate_apply", C.c_int32), ("meet_wait_ticks", C.c_int64), ("debug_meet_extra", C.c_int32), ("reserved0", C.c_int32),
        ("stability", C.c_void_p)]


class QNetAct(C.Structure):
    _fields_ = [("states", C.c_void_p), ("row_stride", C.c_int64), ("seat_idx", C.c_void_p), ("q_seat", C.c_int32), ("epsilon", C.c_float),
                ("seed", C.c_uint64), ("step", C.c_uint64), ("table_id0", C.c_uint64), ("terminated", C.c_void_p), ("row_mask_out", C.c_void_p),
                ("select_scratch", C.c_void_p), ("select_words", C.c_int64)]


class QTable(C.Structure):
    _fields_ = [("entries", C.c_void_p), ("capacity", C.c_uint64), ("region_slots", C.c_uint64)]


class QTableScratch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("count", "cells", "targets", "owner", "acc_key", "acc_cnt", "acc_sum")] + [
        ("n", C.c_uint32), ("acc_slots", C.c_uint32), ("wait_ticks", C.c_int64), ("debug_meet_extra", C.c_int32), ("reserved0", C.c_int32)]


class BlackjackView(C.Structure):
    _fields_ = [("batch_size", C.c_int32)] + [(n, C.c_void_p) for n in (
        "decks", "deck_positions", "players_cards", "players_card_idx", "player_card_sums",
        "dealer_cards", "dealer_card_idx", "dealer_upcard", "dealer_card_sums",
        "terminated", "has_ace", "dealer_has_ace", "rewards", "obs")]


# pulse_blackjack_mc_rollout's accumulator layout (include/pulse_env.h)
BJ_MC_MAX_ACTIONS, BJ_MC_STATES = 16, 1024
BJ_MC_ACC_LEN = BJ_MC_STATES * BJ_MC_MAX_ACTIONS * 2


class BlackjackMC(C.Structure):
    _fields_ = [("n_games", C.c_int32), ("n_episodes", C.c_int32), ("seed", C.c_uint64), ("episode", C.c_uint64),
                ("hit_prob", C.c_void_p), ("decks_src", C.c_void_p), ("acc", C.c_void_p), ("stats", C.c_void_p), ("trace", C.c_void_p),
                ("max_blocks", C.c_int32), ("reserved0", C.c_int32)]


# pulse_blackjack_mc_control_rollout's accumulator layout: per state the hits' (k, sign) cells, then the stand's two
BJ_MCC_CELLS = BJ_MC_MAX_ACTIONS * 2 + 2
BJ_MCC_ACC_LEN = BJ_MC_STATES * BJ_MCC_CELLS
BJ_MCC_TIE_KEY = 0x7C01F11B5EED


class BlackjackMCControl(C.Structure):
    _fields_ = BlackjackMC._fields_


class BlackjackMCImprove(C.Structure):
    _fields_ = [("acc", C.c_void_p), ("gamma", C.c_double), ("epsilon", C.c_double), ("seed", C.c_uint64), ("round", C.c_uint64),
                ("q", C.c_void_p), ("hit_prob", C.c_void_p), ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


# the 2048 Monte-Carlo table (include/pulse_env.h): 128-byte entries {uint64 key, int64 cnt[4], int64 sum[4], 56 spare bytes}
TFE_MC_ENTRY_BYTES, TFE_MC_MAX_PROBE, TFE_MC_R_MAX = 128, 512, 17
_TFE_MC_HEAD = [("entries", C.c_void_p), ("capacity", C.c_uint64), ("n_games", C.c_int32), ("n", C.c_int32), ("max_steps", C.c_int32),
                ("frac_bits", C.c_int32), ("gamma", C.c_double), ("epsilon", C.c_double)]


class TfeMCRollout(C.Structure):
    _fields_ = _TFE_MC_HEAD + [(n, C.c_uint64) for n in ("env_seed", "agent_seed", "tie_seed", "board_id0", "round")] + [
        (n, C.c_void_p) for n in ("keys", "steps", "lengths", "total_score", "episode_reward", "stats")] + [("reserved0", C.c_int64)]


class TfeMCLearn(C.Structure):
    _fields_ = _TFE_MC_HEAD + [(n, C.c_void_p) for n in ("keys", "steps", "lengths", "stats")] + [("reserved0", C.c_int64)]


class TfeMCEval(C.Structure):
    _fields_ = [("entries", C.c_void_p), ("capacity", C.c_uint64), ("n_games", C.c_int32), ("n", C.c_int32), ("max_steps", C.c_int32),
                ("frac_bits", C.c_int32), ("epsilon", C.c_double)] + [
        (n, C.c_uint64) for n in ("env_seed", "agent_seed", "tie_seed", "board_id0", "round")] + [("canonical", C.c_int32), ("reserved0", C.c_int32)] + [
        (n, C.c_void_p) for n in ("summary", "max_tile_hist", "total_score", "lengths")] + [("reserved1", C.c_int64)]


class TfeMCMerge(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_entries", C.c_uint64), ("dst", C.c_void_p), ("dst_capacity", C.c_uint64),
                ("n", C.c_int32), ("canonical", C.c_int32), ("stats", C.c_void_p), ("reserved0", C.c_int64)]


# the 2048 n-tuple network (include/pulse_env.h): the network heads the structs
TFE_NT_MAX_TUPLES, TFE_NT_MAX_LEN, TFE_NT_FRAC_BITS, TFE_NT_DELTA_MAX = 8, 6, 16, 8192.0
TFE_NT_MAX_STAGES = 4
_TFE_NT_SEEDS = [(n, C.c_uint64) for n in ("env_seed", "agent_seed", "tie_seed", "board_id0", "round")]


class TfeNtNet(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n", "n_tuples", "symmetric", "reserved0")] + [
        ("tuple_len", C.c_uint8 * TFE_NT_MAX_TUPLES), ("cells", (C.c_uint8 * 8) * TFE_NT_MAX_TUPLES), ("n_weights", C.c_uint64), ("weights", C.c_void_p)]


class TfeNtRollout(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_games", C.c_int32), ("max_steps", C.c_int32), ("gamma", C.c_double), ("epsilon", C.c_double)] + _TFE_NT_SEEDS + [
        (n, C.c_void_p) for n in ("keys", "values", "steps", "lengths", "total_score", "episode_reward", "stats")] + [("reserved0", C.c_int64)]


class TfeNtLearn(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_games", C.c_int32), ("max_steps", C.c_int32), ("gamma", C.c_double)] + [
        (n, C.c_void_p) for n in ("keys", "values", "steps", "lengths", "acc", "stats")] + [("reserved0", C.c_int64)]


class TfeNtLearnLambda(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_games", C.c_int32), ("max_steps", C.c_int32), ("gamma", C.c_double), ("lam", C.c_double)] + [
        (n, C.c_void_p) for n in ("keys", "values", "steps", "lengths", "deltas", "acc", "stats")] + [("reserved0", C.c_int64)]


class TfeNtApply(C.Structure):
    _fields_ = [("net", TfeNtNet), ("step", C.c_double), ("acc", C.c_void_p), ("reserved0", C.c_int64)]


class TfeNtLearnTc(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_games", C.c_int32), ("max_steps", C.c_int32), ("gamma", C.c_double), ("lam", C.c_double)] + [
        (n, C.c_void_p) for n in ("keys", "values", "steps", "lengths", "deltas", "acc", "acc_abs", "stats")] + [("reserved0", C.c_int64)]


class TfeNtLearnBacked(C.Structure):                                        # TfeNtLearnTc's fields in order, then `backed`
    _fields_ = TfeNtLearnTc._fields_ + [("backed", C.c_void_p)]


class TfeNtRestartPick(C.Structure):
    _fields_ = [("n_games", C.c_int32), ("max_steps", C.c_int32), ("env_seed", C.c_uint64), ("board_id0", C.c_uint64), ("fraction", C.c_double),
                ("min_length", C.c_int32), ("reserved0", C.c_int32)] + [(n, C.c_void_p) for n in ("keys", "lengths", "start", "picked")]


class TfeNtContinuePick(C.Structure):                                       # games continued across rounds
    _fields_ = [("n_games", C.c_int32), ("max_steps", C.c_int32), ("env_seed", C.c_uint64), ("board_id0", C.c_uint64), ("reserved0", C.c_int64)] + [
        (n, C.c_void_p) for n in ("keys", "steps", "lengths", "total_score", "start", "carry_score", "carry_moves", "finished")]


class TfeNtAccList(C.Structure):                                            # rank-parallel rounds: the sparse accumulator exchange
    _fields_ = [("n_entries", C.c_uint64), ("acc", C.c_void_p), ("acc_abs", C.c_void_p), ("capacity", C.c_uint64), ("list", C.c_void_p),
                ("stats", C.c_void_p), ("reserved0", C.c_int64)]


class TfeNtStages(C.Structure):                                           # weight sets by tile stage: beside the struct of a *_staged entry point
    _fields_ = [("n_stages", C.c_int32), ("threshold", C.c_uint8 * 4), ("reserved0", C.c_int64)]


class TfeNtApplyTc(C.Structure):
    _fields_ = [("net", TfeNtNet), ("step", C.c_double)] + [(n, C.c_void_p) for n in ("acc", "acc_abs", "e", "a", "tc_stats")] + [("reserved0", C.c_int64)]


class TfeNtEval(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_games", C.c_int32), ("max_steps", C.c_int32), ("gamma", C.c_double), ("epsilon", C.c_double)] + _TFE_NT_SEEDS + [
        (n, C.c_void_p) for n in ("summary", "max_tile_hist", "total_score", "lengths")] + [("reserved0", C.c_int64)]


class TfeNtSearch(C.Structure):
    _fields_ = [("net", TfeNtNet), ("n_boards", C.c_int32), ("reserved0", C.c_int32), ("gamma", C.c_double), ("tie_seed", C.c_uint64),
                ("round", C.c_uint64)] + [(n, C.c_void_p) for n in ("boards", "q", "action", "candidates")] + [("reserved1", C.c_int64)]


# every symbol include/pulse_env.h declares: (restype, argtypes)
_P, _I32, _U32, _U64, _F32, _I64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_float, C.c_int64
SYMBOLS = {
    "pulse_version": (C.c_int, []),
    "pulse_last_error": (C.c_char_p, []),
    "pulse_handranks_generate": (C.c_int, [_P, C.c_int]),
    "pulse_poker_eval_hands": (C.c_int, [_P, _I32, _P, _I32, _I32, _I32, _P, _P]),
    "pulse_poker_eval_closed_form": (C.c_int, [_P, _I32, _I32, _P, _P]),
    "pulse_poker_step": (C.c_int, [_P, _P, _P, _P]),
    "pulse_poker_phases": (C.c_int, [_P, _U32, _P, _P, _P, _P]),
    "pulse_poker_reset": (C.c_int, [_P, _P, _P]),
    "pulse_poker_policy": (C.c_int, [_P, _I32, _P, _I32, _P, _I32, _U64, _U64, _U64, _P, _P]),
    "pulse_poker_policy_step": (C.c_int, [_P, _P, _U64, _U64, _U64, _P, _P, _P]),
    "pulse_poker_rollout": (C.c_int, [_P, _P, _P, _U64, _U64, _U64, _P, _P, _P, _I32, _P, _P, _P]),
    "pulse_poker_rollout_until": (C.c_int, [_P, _P, _P, _U64, _U64, _U64, _P, _P, _P, _I32, _I32, _P, _I32, _P, _P, _P, _P]),
    "pulse_timer_create": (C.c_int, [_P]),
    "pulse_timer_collect": (C.c_int, [_P, _P, _P, _P]),
    "pulse_timer_destroy": (C.c_int, [_P]),
    "pulse_stoprule_create": (C.c_int, [_I32, _I64, C.c_double, _I32, _P, C.c_char_p, _I32, _I32, _P]),
    "pulse_stoprule_submit": (C.c_int, [_P, _P, _I32, _P]),
    "pulse_stoprule_counts": (C.c_int, [_P, _P, _P, _P]),
    "pulse_stoprule_decide": (C.c_int, [_P, _P]),
    "pulse_stoprule_drain": (C.c_int, [_P]),
    "pulse_stoprule_publish": (C.c_int, [_P]),
    "pulse_stoprule_destroy": (C.c_int, [_P]),
    "pulse_stoprule_mode": (C.c_int, [_P]),
    "pulse_stoprule_side_launches": (_I64, [_P]),
    "pulse_stoprule_set_option": (C.c_int, [_P, _I32, _I64]),
    "pulse_stoprule_stats": (C.c_int, [_P, _P]),
    "pulse_stoprule_long_stats": (C.c_int, [_P, _P]),
    "pulse_shm_create": (C.c_int, [C.c_char_p, _I32, _I32, _P]),
    "pulse_shm_all_sum": (C.c_int, [_P, _I64, _I64, _P]),
    "pulse_shm_set_device": (C.c_int, [_P, C.c_char_p]),
    "pulse_shm_device_is_private": (C.c_int, [_P, _I32]),
    "pulse_shm_destroy": (C.c_int, [_P]),
    "pulse_comm_unique_id": (C.c_int, [_P]),
    "pulse_comm_create": (C.c_int, [_P, _I32, _I32, _P]),
    "pulse_comm_all_reduce_i64": (C.c_int, [_P, _P, _P, _I32, _P]),
    "pulse_comm_destroy": (C.c_int, [_P]),
    "pulse_poker_ablate": (C.c_int, [_P, _U32, _P, _P, _U64, _U64, _P]),
    "pulse_qnet_called_off_meetings": (_I64, []),
    "pulse_poker_act_policy_step": (C.c_int, [_P, _P, _U64, _U64, _U64, _P, _P, _P, _P, _P, _P]),
    "pulse_calib_stream": (C.c_int, [_P, _U64, _I32, _P]),
    "pulse_poker_stats": (C.c_int, [_P, _P, _P, _I32, _P, _P, _P]),
    "pulse_poker_hand_metrics": (C.c_int, [_P, _P, _P, _I32, _P, _P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _P]),
    "pulse_blackjack_reset": (C.c_int, [_P, _P, _P, _U64, _U64, _P]),
    "pulse_blackjack_step": (C.c_int, [_P, _P, _P]),
    "pulse_blackjack_mc_rollout": (C.c_int, [_P, _P]),
    "pulse_blackjack_mc_control_rollout": (C.c_int, [_P, _P]),
    "pulse_blackjack_mc_improve": (C.c_int, [_P, _P]),
    "pulse_tfe_reset": (C.c_int, [_P, _P, _I32, _I32, _U64, _U64, _P]),
    "pulse_tfe_step": (C.c_int, [_P, _P, _P, _P, _P, _I32, _I32, _U64, _U64, _U64, _P]),
    "pulse_tfe_mc_rollout": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_learn": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_rollout_canon": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_evaluate": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_table_merge": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_rollout_after": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_rollout_after_canon": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_learn_after": (C.c_int, [_P, _P]),
    "pulse_tfe_mc_evaluate_after": (C.c_int, [_P, C.c_double, _P]),
    "pulse_tfe_mc_table_fold_after": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_rollout": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_learn": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_learn_lambda": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_apply": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_learn_tc": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_apply_tc": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_evaluate": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_search": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_evaluate_search": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_search_deep": (C.c_int, [_P, _I32, _P]),
    "pulse_tfe_nt_evaluate_search_deep": (C.c_int, [_P, _I32, _P]),
    "pulse_tfe_nt_search_adaptive": (C.c_int, [_P, _I32, _P]),
    "pulse_tfe_nt_evaluate_search_adaptive": (C.c_int, [_P, _I32, _P, _P]),
    "pulse_tfe_nt_rollout_search": (C.c_int, [_P, _I32, _P]),
    "pulse_tfe_nt_rollout_backed": (C.c_int, [_P, _I32, _P, _P]),
    "pulse_tfe_nt_learn_backed": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_rollout_from": (C.c_int, [_P, _I32, _P, _P, _P]),
    "pulse_tfe_nt_rollout_adaptive": (C.c_int, [_P, _I32, _P, _P, _P, _P]),
    "pulse_tfe_nt_restart_pick": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_rollout_staged": (C.c_int, [_P, _P, _I32, _P, _P, _P]),
    "pulse_tfe_nt_learn_staged": (C.c_int, [_P, _P, _P]),
    "pulse_tfe_nt_evaluate_staged": (C.c_int, [_P, _P, _I32, _P]),
    "pulse_tfe_nt_search_staged": (C.c_int, [_P, _P, _P]),
    "pulse_tfe_nt_continue_pick": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_acc_pack": (C.c_int, [_P, _P]),
    "pulse_tfe_nt_acc_unpack": (C.c_int, [_P, _P]),
    "pulse_qtable_select": (C.c_int, [_P, _P, _I32, _I32, C.c_double, _U64, _U64, _U64, _P, _P, _P]),
    "pulse_qtable_update": (C.c_int, [_P, _P, _U64, _P, _P, _P, _P, _P, _I32, _I32, C.c_double, C.c_double, _P]),
    "pulse_qtable_rollout_step": (C.c_int, [_P, _P, _U64, _P, _P, _I32, _I32, C.c_double, C.c_double, C.c_double, _U64, _U64, _U64, _U64, _U64,
                                            _P, _P, _P, _P, _P]),
    "pulse_particle2d_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _I32, _F32, _I32, _P]),
    "pulse_qnet_forward": (C.c_int, [_P, _P, _I64, _I32, _P, _P]),
    "pulse_qnet_act": (C.c_int, [_P, _P, _I64, _I32, _P, _I32, _F32, _U64, _U64, _U64, _P, _P, _P, _P, _P]),
    "pulse_qnet_act_select": (C.c_int, [_P, _P, _I64, _I32, _P, _I32, _F32, _U64, _U64, _U64, _P, _P, _P, _P, _I64, _P]),
    "pulse_qnet_param_count": (C.c_int, [_I32, _I32]),
    "pulse_qnet_slice_floats": (C.c_int, []),
    "pulse_qnet_train_step": (C.c_int, [_P, _P, _I64, _P, _P, _P, _I64, _P, _P, _I32, _U64, _U64, _U64, _P, _P, _P]),
    "pulse_qnet_train_grads": (C.c_int, [_P, _P, _I64, _P, _P, _P, _I64, _P, _P, _I32, _U64, _U64, _U64, _P, _P, _P]),
    "pulse_qnet_train_apply": (C.c_int, [_P, _P]),
}


def build(force: bool = False) -> Path:
    """Compile libpulse_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = list(_CSRC.glob("*.hip")) + list(_CSRC.glob("*.cpp")) + list(_CSRC.glob("*.h")) + [_PKG.parent / "include" / "pulse_env.h"]
    if force or not _SO.exists() or any(s.stat().st_mtime > _SO.stat().st_mtime for s in srcs):
        subprocess.check_call(["make", "-C", str(_CSRC), f"-j{min(8, os.cpu_count() or 1)}"] + (["-B"] if force else []))
    return _SO


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not _SO.exists():
            if os.environ.get("PULSE_NO_AUTOBUILD"):
                raise PulseError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
            build()
        # PyTorch-ROCm ships its own libamdhip64; it must be in the process before this library resolves its HIP
        # dependency, or two HIP runtimes coexist and launches on torch's tensors fail ("no ROCm-capable device")
        import torch  # noqa: F401
        try:
            handle = C.CDLL(str(_SO))
        except OSError as e:  # pragma: no cover - environment specific
            raise PulseError(f"cannot load {_SO}: {e} (the HIP library is required; there is no CPU fallback)") from e
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)   # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if handle.pulse_version() != 1:
            raise PulseError("libpulse_hip.so ABI version mismatch")
        _LIB = handle
    return _LIB


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().pulse_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise PulseError(f"{what}: {msg} (code {rc})")


def gpu_device(device, who: str):
    """`device` as a torch.device with its index filled in; `who` (a class of the package) refuses anything but a 'cuda' device."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"pulselib_amd.{who} runs on an MI355X ('cuda' device); got '{device}'. No CPU fallback.")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def current_stream(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
