/*
 * pulse_env.h -- C ABI of libpulse_hip.so, the MI355X (gfx950) batched env-step engine.
 *
 * Drop-in boundary for the hot path of cerredz/Pulselib: each entry point replaces one chain of
 * eager torch ops in the reference (file:line given per function, relative to the reference
 * checkout).  Plain pointers and sizes only; all device buffers are allocated and owned by the
 * caller (PyTorch-ROCm in the shipped host code, anything else that can hand out HBM pointers
 * works too).  Every launch is enqueued on the caller's hipStream_t and returns without a host
 * sync.  Return value: 0 on success, negative PULSE_E* on error (message: pulse_last_error()).
 * The library never throws across this boundary and keeps no per-call device allocations.
 *
 * There is no CPU fallback: without a usable HIP device the launch functions return
 * PULSE_ENODEVICE.  (pulse_handranks_generate is a host-side data-file builder, not a fallback.)
 */
#ifndef PULSE_ENV_H
#define PULSE_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PULSE_ABI_VERSION 1

#define PULSE_EINVAL    (-1)   /* bad argument (shape / null pointer / unsupported size)            */
#define PULSE_ENODEVICE (-2)   /* no HIP device / HIP runtime error before launch                   */
#define PULSE_ELAUNCH   (-3)   /* hipLaunchKernel / hipGetLastError reported an error               */
#define PULSE_EINTERNAL (-4)

#define PULSE_HANDRANKS_LEN 32487834   /* int32 entries of HandRanks.dat (PokerGPU.py:51-57)        */
#define PULSE_MAX_SEATS     16         /* seats per table the kernels support (reference default 10) */

/* Seat status codes, environments/Poker/PokerGPU.py:11 */
enum { PULSE_ACTIVE = 0, PULSE_FOLDED = 1, PULSE_ALLIN = 2, PULSE_SITOUT = 3 };

/* Agent types for pulse_poker_policy, environments/Poker/utils.py:80-87 (+ Player.py:79-176) */
enum {
    PULSE_AGENT_EXTERNAL = 0,        /* seat is played by the caller (Q-network): action left untouched */
    PULSE_AGENT_RANDOM = 1,          /* utils.py:121                 */
    PULSE_AGENT_HEURISTIC_HANDS = 2, /* Player.py:79-104             */
    PULSE_AGENT_TIGHT_AGGRESSIVE = 3,/* Player.py:106-126            */
    PULSE_AGENT_LOOSE_PASSIVE = 4,   /* Player.py:128-151            */
    PULSE_AGENT_SMALL_BALL = 5       /* Player.py:153-176            */
};

/*
 * Device view of one PokerGPU instance: the reference's own SoA tensors
 * (environments/Poker/PokerGPU.py:81-155), row-major, device pointers.
 *   [N]      int32 : pots stages deck_positions button sb bb idx highest agg acted
 *                    last_raise_size prev_stacks prev_invested
 *   [N]      uint8 : is_done (torch.bool), equity_dirty (torch.bool)
 *   [N,P]    int32 : stacks current_round_bet total_invested status
 *   [N,P,2]  int32 : hands          [N,5] int32 : board        [N,52] int32 : decks (cards 1..52)
 *   [N,A]    fp32  : equities       [N,obs_size] fp32 : obs (obs_size = 13 + 3*(max_players-1))
 *   hand_ranks: int32[hand_ranks_len], the 2+2 table (PokerGPU.py:47-58)
 *   w1,w2 (fp32) K,alpha (int32): 0-d device tensors, read by the kernel at every step because
 *   callers re-assign them (tests/poker/test_poker_gpu_round_progression.py:207-210).
 * is_done_out may alias is_done (in-place) or be a second buffer (the host code ping-pongs two so
 * that the tensor returned by step() is not rewritten by the next step, as in PokerGPU.py:619-623).
 */
/* flags: kernel variants a caller (or a test) selects per view; 0 = the product defaults */
#define PULSE_VIEW_NO_OBS_STAGING 0x1  /* store the observation column by column instead of LDS-staged 16-byte bursts  */
#define PULSE_VIEW_NO_CHUNK       0x2  /* pulse_poker_rollout: one launch per step instead of one launch per chunk     */
#define PULSE_VIEW_FOUR_LANES     0x4  /* chunk launches: four lanes per table also where two are the default (<= 10 seats) */
#define PULSE_VIEW_NO_PAIRS       0x8  /* pulse_poker_rollout_until: one check interval per launch instead of two (lag 1)  */
#define PULSE_VIEW_NO_LONG_LAUNCHES 0x10 /* pulse_poker_rollout_until: at most two check intervals per launch (PULSE_STOPRULE_OPT_LONG_LAUNCHES) */
typedef struct PulsePokerView {
    int32_t n_games, n_players, active_players, max_players;   /* n_games <= 2^24 per view (shard larger batches) */
    int32_t obs_size, hand_ranks_len;
    int32_t flags, reserved0;
    const int32_t* hand_ranks;
    int32_t *pots, *stages, *deck_positions, *button, *sb, *bb, *idx, *highest, *agg, *acted,
            *last_raise_size, *prev_stacks, *prev_invested;
    uint8_t *is_done, *is_done_out, *equity_dirty;
    int32_t *stacks, *current_round_bet, *total_invested, *status;
    int32_t *hands, *board;
    const int32_t* decks;
    float *equities, *obs;
    const float *w1, *w2;
    const int32_t *K, *alpha;
    /* Optional evaluation cache (all four NULL = disabled), owned by the caller like the rest, opaque to
     * it: pulse_poker_reset walks the table once per episode (board first, which reaches the same table
     * state as the reference's hole-cards-first order for any distinct cards) and stores, per table, the
     * board it will deal (pre_board [N], packed cards + valid bit) and, per seat, the hole cards used
     * (pre_hands [N,P]), the three street equities (pre_eq [N,3,P], PokerGPU.py:455-525) and the 7-card
     * rank (pre_rank [N,P], PokerGPU.py:437-444).  The step kernel uses an entry only if the cards it
     * finds in `board` / `hands` at that moment are exactly the cached ones, else it does the reference's
     * literal gather chain -- so poked states stay bit-exact and the common path needs no table gathers. */
    int32_t *pre_board, *pre_hands;
    float *pre_eq;
    int32_t *pre_rank;
} PulsePokerView;

/* Phase bits for pulse_poker_phases: the white-box methods the reference's tests call directly. */
#define PULSE_PH_CAPTURE   0x001u  /* PokerGPU.py:530-539  prev_done / actor / prev_stacks / prev_invested */
#define PULSE_PH_EQUITY    0x002u  /* PokerGPU.py:455-525  calculate_equities                             */
#define PULSE_PH_EXECUTE   0x004u  /* PokerGPU.py:230-303  execute_actions                                */
#define PULSE_PH_ADVANCE   0x008u  /* PokerGPU.py:547-616  next actor, round close, street transition     */
#define PULSE_PH_FOLDWIN   0x010u  /* PokerGPU.py:331-338  resolve_fold_winners                           */
#define PULSE_PH_SHOWDOWN  0x020u  /* PokerGPU.py:380-453  resolve_terminated_games + :340-378 side pots  */
#define PULSE_PH_CLEARDONE 0x040u  /* PokerGPU.py:625-628                                                 */
#define PULSE_PH_REWARD    0x080u  /* PokerGPU.py:305-329,:631-632 poker_reward_gpu                       */
#define PULSE_PH_OBS       0x100u  /* PokerGPU.py:159-179  get_obs                                        */
#define PULSE_PH_STEP      0x1FFu  /* all of the above in reference order = PokerGPU.step :527-633        */

int pulse_version(void);
const char* pulse_last_error(void);

/* Host: build the 2+2 table (replaces the HandRanks.dat download, PokerGPU.py:47-58).
 * out = host int32[PULSE_HANDRANKS_LEN].  Deterministic; n_threads<=0 = all cores. */
int pulse_handranks_generate(int32_t* out, int n_threads);

/* Standalone 5/6/7-card lookup kernel (PokerGPU.py:437-444, :497-500, :518-521):
 * cards device int32[n_hands,n_cards]; out device int32[n_hands]; n_cards 7 -> raw chain value,
 * 6 -> HR[p], 5 -> HR[p] (flop_double=0) or HR[HR[p]] (flop_double=1). */
int pulse_poker_eval_hands(const int32_t* hand_ranks, int32_t hand_ranks_len, const int32_t* cards,
                           int32_t n_hands, int32_t n_cards, int32_t flop_double, int32_t* out, void* stream);

/* The closed-form evaluator the reset kernel fills its evaluation cache with (csrc/hand_eval_device.h: the evaluator
 * the table is generated from), alone, for the tests that hold it to the table walk: cards device
 * int32[n_hands,n_cards] of 5..7 DISTINCT cards in 1..52; out[i] = category << 12 | index, what the walk of
 * PokerGPU.py:437-444 returns for them (n_cards 5 / 6: HR[p] after the last card).  Diagnostic, not drop-in surface. */
int pulse_poker_eval_closed_form(const int32_t* cards, int32_t n_hands, int32_t n_cards, int32_t* out, void* stream);

/* PokerGPU.step (PokerGPU.py:527-633), one fused launch.  actions device int64[N] (any value; <0 =
 * no-op, >12 = raise of 0 as in the reference's masks), rewards device fp32[N] out. */
int pulse_poker_step(const PulsePokerView* v, const int64_t* actions, float* rewards, void* stream);

/* Run a subset of step()'s phases in reference order (white-box methods).  For FOLDWIN/SHOWDOWN
 * without CAPTURE the "newly done" mask is is_done itself, as in PokerGPU.py:333,386.  actor_idx
 * (device int32[N]) is used by REWARD when CAPTURE is absent (PokerGPU.py:305), else NULL. */
int pulse_poker_phases(const PulsePokerView* v, uint32_t phases, const int64_t* actions,
                       const int32_t* actor_idx, float* rewards, void* stream);

/* PokerGPU.reset (PokerGPU.py:73-157) after the host picked active_players (v->active_players).
 *   first          : 1 = no previous episode (stacks := starting_bbs, button := 0)           (:101-102,:121)
 *   prefixed_decks : device int32[N,52] copied into v->decks, or NULL = shuffle on device with
 *                    Philox4x32-10(seed, table id + table_id0, episode) (replaces rand().argsort, :86)
 *   decks_out      : v->decks is const in the view; reset writes through this pointer.
 *   rotation       : torch.roll shift of the stack rows                                     (:104-110)
 *   shuffle_key_bits : the device shuffle orders the 52 cards of a table by the top 26 bits of one Philox word each
 *                    (torch.rand's keys have 24), equal keys keeping card order; 1..25 keeps fewer bits and so
 *                    forces ties: a hook for the tests of the tie-break, not for production use.  0 = 26.
 *   stats_rewards / stats_out : NULL, or the episode statistics of the episode that ENDS here, taken before the state
 *                    is overwritten: the sum of stats_rewards[t] (device fp32[n_games], the last step's rewards) and the
 *                    number of tables with is_done (what a rank all-reduces per episode, scripts/Poker/trainGPU.py:96,
 *                    104) are ADDED into stats_out, device double[PULSE_STATS_SLOTS * PULSE_STATS_STRIDE]: accumulator k
 *                    is {stats_out[k * STRIDE] = reward sum, stats_out[k * STRIDE + 1] = done count}, a wavefront adds to
 *                    accumulator (its index mod SLOTS); the total is the sum over k.  (Spread because same-address
 *                    atomics serialise.)  No launch of its own. */
#define PULSE_STATS_SLOTS 256
#define PULSE_STATS_STRIDE 16
typedef struct PulsePokerResetOpts {
    int32_t first, starting_bbs, max_bbs, rotation;
    uint64_t seed, episode, table_id0;
    const int32_t* prefixed_decks;
    int32_t* decks_out;
    int32_t shuffle_key_bits, reserved0;
    const float* stats_rewards;
    double* stats_out;
} PulsePokerResetOpts;
int pulse_poker_reset(const PulsePokerView* v, const PulsePokerResetOpts* o, void* stream);

/* build_actions + scripted opponents (environments/Poker/utils.py:108-123, Player.py:79-176):
 * obs device fp32[n,obs_stride] (columns 5,6 = hole cards, 9 = pot), seat_idx device int32[n] (the
 * `curr_players` argument).  For every table whose seat has a scripted type, actions[t] is written;
 * EXTERNAL seats are left untouched.  agent_types: host uint8[n_players] (PULSE_AGENT_*).
 * Random draws (the scripted-opponent stream): call = Philox4x32-10(seed, table id + table_id0, step_counter >> 1);
 * an even step_counter takes words (x, y) of the call, an odd one (z, w) -- x/z feed the action's randint, y/w
 * loose_passive's rand() (Player.py:146).  One call serves two steps: the chunked roll-out draws eight steps in one pass. */
int pulse_poker_policy(const float* obs, int32_t obs_stride, const int32_t* seat_idx, int32_t n,
                       const uint8_t* agent_types, int32_t n_players, uint64_t seed, uint64_t step_counter,
                       uint64_t table_id0, int64_t* actions, void* stream);

/* Fused roll-out step for scripted tables: policy (above) + step in ONE launch; actions[] is both
 * input (EXTERNAL seats) and output (what was played).  Same results as policy followed by step. */
int pulse_poker_policy_step(const PulsePokerView* v, const uint8_t* agent_types, uint64_t seed, uint64_t step_counter,
                            uint64_t table_id0, int64_t* actions, float* rewards, void* stream);

/* Roll-out: n_steps fused policy+step transitions enqueued by ONE native call and, by default, executed by ONE
 * launch: every table's state is loaded once, stepped n_steps times in registers and its changed words stored once,
 * while step i's observation, reward and done flag belong into the even buffers (v_even->obs, v_even->is_done_out,
 * rewards_even) when i is even, else into the odd ones (v_odd->obs, v_odd->is_done_out, rewards_odd).
 * The contract (this call and pulse_poker_rollout_until): memory after the call is bit-identical to calling
 * pulse_poker_policy_step n_steps times on v_even, v_odd, v_even, ... (PULSE_VIEW_NO_CHUNK in v_even->flags does exactly
 * that instead); outputs that a later step of the same call overwrites are not materialised.
 * v_odd must be v_even with is_done <-> is_done_out swapped (obs may differ: double-buffered observations).
 * Draws of step i: the scripted-opponent stream at step_counter0 + i (pulse_poker_policy).
 * timer (NULL or a pulse_timer_create handle): the call is bracketed by one HIP event pair on `stream`; read the
 * summed time, the launches and the steps covered with pulse_timer_collect() AFTER synchronising the stream.
 * stoprule (NULL or a pulse_stoprule_create handle): the tables done after the last step are counted for it by the
 * launch itself (each wavefront stores its count; no extra kernel on `stream`). */
int pulse_poker_rollout(const PulsePokerView* v_even, const PulsePokerView* v_odd, const uint8_t* agent_types,
                        uint64_t seed, uint64_t step_counter0, uint64_t table_id0, int64_t* actions,
                        float* rewards_even, float* rewards_odd, int32_t n_steps, void* timer, void* stoprule,
                        void* stream);
/* The trainer's inner loop (scripts/Poker/trainGPU.py:79-108) for scripted tables, natively: roll-out chunks of
 * chunk_steps (the reference's check interval, 5) are enqueued, each followed by the stop rule's verdict
 * (pulse_stoprule_decide), until the rule ends the episode or max_steps steps have run -- no interpreter between the
 * chunks.  *steps_done: steps executed (the caller's views / reward buffers have swapped roles if it is odd);
 * *over: the rule fired.  timer + time_every > 0: every time_every-th chunk opens a HIP-event bracket over the next
 * eight chunks of the call (an event pair around every single launch costs the stream a fifth of the launch).
 * With a lag-1 rule (and unless the view says PULSE_VIEW_NO_PAIRS) ONE launch runs up to TWO check intervals: under
 * the fixed-lag rule a chunk runs iff the count two check points back did not end the episode, and both counts a
 * two-chunk launch needs belong to launches that have completed when it starts -- its first workgroup sums and
 * publishes them, the host answers with the launch's verdict word in pinned memory, and every wavefront reads the
 * relayed word before its first store (the launch then runs two chunks, one, or none).  Episodes come out step for
 * step as with one chunk per launch; the state is loaded and written back half as often.
 * That launch is the one place where device code waits for the host (the word arrives ~5 us after the launch starts).  The
 * wait is bounded (PULSE_STOPRULE_OPT_VERDICT_WAIT_TICKS, 20 s by default) and the host decides by its own clock which side
 * of the bound it is on: a host that is later than half the wait after the enqueue (a stalled rank, a stopped process) does
 * NOT write the word, lets the launch give up -- it then runs nothing and stores nothing --, counts a time-out
 * (pulse_stoprule_stats) and runs these and all further steps of the handle's life with one check interval per launch, which
 * never waits in a kernel.  Same episodes either way.  Ranks that share one device (shm exchange) never pair. */
int pulse_poker_rollout_until(const PulsePokerView* v_even, const PulsePokerView* v_odd, const uint8_t* agent_types,
                              uint64_t seed, uint64_t step_counter0, uint64_t table_id0, int64_t* actions,
                              float* rewards_even, float* rewards_odd, int32_t chunk_steps, int32_t max_steps, void* timer,
                              int32_t time_every, void* stoprule, void* stream, int32_t* steps_done, int32_t* over);
int pulse_timer_create(void** timer);
int pulse_timer_collect(void* timer, float* sum_ms, int32_t* n_launches, int64_t* n_steps);
int pulse_timer_destroy(void* timer);

/* The trainer's episode stop rule (scripts/Poker/trainGPU.py:27-33,99: every 5th step, more than `threshold` of the
 * tables done ends the episode) without its blocking read, for one GPU or for one process per GPU.
 * A "check point" is one evaluation of the rule.  pulse_poker_rollout (or submit) leaves the check point's done
 * tables counted per wavefront on the device; the NEXT launch on that stream sums them in its first workgroup (before that workgroup's own tables) and
 * writes the count + a sequence number into coherent pinned host memory, which decide()/counts() poll -- no event,
 * no second stream, no kernel of its own between the steps' launches, and the host sees a count a microsecond after
 * it exists.  decide() answers for the check point submitted `lag` check points before the newest one: a FIXED lag,
 * so a run is reproducible and every rank of a job takes every decision on the same check point and ends every
 * episode at the same step (equal collective sequences on all ranks).  lag 0 is the reference's blocking check (the
 * count is then flushed by a kernel of its own); lag 1 (default of the host code) never waits in practice.
 * Between the ranks of a job the counts are exchanged
 *   - through a POSIX shared-memory segment (shm_name, rank, world: one cache line per rank and check point; the
 *     ranks of one node; 8 bytes every 5 steps need no device), or
 *   - by an RCCL all-reduce on a side stream of the rule (comm: a pulse_comm_create handle; an event hands each check
 *     point over to that stream, which costs the steps' stream a barrier per check point), or
 *   - by the caller: counts() returns the check point's local count, to be all-reduced by the host code (gloo).
 * counts(): have = 0 while no check point of this episode is due.  drain() marks an episode boundary: earlier check
 * points decide nothing any more.  n_global = tables of the whole job.  The handle owns < 1 MB of device / pinned
 * memory (and, RCCL only, a stream and 8 events), created on the current device. */
int pulse_stoprule_create(int32_t n_local, int64_t n_global, double threshold, int32_t lag, void* comm, const char* shm_name,
                          int32_t rank, int32_t world, void** handle);
int pulse_stoprule_submit(void* handle, const uint8_t* flags, int32_t n, void* stream);   /* flags: device uint8[n], != 0 = done */
int pulse_stoprule_counts(void* handle, int64_t* local, int64_t* global, int32_t* have);
int pulse_stoprule_decide(void* handle, int32_t* over);
/* Publishes the newest check point's count NOW (a one-workgroup launch on the stream that wrote its partial counts) instead
 * of leaving it to the next launch that carries the rule: for a caller whose next such launch is far away (the trainer: every
 * fifth step), so that the verdict due then finds its count long published and waits for nothing. */
int pulse_stoprule_publish(void* handle);
int pulse_stoprule_drain(void* handle);
int pulse_stoprule_destroy(void* handle);
/* How the handle exchanges its counts: 0 = local (one process), 1 = RCCL side stream (any communicator, also of one
 * rank), 2 = shared memory; side_launches = check points that went through the side stream so far (tests assert the
 * RCCL leg really ran). */
int pulse_stoprule_mode(void* handle);
int64_t pulse_stoprule_side_launches(void* handle);
/* Options of a handle.  VERDICT_WAIT_TICKS: how long a paired launch (pulse_poker_rollout_until) waits for its host's verdict,
 * in ticks of the device's 100 MHz clock (default 2,000,000,000 = 20 s; >= 100,000).  ALLOW_SHARED_DEVICE_PAIRS (0 / 1):
 * with the shm exchange, ranks whose GPU (PCI bus id, told to the segment at create time) is also another rank's do not pair,
 * since their launches wait for hosts that wait for every rank's launch to have started and the grids of several processes
 * need not fit one device together; 1 lifts that for grids known to fit (tests).  DEBUG_LATE_VERDICTS (test hook): the next
 * `value` verdicts are treated as "the host is too late": the launch gives up, the handle falls back.
 * stats: out4 = {paired launches issued, verdict time-outs, 1 if the handle would still pair, side-stream check points}. */
#define PULSE_STOPRULE_OPT_VERDICT_WAIT_TICKS        0
#define PULSE_STOPRULE_OPT_ALLOW_SHARED_DEVICE_PAIRS 1
#define PULSE_STOPRULE_OPT_DEBUG_LATE_VERDICTS       2
/* Long launches (pulse_poker_rollout_until; a lag-1 rule of ONE process whose tables are the whole job): a call that has
 * more than one pair's worth of full check intervals left enqueues all the intervals its pairs would cover as ONE launch
 * (the rest of the call, less than two intervals, runs as before: a call returns the same steps and `over` either way).  Its start is the paired launch's (the host's word decides
 * about the first two chunks); from the third chunk on the launch takes the rule's verdicts itself: at a check point every
 * wavefront adds its done count to an arrival word, the wavefront that completes the arrivals compares the total with the
 * rule's threshold and writes the verdict every wavefront reads before the chunk after the next.  Wavefronts wait for each
 * other there, so the mode is used only where every workgroup of the launch is on the device at once: what
 * hipOccupancyMaxActiveBlocksPerMultiprocessor answers for the chunk kernel MINUS ONE workgroup (the query can answer one
 * more than the hardware admits), times the compute units, must cover the grid -- 65,536 tables on an MI355X, not more.  The
 * wait is bounded by VERDICT_WAIT_TICKS, and by 100 ms where that is longer (wavefronts of one launch are microseconds apart; a
 * workgroup kept off the device by another stream's or process's kernels is what such a wait would mean): a wavefront whose wait runs out calls the check point off (one compare-and-swap
 * decides between it and the verdict), the launch ends behind the chunk it is in, exactly as if it had been planned that
 * long, the episode goes on with paired launches and the handle plans no long launch again.  Same episodes either way.
 * LONG_LAUNCHES (0 / 1, default 1).  DEBUG_SKIP_DECISION (test hook, one-shot): in the next long launch nobody decides
 * check point `value` (1 = the launch's first; 0 = none), so its waiters run into the bound and call it off.
 * DEBUG_RESIDENT_BLOCKS (test hook): the occupancy answer to assume (0: ask the device).
 * EARLY_VERDICTS (0 .. 3, default 1): of a long launch only the two steps in front of an end it can still take compute and
 * store rewards, observations and done flags.  On, the launch's first check point (which reads no verdict and so ends nothing)
 * is no such end, and before the two steps in front of every later check point a wavefront looks -- one load, no loop -- whether
 * the verdict that check point will read is settled already: "go on" makes the check point no end either (the two steps run
 * without outputs, the check point reads nothing and arrives), "over" or "called off" ends the launch there as the check
 * point's own read would, and a pending word leaves everything to that read.  Memory behind a call is the same in every case.
 * 0: no look, every check point a possible end (the A/B twin).  2: as 1, and the launches count the looks that found their
 * word settled / pending (long_stats; test use: two atomic adds per wavefront and check point).  3: as 2, but odd-numbered
 * wavefronts treat every look as pending: both paths inside one launch.
 * long_stats: out6 = {long launches issued, verdicts taken in-launch, check points called off, 1 if the handle would
 * still plan long launches (the residency of a grid is only known per call), early looks that found the verdict settled, early
 * looks that found it pending (both 0 unless EARLY_VERDICTS has been 2 or 3; reading them waits for the launches' stream)};
 * PULSE_EINTERNAL if a launch told the host its chunk count more than once (it must not: the device counts its writes of that word). */
#define PULSE_STOPRULE_OPT_LONG_LAUNCHES             3
#define PULSE_STOPRULE_OPT_DEBUG_SKIP_DECISION       4
#define PULSE_STOPRULE_OPT_DEBUG_RESIDENT_BLOCKS     5
#define PULSE_STOPRULE_OPT_EARLY_VERDICTS            6
int pulse_stoprule_set_option(void* handle, int32_t option, int64_t value);
int pulse_stoprule_stats(void* handle, int64_t* out4);
int pulse_stoprule_long_stats(void* handle, int64_t* out6);

/* The shared-memory exchange of the stop rule as an object of its own (host code only; the rule creates one itself when
 * given shm_name).  Every rank maps the POSIX segment `name` (created by whoever comes first; unlink it once all ranks
 * have it mapped) and calls all_sum with the same sequence of indices 0, 1, 2, ...: *total = sum of the ranks' values. */
int pulse_shm_create(const char* name, int32_t rank, int32_t world, void** handle);
int pulse_shm_all_sum(void* handle, int64_t index, int64_t value, int64_t* total);
/* The segment also carries one record per rank naming the GPU the rank computes on (any string equal exactly for ranks on
 * one device; the rule stores the PCI bus id).  device_is_private: 1 = every rank has named its GPU within wait_ms and none
 * shares this rank's, 0 otherwise. */
int pulse_shm_set_device(void* handle, const char* bus_id);
int pulse_shm_device_is_private(void* handle, int32_t wait_ms);
int pulse_shm_destroy(void* handle);

/* RCCL communicator of the job (one process per GPU), for the stop rule's 8-byte all-reduce on its side
 * stream (the `comm` exchange above).  librccl is bound at run time (the copy PyTorch-ROCm loaded, else the system one), so the library loads
 * without it.  unique_id: call on rank 0, hand the 128 bytes to every rank (torch.distributed broadcast), then
 * every rank calls create (collective).  all_reduce_i64: sum of int64[count], device pointers, in `stream` order. */
int pulse_comm_unique_id(uint8_t* out128);
int pulse_comm_create(const uint8_t* id128, int32_t rank, int32_t world, void** comm);
int pulse_comm_all_reduce_i64(void* comm, const int64_t* send, int64_t* recv, int32_t count, void* stream);
int pulse_comm_destroy(void* comm);

/* Diagnostic only (tools/ablate_step.py): fused policy+step with phases compiled out, to price them. */
int pulse_poker_ablate(const PulsePokerView* v, uint32_t phases, int64_t* actions, float* rewards, uint64_t types_packed,
                       uint64_t step_counter, void* stream);

/* Diagnostic only (tools/pmc_calibrate.py): stream n_words dwords, one dword per lane, read (write=0) or
 * written (write=1), to calibrate rocprofv3 FETCH_SIZE / WRITE_SIZE on a known byte count. */
int pulse_calib_stream(int32_t* buf, uint64_t n_words, int32_t write, void* stream);

/* Episode statistics for the trainer's stop rule and returns (scripts/Poker/trainGPU.py:27-33,96):
 * stats device int64[2] += {#tables with is_done, 0}; fstats device double[1] += sum(rewards[mask]).
 * stats NULL: the done count goes to fstats[1] instead (double[2] = {reward sum, done count}: one tensor to all-reduce). */
int pulse_poker_stats(const uint8_t* is_done, const float* rewards, const uint8_t* mask, int32_t n,
                      int64_t* stats, double* fstats, void* stream);

/* Hand-level metrics side-channel (scripts/Poker/trainGPU_performance.py:198-206, utils/performance.py): for every
 * table with dones[t] && !terminated_before[t] (NULL = none terminated) the learner seat's chip delta
 * stacks[t][q_seat] - initial_q_stacks[t] is added to acc[position][bucket][4] = {hands, wins, sum delta, sum delta^2}
 * (device int64[16*5*4], zeroed by the caller when a new aggregation starts); position = (q_seat - button[t]) mod
 * active_players, bucket = clamp(stages[t], 0, 4).  No host sync; BB/100, win rates by street / position and the
 * confidence bound follow from the sums on the host (pulselib_amd/utils/performance.py).
 * The ordered hand log (optional; both NULL or both set): finish_step[t] = step_index and hand_delta[t] = the delta for
 * every table accounted in this call (device int32[n] each; the caller fills finish_step with -1 when an episode
 * starts).  Sorting the finished tables by (finish_step, t) gives the hands in the order the reference's per-step
 * boolean pulls append them -- what its rolling-window average runs over (utils/performance.py:128-135). */
int pulse_poker_hand_metrics(const uint8_t* dones, const uint8_t* terminated_before, const int32_t* stacks, int32_t n_players,
                             const int32_t* initial_q_stacks, const int32_t* stages, const int32_t* button, int32_t q_seat,
                             int32_t active_players, int32_t n, int64_t* acc, int32_t step_index, int32_t* finish_step,
                             int32_t* hand_delta, void* stream);

/* ---- Blackjack (environments/blackjack/blackjack.py) ------------------------------------------ */
typedef struct PulseBlackjackView {
    int32_t batch_size;
    const int32_t* decks;              /* [B,52] cards 0..51 (blackjack.py:24-29)                  */
    int32_t *deck_positions, *players_cards, *players_card_idx, *player_card_sums;
    int32_t *dealer_cards, *dealer_card_idx, *dealer_upcard, *dealer_card_sums;
    uint8_t *terminated, *has_ace, *dealer_has_ace;
    int32_t *rewards, *obs;            /* obs [B,3] int32                                          */
} PulseBlackjackView;
/* reset: decks_src NULL = device shuffle Philox(seed, game id, episode), else copied (blackjack.py:23-101) */
int pulse_blackjack_reset(const PulseBlackjackView* v, const int32_t* decks_src, int32_t* decks_out,
                          uint64_t seed, uint64_t episode, void* stream);
int pulse_blackjack_step(const PulseBlackjackView* v, const int64_t* actions, void* stream);   /* :113-186 */

/* ---- Blackjack: first-visit Monte-Carlo value estimation in one launch (agents/MonteCarlo/FirstVisitMonteCarlo.py:5-31 and the
 * reset / step / per-game learn() loop that feeds it).  One lane plays one game from the shuffle to the terminal step, n_episodes
 * episodes of n_games games per launch; the env's decks, card rows and per-game state are never written.  Game g of episode e is
 * the game pulse_blackjack_reset(seed, episode + e) + pulse_blackjack_step play: the same Fisher-Yates shuffle on
 * Philox4x32-10(seed, g, (episode + e) * 16 + (q >> 2)), the same deal / hit / stand / dealer rules.
 * The reward is 0 before the terminal step and +-1 at it, so the first-visit return of the state seen k steps before the terminal
 * step is r * gamma^k, and the launch COUNTS: acc[PULSE_BJ_MC_CELL(state, k, r < 0)] += 1 for the first visit of every state of
 * every game, with state = PULSE_BJ_MC_STATE_INDEX(player's sum, usable ace, dealer's upcard) -- the observation
 * (blackjack.py:103-108).  Integer adds only: the result is the same bit for bit whatever the order of the atomics.  The sum of
 * returns of a state follows on the host as sum over k of (acc[.., k, 0] - acc[.., k, 1]) * gamma^k, its count as the sum of both.
 *   acc      : device int64[PULSE_BJ_MC_ACC_LEN], 8-byte aligned, ADDED to, never cleared: the caller zeroes it when a new
 *              estimate starts (the convention of pulse_poker_hand_metrics).
 *   stats    : device int64[4], 8-byte aligned, added to: {games played, games won, actions taken, games capped}.
 *   hit_prob : device fp32[PULSE_BJ_MC_STATES], the policy: the probability of hitting in each state.  <= 0 (or NaN) = stand,
 *              >= 1 = hit, between = hit iff u < p with u = (w >> 8) * 2^-24, w = word (t & 3) of
 *              Philox4x32-10(seed ^ 0xB1AC7AC4D3A1E5, g, (episode + e) * 4 + (t >> 2)) for action t of the game -- the policy's
 *              own stream, keyed apart from the shuffle's; a word is only drawn where the table holds such a probability.
 *   decks_src: NULL = device shuffle, else device int32[n_episodes * n_games, 52], row e * n_games + g, used as it is (any
 *              int32, as pulse_blackjack_reset takes them).
 *   trace    : NULL, or device int8[n_episodes * n_games, PULSE_BJ_MC_MAX_ACTIONS], 16-byte aligned: row e * n_games + g holds
 *              the actions of that game (0 = hit, 1 = stand), then -1.  For tests and diagnostics; with NULL nothing is stored
 *              per game.
 *   max_blocks: 0 = two persistent workgroups per CU, else the largest grid (each workgroup loops over games and adds its
 *              histogram to acc once, at the end of the launch).
 * A game is capped at PULSE_BJ_MC_MAX_ACTIONS actions: one that has not ended by then records nothing and counts in stats[3]
 * (and in stats[0], not in stats[1..2]).  Cards 0..51 cannot get there; an injected deck of arbitrary values can.  Such values can
 * also lead to a state outside the layout below (a sum outside 0..31): the policy stands in it and its visit is not counted.
 * n_games * n_episodes < 2^32 per launch.  Zero-initialise the struct; reserved0 != 0 is PULSE_EINVAL. */
#define PULSE_BJ_MC_MAX_ACTIONS 16
#define PULSE_BJ_MC_STATES      1024       /* 32 sums x 2 x 16 upcards */
#define PULSE_BJ_MC_STATE_INDEX(sum, has_ace, upcard) ((((sum) * 2 + (has_ace)) * 16) + (upcard))   /* sum 0..31, upcard 0..15 */
#define PULSE_BJ_MC_CELL(state, k, negative) ((((state) * PULSE_BJ_MC_MAX_ACTIONS + (k)) * 2) + (negative))
#define PULSE_BJ_MC_ACC_LEN     (PULSE_BJ_MC_STATES * PULSE_BJ_MC_MAX_ACTIONS * 2)
typedef struct PulseBlackjackMC {
    int32_t n_games, n_episodes;
    uint64_t seed, episode;
    const float* hit_prob;
    const int32_t* decks_src;
    int64_t* acc;
    int64_t* stats;
    int8_t* trace;
    int32_t max_blocks, reserved0;
} PulseBlackjackMC;
int pulse_blackjack_mc_rollout(const PulseBlackjackMC* o, void* stream);

/* ---- Blackjack: on-policy first-visit Monte-Carlo CONTROL on the device (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71): the
 * roll-out above counting first visits of (state, action) PAIRS, and the policy improvement as a launch of its own, so that
 * roll-out -> improve -> roll-out runs without a host round trip.
 * pulse_blackjack_mc_control_rollout plays the games pulse_blackjack_mc_rollout plays -- same shuffle, same policy stream, same
 * cap, trace and stats, same fields with the same meanings and checks -- and counts action t at state s iff no earlier action of
 * that game was the same action at the same state.  A stand ends the game, so it is only ever seen k = 0 steps before the
 * terminal reward: a state has the 32 cells (k, sign) of its hits and 2 cells (sign) of its stands,
 *   acc[PULSE_BJ_MCC_CELL_HIT(state, k, r < 0)] += 1   /   acc[PULSE_BJ_MCC_CELL_STAND(state, r < 0)] += 1,
 * acc: device int64[PULSE_BJ_MCC_ACC_LEN], added to.  Summed over the actions the cells are pulse_blackjack_mc_rollout's wherever no
 * state repeats within a game (cards 0..51).  The launch holds two workgroups per CU; where the device cannot, it is an error.
 *
 * pulse_blackjack_mc_improve: one lane per state, float64.  pow[0] = 1, pow[k] = gamma * pow[k - 1]; for each action n_a = the
 * sum of its cells, sum_a = the sum over ascending k of (double)(acc[.., k, 0] - acc[.., k, 1]) * pow[k] (stand: k = 0 only),
 * q_a = n_a ? sum_a / n_a : 0.0 (an unseen pair reads 0, as the reference's defaultdict).  A state with n_hit + n_stand = 0 keeps
 * its hit_prob.  Otherwise the greedy action is stand if q_stand > q_hit, hit if q_stand < q_hit, and on equality stand iff bit 0
 * of word 0 of Philox4x32-10(seed ^ PULSE_BJ_MCC_TIE_KEY, state, round) is set -- a third stream, keyed apart from the shuffle's
 * (the seed itself) and the policy's (seed ^ 0xB1AC7AC4D3A1E5) -- and hit_prob[state] = (float)(1 - epsilon + epsilon / 2) where
 * hit is greedy, (float)(epsilon / 2) where stand is: computed in double, rounded once.
 *   acc      : device int64[PULSE_BJ_MCC_ACC_LEN], 8-byte aligned, read only.
 *   q        : NULL, or device float64[PULSE_BJ_MC_STATES][2], (hit, stand), 8-byte aligned: written for every state.
 *   hit_prob : device fp32[PULSE_BJ_MC_STATES], 4-byte aligned, updated in place.
 * epsilon outside [0, 1], a gamma that is not finite and non-zero reserved fields are PULSE_EINVAL. */
#define PULSE_BJ_MCC_CELLS      34         /* hit x k 0..15 x sign, then stand x sign */
#define PULSE_BJ_MCC_CELL_HIT(state, k, negative) (((state) * PULSE_BJ_MCC_CELLS) + ((k) * 2) + (negative))
#define PULSE_BJ_MCC_CELL_STAND(state, negative) (((state) * PULSE_BJ_MCC_CELLS) + (PULSE_BJ_MC_MAX_ACTIONS * 2) + (negative))
#define PULSE_BJ_MCC_ACC_LEN    (PULSE_BJ_MC_STATES * PULSE_BJ_MCC_CELLS)
#define PULSE_BJ_MCC_TIE_KEY    0x7C01F11B5EEDull
typedef struct PulseBlackjackMCControl {
    int32_t n_games, n_episodes;
    uint64_t seed, episode;
    const float* hit_prob;
    const int32_t* decks_src;
    int64_t* acc;                       /* int64[PULSE_BJ_MCC_ACC_LEN] */
    int64_t* stats;
    int8_t* trace;
    int32_t max_blocks, reserved0;
} PulseBlackjackMCControl;
int pulse_blackjack_mc_control_rollout(const PulseBlackjackMCControl* o, void* stream);
typedef struct PulseBlackjackMCImprove {
    const int64_t* acc;
    double gamma, epsilon;
    uint64_t seed, round;
    double* q;
    float* hit_prob;
    int32_t reserved0, reserved1;
} PulseBlackjackMCImprove;
int pulse_blackjack_mc_improve(const PulseBlackjackMCImprove* o, void* stream);

/* ---- 2048 (environments/2048/TFE.py), batched: boards device int32[B,n,n], n = 2..8 ------------
 * 4 x 4 (config/tfe.yaml) with 16-byte aligned boards runs packed: the board as 64 bits of 4-bit log2 tiles, the move as four
 * lookups in a 65,536-entry row table the library builds on the device at the first call (256 KB of static device memory, one
 * synchronisation of the null stream, once per device); a board holding anything but 0 and the powers of two 2 .. 16,384 is
 * stepped cell by cell like the other sides -- any int32 board gives the reference's result. */
int pulse_tfe_reset(int32_t* boards, int64_t* total_score, int32_t n_boards, int32_t n, uint64_t seed,
                    uint64_t board_id0, void* stream);                                          /* :143-149 */
int pulse_tfe_step(int32_t* boards, int64_t* total_score, const int64_t* actions, int32_t* rewards,
                   uint8_t* dones, int32_t n_boards, int32_t n, uint64_t seed, uint64_t board_id0,
                   uint64_t step_counter, void* stream);                                        /* :152-189 */

/* ---- tabular Q-learning for the batched 2048 roll-out (utils/numba.py:5-39, agents/TemperalDifference/QLearningNumba.py:10-37)
 * The reference's `defaultdict(state -> float64[4])` is an open-addressing hash table of 64-byte ENTRIES in HBM:
 *   entry = { uint64 key (the board packed as 4-bit log2 tiles; 0 = free), double q[4], 24 spare bytes }
 * -- key and values of a state in ONE memory line.  entries: device memory, capacity * 64 bytes, 64-byte aligned,
 * zero-initialised by the caller; capacity and region_slots are powers of two.  region_slots > 0: board g owns entries
 * [g*region_slots, (g+1)*region_slots) (independent learners = copies of the reference agent, race-free, bit-exact);
 * 0: one table shared by all boards.  Shared table: an update whose single compare-and-swap loses against a concurrent
 * update of the same cell is deferred, and the deferred transitions of a launch are combined per cell --
 *   q <- q + (1 - (1 - alpha)^k) (mean of the k targets - q)   (k = 1: numba.py:38-39 itself)
 * -- with plain atomic adds into the per-launch scratch below (linear in the number of contenders; a CAS retry loop is
 * quadratic: all boards leave reset from a few hundred states). */
#define PULSE_QTABLE_ENTRY_BYTES 64
typedef struct PulseQTable {
    void* entries;
    uint64_t capacity, region_slots;
} PulseQTable;
/* Scratch of a shared table (NULL for private regions): caller-owned device memory, zero-initialised once.
 * count uint32[64 + 2 * n / 256]; cells uint64[n]; targets double[n]; owner int32[n]; acc_key uint64[acc_slots]; acc_cnt
 * uint32[acc_slots]; acc_sum double[acc_slots]; n >= n_boards, a multiple of 256 (the deferred list is kept in one segment
 * per workgroup of the launch; at most 1,048,576 boards per launch); acc_slots a power of two >= 2 n.  launch_index: the
 * caller counts its update / rollout_step launches on this scratch (0, 1, 2, ...: its parity picks the list).
 * A long list of deferred transitions is combined by 64 workgroups that meet inside the follow-up launch; if they cannot
 * gather within wait_ticks (a co-tenant on the GPU) the meeting is called off as a whole, that launch's combined updates
 * are dropped, and the next call on a shared table clears the accumulators and returns PULSE_EINTERNAL once. */
typedef struct PulseQTableScratch {
    uint32_t* count;
    uint64_t* cells;
    double* targets;
    int32_t* owner;
    uint64_t* acc_key;
    uint32_t* acc_cnt;
    double* acc_sum;
    uint32_t n, acc_slots;
    int64_t wait_ticks;             /* how long the follow-up launch's workgroups wait for each other (100 MHz ticks); 0 = 3 s */
    int32_t debug_meet_extra;       /* test hook: arrivals that meeting expects beyond the grid's own (> 0: it never comes about) */
    int32_t reserved0;
} PulseQTableScratch;
/* state lookup/insert + epsilon-greedy: actions int64[B] out, slots int64[B] out (-1 = no room: the region is full or
 * 4,096 consecutive slots were taken -- size a shared table for the states a run will visit; such a board acts at
 * random and is not updated) */
int pulse_qtable_select(const PulseQTable* q, const int32_t* boards, int32_t n_boards, int32_t n, double epsilon,
                        uint64_t seed, uint64_t board_id0, uint64_t step_counter, int64_t* actions, int64_t* slots,
                        void* stream);
/* q[s][a] += alpha * ((terminal ? r : r + gamma * max q[s']) - q[s][a]) for every board */
int pulse_qtable_update(const PulseQTable* q, const PulseQTableScratch* scratch, uint64_t launch_index, const int64_t* slots,
                        const int64_t* actions, const int32_t* rewards, const int32_t* next_boards, const uint8_t* terminal,
                        int32_t n_boards, int32_t n, double alpha, double gamma, void* stream);
/* One roll-out step of B learners in ONE launch: pulse_qtable_select + pulse_tfe_step + pulse_qtable_update with the board
 * in registers throughout (same draws, same results: the agent's stream (agent_seed, board, agent_step), the
 * environment's (env_seed, board, env_step >= 1)).  slots_io int64[B]: in = the entry of every board's current state if
 * the previous step found it, -2 = look it up; out = the entry of the state the move led to.  boards / total_score are
 * updated in place, actions / rewards / dones written as the three calls would. */
int pulse_qtable_rollout_step(const PulseQTable* q, const PulseQTableScratch* scratch, uint64_t launch_index, int32_t* boards,
                              int64_t* total_score, int32_t n_boards, int32_t n, double epsilon, double alpha, double gamma,
                              uint64_t agent_seed, uint64_t agent_step, uint64_t env_seed, uint64_t env_step, uint64_t board_id0,
                              int64_t* actions, int32_t* rewards, uint8_t* dones, int64_t* slots_io, void* stream);

/* ---- 2048: on-policy first-visit Monte-Carlo control on the device (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71 on the
 * games of scripts/TFE/mctrain.py): whole games against a table policy in one launch, the backward first-visit pass into
 * that table in a second one.  Stream-ordered: a round needs no host synchronisation.
 *
 * The table is an open-addressing hash table (linear probing) of 128-byte ENTRIES in HBM, 128-byte aligned, zeroed by the
 * caller, capacity a power of two:
 *   entry = { uint64 key (the board as 4-bit log2 tiles, pulse_qtable's key; 0 = free), int64 cnt[4], int64 sum[4], 56 spare bytes }
 * sum[a] = the fixed-point sum of the first-visit returns of (state, a), llrint(G * 2^frac_bits) each; cnt[a] = their number;
 *   q(s, a) = cnt[a] > 0 ? (double)sum[a] / (double)cnt[a] * 2^-frac_bits : 0.0   (the reference's defaultdict(float)).
 * Integer adds only: the table read as a map key -> {cnt, sum} does not depend on scheduling (the slots' positions do).
 * frac_bits: 0 .. the largest value <= 30 with G_max * 2^frac_bits * 2^32 < 2^62, G_max = 17 * min(max_steps, 1 / (1 - gamma))
 * (17 bounds the reward of a step for n <= 4): room for 2^32 adds per cell.  gamma .9: 22.
 *
 * pulse_tfe_mc_rollout: one lane per game, from reset to the terminal step or to max_steps moves.  The games are the
 * environment's own: reset and spawns draw from Philox4x32-10(env_seed, board_id0 + g, env_step), env_step 0 at reset and t + 1
 * at move t, as pulse_tfe_reset / pulse_tfe_step.  The table is only READ (a lookup never inserts; at most
 * PULSE_TFE_MC_MAX_PROBE slots are examined): the policy of a round is fixed.  The action at move t, from {x, y, ..} =
 * Philox4x32-10(agent_seed, board_id0 + g, t):
 *   no entry for the state, or (x >> 8) < floor(epsilon * 2^24)   ->   y >> 30;
 *   otherwise the greedy action of the entry: a = 0..3 in order, a larger q replaces the best, an equal q replaces it iff bit
 *   31 of word a - 1 of Philox4x32-10(tie_seed, key, round) is set (float64, IEEE division).
 * Output, step-major: keys[t * n_games + g] = the state before move t, steps[t * n_games + g] = action | reward << 2 | first << 7,
 * first = the action was not yet taken in the current run of identical boards (equal states of a game are consecutive: the
 * tile sum rises at every step that changes the board or spawns).  Rows t >= lengths[g] are not written.  Per game: lengths
 * (moves played), total_score (TFE.py:168), episode_reward (the sum of the rewards).  stats: device int64[8], added to:
 * [0] moves played, [3] games cut at max_steps (this call); [1] first visits added, [2] first visits dropped (learn).
 *
 * pulse_tfe_mc_learn: one lane per game, t = lengths[g] - 1 .. 0, G = gamma * G + reward in float64 (from 0 at the end, also of
 * a game that was cut); at a step with `first` set the entry is found or inserted (compare-and-swap on the key) and
 * sum[a] += llrint(ldexp(G, frac_bits)), cnt[a] += 1.  A state with no room (PULSE_TFE_MC_MAX_PROBE slots, or all of them, taken)
 * counts in stats[2] and is not learnt.
 *
 * PULSE_EINVAL, before anything is launched: n outside 2..4, epsilon or gamma outside [0, 1], a capacity that is no power of two,
 * entries not 128-byte aligned, a null or misaligned buffer, n_games < 1, max_steps outside 1..65,535, frac_bits outside its
 * bound, non-zero reserved fields. */
#define PULSE_TFE_MC_ENTRY_BYTES 128
#define PULSE_TFE_MC_MAX_PROBE   512
#define PULSE_TFE_MC_R_MAX       17
typedef struct PulseTfeMCRollout {
    void* entries;
    uint64_t capacity;
    int32_t n_games, n, max_steps, frac_bits;
    double gamma, epsilon;
    uint64_t env_seed, agent_seed, tie_seed, board_id0, round;
    uint64_t* keys;                     /* uint64[max_steps * n_games] */
    uint8_t* steps;                     /* uint8[max_steps * n_games] */
    int32_t* lengths;                   /* int32[n_games] */
    int64_t* total_score;               /* int64[n_games] */
    int32_t* episode_reward;            /* int32[n_games] */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
} PulseTfeMCRollout;
int pulse_tfe_mc_rollout(const PulseTfeMCRollout* o, void* stream);
typedef struct PulseTfeMCLearn {
    void* entries;
    uint64_t capacity;
    int32_t n_games, n, max_steps, frac_bits;
    double gamma, epsilon;
    const uint64_t* keys;
    const uint8_t* steps;
    const int32_t* lengths;
    int64_t* stats;
    int64_t reserved0;
} PulseTfeMCLearn;
int pulse_tfe_mc_learn(const PulseTfeMCLearn* o, void* stream);

/* ---- 2048 Monte-Carlo control: the eight symmetries of the square as one state, and an evaluation launch.
 *
 * T_0 .. T_7: T_j rotates the board j & 3 times by the environment's rotation (TFE.py:38-44: out[r][c] = in[c][n - 1 - r]), for
 * j >= 4 after a transpose.  canon(board) = (key_c, j*): key_c = the smallest of the eight images' keys as uint64, j* = the smallest
 * j whose image has it.  amap[j][a] = the action with T_j(move(B, a)) == move(T_j(B), amap[j][a]) and the same merge score:
 *   amap = {0,1,2,3}, {3,0,1,2}, {2,3,0,1}, {1,2,3,0}, {1,0,3,2}, {0,3,2,1}, {3,2,1,0}, {2,1,0,3}   (0 left, 1 up, 2 right, 3 down).
 *
 * pulse_tfe_mc_rollout_canon: pulse_tfe_mc_rollout (same struct, same checks, same game of the environment, same draws) on the
 * table of canonical states.  Per move key_c is looked up.  No entry, or the epsilon branch: the board moves by a = y >> 30 as
 * there, so on an empty table the two entry points play the same games.  Otherwise a_c = the greedy action of the entry with the
 * tie coins of Philox4x32-10(tie_seed, key_c, round), and the board moves by the a with amap[j*][a] = a_c.  Recorded:
 * keys[t * n_games + g] = key_c, steps = a_c | reward << 2 | first << 7 with a_c = amap[j*][a], first = a_c was not yet taken in
 * the current run of equal key_c (equal key_c: equal tile sums: the same run of one unchanged board: the same j*).
 * pulse_tfe_mc_learn takes these as it takes the plain ones.
 *
 * pulse_tfe_mc_evaluate: the games pulse_tfe_mc_rollout (canonical = 0) or pulse_tfe_mc_rollout_canon (canonical = 1) plays for
 * equal env_seed, agent_seed, tie_seed, board_id0, round, epsilon and table, without a trajectory.  The table is only read.
 * summary, device int64[8], ADDED TO: [0] games, [1] moves, [2] sum of total_score, [3] sum of total_score^2, [4] the largest
 * total_score (atomic max), [5] games cut at max_steps, [6] moves whose state had an entry, [7] moves decided greedily (an entry
 * and not the epsilon branch).  max_tile_hist, device int64[16], added to: bin = log2 of the largest tile of the final board.
 * total_score int64[n_games] / lengths int32[n_games]: per game, or NULL.  One launch: the counters are reduced in the workgroup
 * and added with one atomic per workgroup and non-zero bin.  frac_bits: the table's, 0..30 (the scale of q does not change an
 * order).  PULSE_EINVAL as above, and for canonical outside {0, 1}, a null summary or max_tile_hist, non-zero reserved fields. */
int pulse_tfe_mc_rollout_canon(const PulseTfeMCRollout* o, void* stream);
typedef struct PulseTfeMCEval {
    const void* entries;
    uint64_t capacity;
    int32_t n_games, n, max_steps, frac_bits;
    double epsilon;
    uint64_t env_seed, agent_seed, tie_seed, board_id0, round;
    int32_t canonical, reserved0;
    int64_t* summary;                   /* int64[8] */
    int64_t* max_tile_hist;             /* int64[16] */
    int64_t* total_score;               /* int64[n_games] or NULL */
    int32_t* lengths;                   /* int32[n_games] or NULL */
    int64_t reserved1;
} PulseTfeMCEval;
int pulse_tfe_mc_evaluate(const PulseTfeMCEval* o, void* stream);

/* ---- 2048 Monte-Carlo table: dst += src over entries, one launch.  Growing a table (src = the old table, dst = a larger zeroed
 * one), folding a plain table into a symmetric one (canonical = 1), adding the tables of two agents and loading a checkpoint
 * (src = a dense array of entries) are all this call.
 *
 * src: src_entries entries of PULSE_TFE_MC_ENTRY_BYTES in the table's layout, 128-byte aligned.  It is only SCANNED, one lane per
 * slot, never probed: a hash table with holes or a dense array of ANY length >= 1; an entry with key 0 is skipped.  dst: a
 * pulse_tfe_mc table (capacity a power of two, caller-owned).  Per live source entry: with canonical = 1 the key's n * n nibbles are
 * unpacked, (key_c, j*) = canon of that board, and the eight values go to cnt[amap[j*][a]] / sum[amap[j*][a]]; with canonical = 0 key and
 * values go as they are.  The key is found or inserted in dst by the learner's bounded probe (at most PULSE_TFE_MC_MAX_PROBE slots)
 * and cnt[a], sum[a] are added there with 64-bit integer atomics for every action whose cnt | sum is non-zero.  Integer adds: dst read
 * as a map key -> {cnt, sum} does not depend on scheduling.  An entry with no room adds NOTHING of itself and counts in stats[2].
 * stats, device int64[4], ADDED TO: [0] live source entries, [1] entries placed, [2] entries dropped, [3] not written.  One
 * launch, counters reduced per workgroup, no wait between workgroups, no loop whose end depends on table content.
 *
 * Limits.  (1) dst is NOT zeroed by the call: a new table is the caller's to zero.  (2) The room the fixed-point rule leaves -- 2^32
 * adds per cell -- now covers the SUM of the merged tables' counts per cell.  (3) frac_bits, gamma and the board side of the two
 * tables must agree; the kernel cannot see that (the Python layer refuses).  (4) With canonical = 1 only the low n * n nibbles of
 * a source key are read: a key with bits above them is folded as the state of its low nibbles, and nothing counts that.
 * PULSE_EINVAL, before anything is launched: src or dst null or not 128-byte aligned, src_entries < 1 (or 2^32 and more: one lane
 * per slot in one launch), dst_capacity no power of two, overlapping byte ranges, canonical outside {0, 1}, n outside 2..4 (also when it is not
 * used), stats null or not 8-byte aligned, non-zero reserved0. */
typedef struct PulseTfeMCMerge {
    const void* src;
    uint64_t src_entries;
    void* dst;
    uint64_t dst_capacity;
    int32_t n, canonical;
    int64_t* stats;                     /* int64[4] */
    int64_t reserved0;
} PulseTfeMCMerge;
int pulse_tfe_mc_table_merge(const PulseTfeMCMerge* o, void* stream);

/* ---- 2048 Monte-Carlo control on AFTERSTATES: the table holds V(board after the move, before the spawn), not Q(state, action).
 * Five entry points on the structs above, with the checks of their namesakes (messages carry the new names); the plain ones are
 * unchanged.
 *
 * The table is the same table.  The key is the afterstate's key; cnt[0] / sum[0] hold the count and the fixed-point sum of the returns
 * that FOLLOWED the afterstate, cnt[1..3] and sum[1..3] stay 0:
 *   v(key) = cnt[0] > 0 ? (double)sum[0] / (double)cnt[0] * 2^-frac_bits : 0.0.
 * frac_bits obeys the same bound (the stored return is bounded by the same G_max).  pulse_tfe_mc_table_merge with canonical = 0
 * (grow, add, load) works on such a table as it is; with canonical = 1 it would permute the slots, so the fold is a call of its own.
 *
 * pulse_tfe_mc_rollout_after / pulse_tfe_mc_rollout_after_canon: the games of pulse_tfe_mc_rollout (same reset, spawns and agent
 * draws {x, y, ..} = Philox4x32-10(agent_seed, board_id0 + g, t)).  At move t on board B, for a = 0..3: (B_a, score_a) = the move of B
 * by a without a spawn, r_a = the environment's reward of score_a (bit length - 1, 0 for 0), key_a = the key of B_a (_canon: the
 * smallest key of its eight images; a value has no action, so nothing is mapped), v_a = v(entry of key_a) by a read-only lookup of at
 * most PULSE_TFE_MC_MAX_PROBE slots, 0.0 without an entry, q_a = r_a + gamma * v_a in float64 (one rounding per operation, IEEE
 * division).  A move that changes nothing is a candidate like any other: the environment accepts it and spawns after it.
 *   none of the four keys has an entry, or (x >> 8) < floor(epsilon * 2^24)   ->   a = y >> 30;
 *   otherwise a = 0..3 in order, a larger q replaces the best, an equal q replaces it iff bit 31 of word a - 1 of
 *   Philox4x32-10(tie_seed, key of B, round) is set -- the plain key of the state before the move, in both forms.
 * Recorded: keys[t * n_games + g] = key_a of the action taken, steps = a | r_a << 2 | first << 7 with a the BOARD's action (a replay
 * through pulse_tfe_step works in both forms), first = key_a differs from the key recorded at t - 1 (1 at t = 0).  Equal
 * afterstates of a game are consecutive: a move keeps the tile sum and the sum rises from one distinct state to the next, so equal
 * afterstates come from one run of an unchanged full board, where every unchanged move has the board itself as its afterstate and
 * the move that ends the run merges tiles -- its afterstate has an empty cell.  lengths, total_score, episode_reward and stats as
 * pulse_tfe_mc_rollout.
 *
 * pulse_tfe_mc_learn_after: t = lengths[g] - 1 .. 0; at a step with `first` set the key is found or inserted and
 * sum[0] += llrint(ldexp(G, frac_bits)), cnt[0] += 1 with G as it stands; THEN G = gamma * G + reward.  So an afterstate collects the
 * return that follows it, and r_a + gamma * v_a above is the reference's G_t.  Counters as pulse_tfe_mc_learn.
 *
 * pulse_tfe_mc_evaluate_after: the games of the two roll-outs above (by `canonical`) without a trajectory; summary and histogram as
 * pulse_tfe_mc_evaluate, summary[6] = moves where at least one of the four keys had an entry.  gamma: the policy's (PulseTfeMCEval
 * holds none); PULSE_EINVAL outside [0, 1].
 *
 * pulse_tfe_mc_table_fold_after: pulse_tfe_mc_table_merge's checks and launch for the fold of a value table -- every key goes to its
 * canonical key, cnt[a] / sum[a] go to slot a as they are.  canonical must be 1. */
int pulse_tfe_mc_rollout_after(const PulseTfeMCRollout* o, void* stream);
int pulse_tfe_mc_rollout_after_canon(const PulseTfeMCRollout* o, void* stream);
int pulse_tfe_mc_learn_after(const PulseTfeMCLearn* o, void* stream);
int pulse_tfe_mc_evaluate_after(const PulseTfeMCEval* o, double gamma, void* stream);
int pulse_tfe_mc_table_fold_after(const PulseTfeMCMerge* o, void* stream);

/* ---- 2048 on 4 x 4: an n-tuple network trained by batch TD(0) on afterstates.  Four launches, stream-ordered, no host
 * synchronisation between them: whole games under the network, the temporal differences of every recorded move into integer
 * accumulators, the accumulators into the weights, and an evaluation.  n = 4 only; the board is the packed 64-bit key for the whole game.
 *
 * The network (PulseTfeNtNet, the first member of the four structs).  n_tuples = 1..8 tuples; tuple t is tuple_len[t] = 1..6 distinct
 * cells (0..15, row-major) in cells[t][0 .. len - 1] (the other bytes of cells[t] are not read) with its own table of 16^len weights:
 *   float weights[n_weights], n_weights = the sum of 16^len over the tuples, tuple t's table at the sum of the earlier tables' sizes;
 *   4-byte aligned, caller-owned, zeroed = the empty network.
 * The index of a tuple on a board = the sum over i of nibble(cell_i) << 4 i, the nibble being the key's (log2 of the tile, 0 = empty).
 * symmetric = 1: every tuple is read on the eight images T_0 .. T_7 of the board (the eight symmetries above) -- image j reads the
 * cells T_j shows at the tuple's positions -- and all eight read the tuple's one table; F = 8 n_tuples features (n_tuples with
 * symmetric = 0, where only T_0, the board as it lies, is read).  The library derives the images' cells from T_j; the caller passes
 * the tuples only.
 *   V(board) = the sum over the features of (double)weights[index], in float64, tuple-major and image j = 0..7 within a tuple, from
 *   0.0, one rounding per add.
 * Accumulators: int64 acc[n_weights][2] = {sum, cnt}, 16-byte aligned, caller-owned, zeroed once by the caller (the apply launch
 * zeroes what it reads).  sum holds temporal differences as llrint(delta * 2^PULSE_TFE_NT_FRAC_BITS), |delta| clamped to
 * PULSE_TFE_NT_DELTA_MAX: 8192 * 2^16 * 2^32 < 2^62, room for 2^32 adds per cell (the bound of the Monte-Carlo table's frac_bits).
 * stats, device int64[8], ADDED TO: [0] moves played, [3] games cut (roll-out); [1] moves learnt, [2] moves skipped, [4] temporal
 * differences clamped (learn); [5..7] not written.
 *
 * pulse_tfe_nt_rollout: one lane per game, from reset to the terminal step or to max_steps moves; the environment's own games,
 * exactly as pulse_tfe_mc_rollout draws them (Philox4x32-10(env_seed, board_id0 + g, env_step), env_step 0 at reset and t + 1 at move
 * t; the agent's draw {x, y, ..} = Philox4x32-10(agent_seed, board_id0 + g, t)).  The weights are only read.  At move t on board B,
 * for a = 0..3: (B_a, score_a) = the move of B by a without a spawn, r_a = the environment's reward (bit length of score_a - 1, 0 for
 * 0), q_a = r_a + gamma * V(B_a) in float64, one rounding per operation.  The CANDIDATES are the moves with B_a != B (a board that is
 * not over has one) -- unlike pulse_tfe_mc_rollout_after: a move that changes nothing on a full board has a temporal difference of 0
 * at gamma = 1, which TD would never unlearn.
 *   (x >> 8) < floor(epsilon * 2^24)   ->   a = y >> 30 (uniform over the four; the environment accepts a move that changes nothing);
 *   otherwise the candidates in the order a = 0..3: the first is the best so far, a larger q replaces it, an equal q replaces it iff
 *   bit 31 of word a - 1 of Philox4x32-10(tie_seed, key of B, round) is set.  On zero weights: greedy on the reward.
 * Recorded, step-major: keys[t * n_games + g] = the key of the afterstate B_a taken, values[...] = V(B_a) as float64,
 * steps[...] = a | r_a << 2 | terminal << 7, terminal = the game was over after this move's spawn.  Rows t >= lengths[g] are not
 * written.  Per game: lengths, total_score, episode_reward.  A game whose board comes to hold nibble 15 (a 32,768 tile: the row
 * table cannot merge two of them) stops there; a game that stopped without being over -- at max_steps or at that tile -- is CUT.
 *
 * pulse_tfe_nt_learn: one lane per recorded move (t, g), t < lengths[g]; no weight is read.  The last move of a game has target 0
 * if its terminal bit is set and is SKIPPED otherwise (a cut game's last afterstate has no known successor); any other move has
 * target = reward(steps[t + 1]) + gamma * values[t + 1].  delta = target - values[t], clamped to +-PULSE_TFE_NT_DELTA_MAX (counted),
 * d = llrint(ldexp(delta, PULSE_TFE_NT_FRAC_BITS)); for every feature of keys[t]: acc[index].sum += d, acc[index].cnt += 1 (64-bit
 * integer atomics without a returned value; two images that land on one weight add twice).  Integer adds: acc does not depend on
 * scheduling.
 *
 * pulse_tfe_nt_apply: one lane per weight; where cnt > 0,
 *   weights[i] = (float)((double)weights[i] + step * (((double)sum / (double)cnt) * 2^-16))   (one rounding per operation, IEEE
 *   division), and both accumulator words become 0.  A weight with cnt = 0 keeps its bits.  step = alpha / F: each weight moves
 *   by alpha / F of the MEAN temporal difference of its visits in the round, whatever the number of games.
 *
 * pulse_tfe_nt_evaluate: the roll-out's games for equal seeds, ids, round, gamma, epsilon and weights, without a trajectory.
 * summary, device int64[8], ADDED TO: [0] games, [1] moves, [2] sum of total_score, [3] sum of total_score^2, [4] the largest
 * total_score (atomic max), [5] games cut, [6] moves decided greedily (not the epsilon branch), [7] games stopped at the 32,768 tile
 * (counted in [5] too unless the game was over as well).  max_tile_hist, device int64[16], added to: bin = the largest nibble of
 * the final board.  total_score int64[n_games] / lengths int32[n_games]: per game, or NULL.  Reduced in the workgroup: one atomic per
 * workgroup and non-zero bin.
 *
 * PULSE_EINVAL, before anything is launched: n != 4, n_tuples outside 1..8, a length outside 1..6, a cell above 15 or repeated within
 * a tuple, n_weights != the sum of 16^len, symmetric outside {0, 1}, gamma or epsilon outside [0, 1], step outside (0, 1], max_steps
 * outside 1..65,535, n_games < 1, a null or misaligned buffer the call needs (learn needs no weights), non-zero reserved fields. */
#define PULSE_TFE_NT_MAX_TUPLES 8
#define PULSE_TFE_NT_MAX_LEN    6
#define PULSE_TFE_NT_FRAC_BITS  16
#define PULSE_TFE_NT_DELTA_MAX  8192.0
typedef struct PulseTfeNtNet {
    int32_t n, n_tuples, symmetric, reserved0;
    uint8_t tuple_len[PULSE_TFE_NT_MAX_TUPLES];
    uint8_t cells[PULSE_TFE_NT_MAX_TUPLES][8];
    uint64_t n_weights;
    float* weights;                     /* float[n_weights] */
} PulseTfeNtNet;
typedef struct PulseTfeNtRollout {
    PulseTfeNtNet net;
    int32_t n_games, max_steps;
    double gamma, epsilon;
    uint64_t env_seed, agent_seed, tie_seed, board_id0, round;
    uint64_t* keys;                     /* uint64[max_steps * n_games] */
    double* values;                     /* float64[max_steps * n_games] */
    uint8_t* steps;                     /* uint8[max_steps * n_games] */
    int32_t* lengths;                   /* int32[n_games] */
    int64_t* total_score;               /* int64[n_games] */
    int32_t* episode_reward;            /* int32[n_games] */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
} PulseTfeNtRollout;
int pulse_tfe_nt_rollout(const PulseTfeNtRollout* o, void* stream);
typedef struct PulseTfeNtLearn {
    PulseTfeNtNet net;                  /* weights may be NULL */
    int32_t n_games, max_steps;
    double gamma;
    const uint64_t* keys;
    const double* values;
    const uint8_t* steps;
    const int32_t* lengths;
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
} PulseTfeNtLearn;
int pulse_tfe_nt_learn(const PulseTfeNtLearn* o, void* stream);
typedef struct PulseTfeNtApply {
    PulseTfeNtNet net;
    double step;                        /* alpha / F */
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t reserved0;
} PulseTfeNtApply;
int pulse_tfe_nt_apply(const PulseTfeNtApply* o, void* stream);
typedef struct PulseTfeNtEval {
    PulseTfeNtNet net;
    int32_t n_games, max_steps;
    double gamma, epsilon;
    uint64_t env_seed, agent_seed, tie_seed, board_id0, round;
    int64_t* summary;                   /* int64[8] */
    int64_t* max_tile_hist;             /* int64[16] */
    int64_t* total_score;               /* int64[n_games] or NULL */
    int32_t* lengths;                   /* int32[n_games] or NULL */
    int64_t reserved0;
} PulseTfeNtEval;
int pulse_tfe_nt_evaluate(const PulseTfeNtEval* o, void* stream);

/* ---- the n-tuple network's TD(lambda) learner: pulse_tfe_nt_learn with lambda-differences in place of one-step differences, on the
 * same recorded games and into the same accumulators; pulse_tfe_nt_apply follows as it does there.  Everything is float64, one
 * rounding per operation.  For game g let L = min(lengths[g], max_steps), moves t = 0 .. L - 1.
 *   delta_t  = pulse_tfe_nt_learn's one-step difference, unclamped: 0 - V_t at the last move with its terminal bit,
 *              (r_{t+1} + gamma * V_{t+1}) - V_t at any other; the last move without its terminal bit is SKIPPED as it is there
 *              (it adds nothing, is counted in stats[2]) and its lambda-difference is +0.0;
 *   gl       = gamma * lambda, one multiply, formed once;
 *   D_{L-1}  = delta_{L-1}, or +0.0 if that move is skipped;   D_t = delta_t + gl * D_{t+1}, one multiply and one add.
 * The recurrence carries the UNCLAMPED D.  Where a move is added, D_t is clamped to +-PULSE_TFE_NT_DELTA_MAX (counted in stats[4]),
 * d = llrint(ldexp(D_t, PULSE_TFE_NT_FRAC_BITS)), and for every feature of keys[t]: acc[index].sum += d, acc[index].cnt += 1, the
 * adds and the counters stats[1], [2], [4] of pulse_tfe_nt_learn.  At lambda = 0 acc is pulse_tfe_nt_learn's.
 * Two launches on the stream: one lane per game walks t downwards and writes deltas[t * n_games + g] = D_t for t < L (rows at and
 * beyond L are not written); one lane per recorded move then adds.  deltas: device float64[max_steps * n_games], step-major like
 * values, caller-owned scratch that holds the round's D afterwards.
 *
 * PULSE_EINVAL, before anything is launched: pulse_tfe_nt_learn's refusals; lambda outside [0, 1] (NaN included); deltas null or not
 * 8-byte aligned. */
typedef struct PulseTfeNtLearnLambda {
    PulseTfeNtNet net;                  /* weights may be NULL */
    int32_t n_games, max_steps;
    double gamma, lambda;
    const uint64_t* keys;
    const double* values;
    const uint8_t* steps;
    const int32_t* lengths;
    double* deltas;                     /* float64[max_steps * n_games] */
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
} PulseTfeNtLearnLambda;
int pulse_tfe_nt_learn_lambda(const PulseTfeNtLearnLambda* o, void* stream);

/* ---- the n-tuple network's temporal-coherence (TC) step sizes: every weight moves by step * rho, rho = |E| / A, from the running sums
 * of its rounds' mean errors (E) and mean absolute errors (A).  A weight whose errors keep their sign keeps the full step; one whose
 * errors cancel stops moving.  Opt-in: a caller that never calls these two keeps the launches above unchanged.  Everything is
 * float64, one rounding per operation.
 * State per weight, caller-owned, zeroed once by the caller: double e[n_weights], double a[n_weights], 8-byte aligned.
 * A third accumulator beside acc: int64 acc_abs[n_weights], 8-byte aligned, zeroed once by the caller (the apply launch zeroes what
 * it reads).
 *
 * pulse_tfe_nt_learn_tc: pulse_tfe_nt_learn's adds (deltas NULL; needs lambda == 0) or pulse_tfe_nt_learn_lambda's walk and adds (deltas
 * set, any lambda in [0, 1]), with the same skip rule, clamp and counters stats[1], [2], [4]; wherever those add sum += d, cnt += 1
 * this also adds acc_abs[index] += |d|, d the clamped fixed-point integer read as signed.  acc is what the other two learners leave.
 *
 * pulse_tfe_nt_apply_tc: one lane per weight; where cnt > 0,
 *   m   = ((double)sum / (double)cnt) * 2^-16            (pulse_tfe_nt_apply's mean)
 *   ab  = ((double)abs / (double)cnt) * 2^-16
 *   rho = a[i] > 0 ? |e[i]| / a[i] : 1.0                 (from e and a BEFORE this round's m and ab are added)
 *   weights[i] = (float)((double)weights[i] + (step * rho) * m)      (step * rho is formed first)
 *   e[i] = e[i] + m;  a[i] = a[i] + ab;  sum, cnt and abs become 0.
 * A weight with cnt = 0 keeps its bits, and so do its e and a.  On zeroed e and a (the first apply) rho is 1.0 exactly and the
 * weights are pulse_tfe_nt_apply's, bit for bit.
 * tc_stats, device int64[4], 8-byte aligned, ADDED TO: [0] weights moved, [1] the sum over them of llrint(rho * 2^32) (the mean rho
 * of a round = [1] / [0] * 2^-32); [2], [3] not written.  Summed per workgroup, then one atomic per workgroup and word; integer
 * adds, so tc_stats does not depend on scheduling.
 *
 * PULSE_EINVAL, before anything is launched: pulse_tfe_nt_learn_lambda's refusals, except that deltas may be NULL at lambda == 0;
 * lambda > 0 with deltas NULL; acc_abs null or not 8-byte aligned; for the apply pulse_tfe_nt_apply's, and acc_abs, e, a or tc_stats
 * null or not 8-byte aligned. */
typedef struct PulseTfeNtLearnTc {
    PulseTfeNtNet net;                  /* weights may be NULL */
    int32_t n_games, max_steps;
    double gamma, lambda;
    const uint64_t* keys;
    const double* values;
    const uint8_t* steps;
    const int32_t* lengths;
    double* deltas;                     /* float64[max_steps * n_games], or NULL at lambda == 0 */
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t* acc_abs;                   /* int64[n_weights] */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
} PulseTfeNtLearnTc;
int pulse_tfe_nt_learn_tc(const PulseTfeNtLearnTc* o, void* stream);
typedef struct PulseTfeNtApplyTc {
    PulseTfeNtNet net;
    double step;                        /* alpha / F */
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t* acc_abs;                   /* int64[n_weights] */
    double* e;                          /* float64[n_weights] */
    double* a;                          /* float64[n_weights] */
    int64_t* tc_stats;                  /* int64[4] */
    int64_t reserved0;
} PulseTfeNtApplyTc;
int pulse_tfe_nt_apply_tc(const PulseTfeNtApplyTc* o, void* stream);

/* ---- the n-tuple network under expectimax search, one chance layer deep: the same network asked about the boards AFTER the random
 * tile.  Everything is float64, one rounding per operation.  For a board B and a = 0..3, (B_a, score_a), r_a, V and "candidate"
 * (B_a != B) are pulse_tfe_nt_rollout's.  For a candidate a the CHANCE BOARDS of B_a are C(c, k) = B_a with nibble k at the empty cell
 * c, k = 1 (a 2-tile) or 2 (a 4-tile), in slot s = 2 c + (k - 1), s = 0..31.  The tile odds are the environment's own:
 * P_1 = 15099495 * 2^-24 and P_2 = 1677721 * 2^-24 (exact doubles); the cell is uniform over the n_empty(B_a) empty cells.
 *   m(C)   = the maximum over the candidates a' of C of r_a' + gamma * V(C_a'), 0.0 where C has none (the game is over there); a chance
 *            board is valued like any board (the 32,768-tile cut is a rule of real games only);
 *   term_s = P_k * m(C(c, k)), +0.0 at a slot whose cell is filled;
 *   S      = the pairwise tree over the 32 terms in slot order: level 0 adds slots s and s ^ 1, level 1 s and s ^ 2, .. up to 16;
 *   E_a    = S / n_empty(B_a),  q_a = r_a + gamma * E_a;  q_a = +0.0 for a move that is no candidate.
 * The action: pulse_tfe_nt_rollout's rule on these q -- the epsilon branch, the scan over the candidates in the order a = 0..3, the
 * tie coins Philox4x32-10(tie_seed, key of B, round).  At gamma = 0 this is the one-ply policy.  32 lanes play one board.
 * (A row of four nibbles 15 has a merge score the row table cannot hold, as in the roll-out: q of a board whose move or chance board
 * squashes such a row is not defined.)
 *
 * pulse_tfe_nt_search: for boards[g], g < n_boards (any packed boards, device uint64): q[g][0..3], action[g] = the greedy action
 * (-1: no candidate: the board is over), candidates[g] = bit a set where B_a != B.  The weights are only read.
 *
 * pulse_tfe_nt_evaluate_search: pulse_tfe_nt_evaluate's games, streams, counters and per-game arrays under the search policy.
 *
 * PULSE_EINVAL, before anything is launched: the network's checks; n_boards < 1; gamma outside [0, 1]; a null buffer; boards or q not
 * 8-byte aligned; non-zero reserved fields; pulse_tfe_nt_evaluate's own for pulse_tfe_nt_evaluate_search. */
typedef struct PulseTfeNtSearch {
    PulseTfeNtNet net;
    int32_t n_boards, reserved0;
    double gamma;
    uint64_t tie_seed, round;
    const uint64_t* boards;             /* uint64[n_boards] */
    double* q;                          /* float64[n_boards][4] */
    int8_t* action;                     /* int8[n_boards] */
    uint8_t* candidates;                /* uint8[n_boards] */
    int64_t reserved1;
} PulseTfeNtSearch;
int pulse_tfe_nt_search(const PulseTfeNtSearch* o, void* stream);
int pulse_tfe_nt_evaluate_search(const PulseTfeNtEval* o, void* stream);

/* ---- ... two chance layers deep.  The two structs above, with the depth beside them: `layers` = 1 is exactly the two entry points
 * above (the same kernels); `layers` = 2 replaces m(C) by W2(C), the best q of the one-layer search of C:
 *   W2(C)  = the best of q_a'(C) over the candidates a' of C, q(C) being the four q of the definition above on board C (its own
 *            chance boards, terms, tree and division); scanned a' = 0..3, the first candidate starts and a strictly larger q
 *            replaces it; +0.0 where C has no candidate.  No tie coins are drawn inside the tree;
 *   term_s = P_k * W2(C(c, k)), +0.0 at a slot whose cell is filled; S, E_a, q_a and the action as above.
 * One board or game per workgroup of 256 lanes: the live (move, slot) children are dealt to its 8 groups of 32 lanes, each of which
 * searches its child as the one-layer kernels search a board; the terms meet in LDS and are summed in the order above.
 *
 * PULSE_EINVAL, before anything is launched: what pulse_tfe_nt_search / pulse_tfe_nt_evaluate_search refuse, under these names;
 * `layers` other than 1 or 2 ("layers must be 1 or 2"). */
int pulse_tfe_nt_search_deep(const PulseTfeNtSearch* o, int32_t layers, void* stream);
int pulse_tfe_nt_evaluate_search_deep(const PulseTfeNtEval* o, int32_t layers, void* stream);

/* ---- ... at a depth the board chooses, per move.  The two structs above, with the threshold beside them: `deep_empty_max` = E in
 * 0..16.  For a board B to decide, n = the number of empty cells of B, the board the move is made from (not its afterstates):
 *   n <= E:    q(B) is the four q of the two-layer search (pulse_tfe_nt_search_deep at layers = 2);
 *   otherwise: q(B) is the four q of the one-layer search (pulse_tfe_nt_search), bit for bit.
 * Nothing else changes: the candidates, the greedy scan with its tie coins Philox(tie_seed, key of B, round), the epsilon branch,
 * the 32,768 cut, the counters.  E = 16 is the two-layer search on every board; E = 0 searches two layers on full boards only.
 * One board or game per workgroup of 256 lanes; n is the same in every lane that plays the board, so the choice is the workgroup's.
 * On a shallow move groups 0..3 of 32 lanes search one candidate move each and the four q meet in LDS.
 *
 * depth_stats: device int64[2], or NULL: [0] += the moves whose q came from two layers, [1] += those from one layer; every move of
 * every game counts, the epsilon branch's too (q is formed before the branch); added once per game, at its end.
 *
 * PULSE_EINVAL, before anything is launched: what pulse_tfe_nt_search_deep / pulse_tfe_nt_evaluate_search_deep refuse of their
 * structs, under these names; `deep_empty_max` outside 0..16 ("deep_empty_max must be in 0..16"); depth_stats not 8-byte aligned. */
int pulse_tfe_nt_search_adaptive(const PulseTfeNtSearch* o, int32_t deep_empty_max, void* stream);
int pulse_tfe_nt_evaluate_search_adaptive(const PulseTfeNtEval* o, int32_t deep_empty_max, int64_t* depth_stats, void* stream);

/* ---- ... and in the training roll-out: pulse_tfe_nt_rollout's games under the search policy.  The roll-out's struct, with the depth
 * beside it.  Everything is pulse_tfe_nt_rollout's -- the boards board_id0 + g, the three Philox streams, the epsilon branch and its
 * uniform action, the cap at a 32,768 tile, max_steps, the counters stats[0] (moves) and stats[3] (games cut), the per-game arrays
 * and the rows at and beyond a game's length, which are not written -- except the q the greedy scan reads: those of the definitions
 * above at `layers` chance layers, on the same tie coins (tie_seed, the board's key, round).  What a move records is unchanged too:
 *   keys[t, g]   = the chosen afterstate B_a;
 *   values[t, g] = V(B_a) of the NETWORK (tuple-major, image-minor, one rounding per add), not the search's q_a or E_a;
 *   steps[t, g]  = the action, the reward and the game-over bit.
 * So pulse_tfe_nt_learn, pulse_tfe_nt_learn_lambda and pulse_tfe_nt_learn_tc read the records as they read pulse_tfe_nt_rollout's: the
 * target of a move is the reward and V of the next move the search chose.  At gamma = 0 the records are pulse_tfe_nt_rollout's.
 * One game per group of 32 lanes at layers = 1 and per workgroup of 256 at layers = 2, as the evaluations above play theirs.
 *
 * PULSE_EINVAL, before anything is launched: what pulse_tfe_nt_rollout refuses, under this name; `layers` other than 1 or 2
 * ("layers must be 1 or 2"). */
int pulse_tfe_nt_rollout_search(const PulseTfeNtRollout* o, int32_t layers, void* stream);

/* ---- ... and learning towards the value the search backed up.  Opt-in: a caller that never calls these two keeps every launch above
 * unchanged.  Everything is float64, one rounding per operation.
 *
 * pulse_tfe_nt_rollout_backed: pulse_tfe_nt_rollout_search's games and records, word for word, and one more word per move.  Let
 * q[0..3] be the search's q of the board before move t (the definitions above at `layers`):
 *   backed[t, g] = the largest q[a] over the candidate moves (B_a != B), scanned a = 0..3: the first candidate starts, a strictly
 *                  larger q replaces it.  A maximum: no tie coin enters.  It is formed on every move, the epsilon branch included,
 *                  and does not depend on the action taken; at epsilon = 0 it is the q of the action taken.
 * backed: device float64[max_steps * n_games], step-major like values; rows at and beyond a game's length are not written.
 *
 * pulse_tfe_nt_learn_backed: pulse_tfe_nt_learn_lambda with another one-step difference.  V_t = values[t, g] estimates the value of
 * the board after the next spawn; backed[t + 1] is the search's estimate for the spawn that happened, r_{t+1} and its gamma inside.
 * For game g let L = min(lengths[g], max_steps):
 *   delta_{L-1} = 0 - V_{L-1} at the last move with its terminal bit; the last move without it is SKIPPED as in pulse_tfe_nt_learn
 *                 (counted in stats[2]; its difference is +0.0);
 *   delta_t     = backed[t + 1] - V_t at any other move, one subtract;
 *   gl = gamma * lambda, formed once;  D_{L-1} = delta_{L-1};  D_t = delta_t + gl * D_{t+1}, the UNCLAMPED D carried; the same
 *   recurrence at lambda = 0: one path.
 * The adds are pulse_tfe_nt_learn_lambda's: D_t clamped to +-PULSE_TFE_NT_DELTA_MAX (stats[4]), d = llrint(ldexp(D_t, 16)),
 * sum += d and cnt += 1 at every feature of keys[t]; with acc_abs set also acc_abs += |d| (pulse_tfe_nt_learn_tc's third
 * accumulator), with acc_abs NULL the plain accumulators.  pulse_tfe_nt_apply or pulse_tfe_nt_apply_tc follows, unchanged.  Two
 * launches on the stream: one lane per game walks t downwards and writes deltas[t * n_games + g] = D_t for t < L, reading 25 bytes
 * per move (backed[t + 1], V_t, the step byte); one lane per recorded move then adds.
 * The struct is PulseTfeNtLearnTc's fields in order, followed by `backed`.  Zero-initialise it: reserved0 must be 0.
 *
 * PULSE_EINVAL, before anything is launched: for the recording what pulse_tfe_nt_rollout refuses, under this name, `layers` other
 * than 1 or 2, backed null or not 8-byte aligned; for the learner pulse_tfe_nt_learn's refusals, lambda outside [0, 1] (NaN
 * included), deltas or backed null, keys / values / deltas / stats / backed / acc_abs not 8-byte aligned. */
int pulse_tfe_nt_rollout_backed(const PulseTfeNtRollout* o, int32_t layers, double* backed, void* stream);
typedef struct PulseTfeNtLearnBacked {
    PulseTfeNtNet net;                  /* weights may be NULL */
    int32_t n_games, max_steps;
    double gamma, lambda;
    const uint64_t* keys;
    const double* values;
    const uint8_t* steps;
    const int32_t* lengths;
    double* deltas;                     /* float64[max_steps * n_games] */
    int64_t* acc;                       /* int64[n_weights][2] */
    int64_t* acc_abs;                   /* int64[n_weights], or NULL: the plain accumulators */
    int64_t* stats;                     /* int64[8] */
    int64_t reserved0;
    const double* backed;               /* float64[max_steps * n_games] */
} PulseTfeNtLearnBacked;
int pulse_tfe_nt_learn_backed(const PulseTfeNtLearnBacked* o, void* stream);

/* ---- ... and rounds whose games start half-way through the games of the round before (the "restart" strategy of the n-tuple 2048
 * literature).  Opt-in: a caller that never calls these two keeps every launch above unchanged.
 *
 * pulse_tfe_nt_rollout_from: pulse_tfe_nt_rollout (layers = 0), pulse_tfe_nt_rollout_search at one layer (layers = 1, backed NULL) or
 * pulse_tfe_nt_rollout_backed at one layer (layers = 1, backed set), with one difference: game g begins on the board packed in
 * start[g] (the state key: 4 bits of log2(tile) per cell) instead of its reset board, where that board is USABLE:
 *   - it is not 0;
 *   - at least one of its four moves changes it;
 *   - it holds no nibble 15 (a 32,768 tile stops a game).
 * Otherwise the game begins at its reset exactly as in those launches, and 0 is stored into start[g]: after the launch start[g] != 0
 * says exactly which games began from their start board.  Nothing else differs.  Move t of game g, counted from the start board,
 * draws Philox4x32-10(agent_seed, board_id0 + g, t), and the spawn after it Philox4x32-10(env_seed, board_id0 + g, t + 1); total_score
 * and episode_reward count from the start board; max_steps, the 32,768 cap, the terminal bit, stats[0] and stats[3] and the records
 * (keys, values, steps, backed) are as before, so every learner reads them unchanged.  With start all 0 the launch's outputs are
 * those of its sibling, byte for byte.
 * start: device uint64[n_games], read and, where unusable, written.  One lane per game at layers = 0, one group of 32 lanes at 1.
 *
 * pulse_tfe_nt_restart_pick: the next round's `start` from the round just recorded.  For game g let L = min(lengths[g], max_steps)
 * and t* = (int)floor((double)L * fraction), one float64 multiply:
 *   L >= min_length and 1 <= t* <= L - 1:  start[g] = the board move t* was made on: keys[(t* - 1) * n_games + g] with the spawn of
 *                                          Philox4x32-10(env_seed, board_id0 + g, t*) words x (cell) and y (tile) put into it;
 *   otherwise:                             start[g] = 0.
 * env_seed and board_id0 are those of the launch that RECORDED keys.  The board is one the recorded game stood on and moved on: it
 * is usable by construction.  picked: device int64[2], added to: [0] the boards picked, [1] the sum of their t*.
 * Zero-initialise the struct: reserved0 must be 0.
 *
 * PULSE_EINVAL, before anything is launched: for the roll-out what pulse_tfe_nt_rollout refuses, under this name; `layers` other
 * than 0 or 1 ("layers must be 0 or 1": two layers are not built); backed set with layers = 0; backed or start not 8-byte aligned;
 * start null.  For the pick: null options, n_games < 1, max_steps outside 1..65,535, fraction not in the open interval (0, 1) (NaN
 * included), min_length outside 2..65,535, reserved0 not 0, a null pointer, keys / start / picked not 8-byte or lengths not 4-byte
 * aligned. */
int pulse_tfe_nt_rollout_from(const PulseTfeNtRollout* o, int32_t layers, double* backed, uint64_t* start, void* stream);
typedef struct PulseTfeNtRestartPick {
    int32_t n_games, max_steps;
    uint64_t env_seed, board_id0;       /* of the round that recorded keys */
    double fraction;                    /* in (0, 1) */
    int32_t min_length, reserved0;
    const uint64_t* keys;               /* uint64[max_steps * n_games] */
    const int32_t* lengths;             /* int32[n_games] */
    uint64_t* start;                    /* uint64[n_games], written */
    int64_t* picked;                    /* int64[2], added to */
} PulseTfeNtRestartPick;
int pulse_tfe_nt_restart_pick(const PulseTfeNtRestartPick* o, void* stream);

/* ---- ... and the training roll-out at the depth the board chooses, per move.  Opt-in: a caller that never calls it keeps every launch
 * above unchanged.  pulse_tfe_nt_rollout_search's games and records under pulse_tfe_nt_evaluate_search_adaptive's policy: for the
 * board B a move is made from, n = its empty cells, the q the greedy scan reads are those of the two-layer search with
 * n <= deep_empty_max and those of the one-layer search otherwise, bit for bit.  What a move records is unchanged: keys[t, g] the
 * chosen afterstate, values[t, g] the NETWORK's V of it, steps[t, g] the action, the reward and the game-over bit.
 *   backed:      device float64[max_steps * n_games], or NULL: pulse_tfe_nt_rollout_backed's word per move, the largest q over the
 *                candidate moves, of the q at the depth the board chose; NULL records none.
 *   start:       device uint64[n_games], or NULL: pulse_tfe_nt_rollout_from's start boards -- game g begins on start[g] where that
 *                board is usable and at its reset otherwise, with 0 stored into start[g]; NULL begins every game at its reset.
 *   depth_stats: device int64[2], or NULL: [0] += the moves whose q came from two layers, [1] += those from one layer; every move of
 *                every game counts, the epsilon branch's too; added once per game, at its end, and never zeroed by the launch.
 * deep_empty_max = 16 is pulse_tfe_nt_rollout_search / _backed at layers = 2, record for record.  One game per workgroup of 256 lanes.
 *
 * PULSE_EINVAL, before anything is launched, in this order: null options; `deep_empty_max` outside 0..16 ("deep_empty_max must be in
 * 0..16"); depth_stats, backed or start not 8-byte aligned; what pulse_tfe_nt_rollout refuses of the struct, under this name. */
int pulse_tfe_nt_rollout_adaptive(const PulseTfeNtRollout* o, int32_t deep_empty_max, double* backed, uint64_t* start,
                                  int64_t* depth_stats, void* stream);

/* ---- ... and weight sets by tile stage ("multi-stage TD"; promoting a stage's weights into a new one is "weight promotion").
 * Opt-in: a caller that never calls these four keeps every launch above unchanged.
 *
 * A staged network is S = n_stages = 1..4 copies of the tables, chosen per board by how far the game has come.  Let m(B) be the
 * largest nibble of the packed board B and threshold[0] < ... < threshold[S - 2] nibbles in 1..15:
 *   stage(B) = the number of s with threshold[s] <= m(B)        (threshold[s - 1] is the nibble at which stage s begins)
 * Stage s owns the weights [s * W, (s + 1) * W), W = net.n_weights (still the sum of 16^len: ONE stage's size), so net.weights is
 * float[S * W], acc int64[S * W][2], acc_abs int64[S * W]; S * W <= 2^29 by the network's own limits (8 tuples of length 6).  A feature's index is that of the one-stage network plus
 * stage * W.  V(B) is read in the stage of B itself, the afterstate whose value it is -- float64, tuple-major, image order, as before;
 * a recorded move's adds go to the stage of keys[t].  Targets need nothing new: values[t + 1] was recorded in whatever stage that
 * afterstate was in, so a difference crosses a stage boundary by itself.  The learners still read no weight, and the backward walks
 * are the launches they were.  With n_stages = 1 every output is the parent entry point's, byte for byte.
 * Bytes of threshold at and beyond n_stages - 1 must be 0.  Zero-initialise the struct: reserved0 must be 0.
 *
 * pulse_tfe_nt_rollout_staged: pulse_tfe_nt_rollout_from's contract word for word -- layers 0 or 1, backed only with layers 1, start
 *   read and zeroed where unusable (all 0: the games from reset) -- with V read by stage.
 * pulse_tfe_nt_learn_staged: the four learners through the superset struct.  deltas NULL (needs lambda == 0 and backed NULL):
 *   pulse_tfe_nt_learn's one-step differences; deltas set and backed NULL: pulse_tfe_nt_learn_lambda's walk; backed set (needs
 *   deltas): pulse_tfe_nt_learn_backed's walk; acc_abs set: the third accumulator.  The walks are the existing launches; the adds go
 *   to the stage of keys[t].
 * pulse_tfe_nt_evaluate_staged: layers 0 pulse_tfe_nt_evaluate, layers 1 pulse_tfe_nt_evaluate_search.
 * pulse_tfe_nt_search_staged: pulse_tfe_nt_search, one chance layer.
 * The apply launches need nothing new: pulse_tfe_nt_apply / pulse_tfe_nt_apply_tc once per stage on that stage's slice of weights,
 * acc, acc_abs, e and a (tc_stats is added to).
 *
 * PULSE_EINVAL, before anything is launched: everything the parent entry point refuses, under the new name; null stages; n_stages
 * outside 1..4; a threshold outside 1..15 or not strictly increasing; a non-zero byte beyond n_stages - 1; reserved0 not 0;
 * `layers` outside what the entry point takes (two layers are not built on stages). */
#define PULSE_TFE_NT_MAX_STAGES 4
typedef struct PulseTfeNtStages { int32_t n_stages; uint8_t threshold[4]; int64_t reserved0; } PulseTfeNtStages;  /* 16 bytes */
int pulse_tfe_nt_rollout_staged(const PulseTfeNtRollout* o, const PulseTfeNtStages* stages, int32_t layers, double* backed, uint64_t* start,
                                void* stream);
int pulse_tfe_nt_learn_staged(const PulseTfeNtLearnBacked* o, const PulseTfeNtStages* stages, void* stream);
int pulse_tfe_nt_evaluate_staged(const PulseTfeNtEval* o, const PulseTfeNtStages* stages, int32_t layers, void* stream);
int pulse_tfe_nt_search_staged(const PulseTfeNtSearch* o, const PulseTfeNtStages* stages, void* stream);

/* ---- ... and games continued across rounds: a round of a small max_steps = K plays K moves of every game, and the next round takes
 * the cut games up again under the new weights.  Opt-in: a caller that never calls this keeps every launch above unchanged.
 *
 * pulse_tfe_nt_continue_pick: from the round just recorded, the next round's `start` (pulse_tfe_nt_rollout_from, _rollout_staged), the
 * score and moves of every game so far, and the whole games that finished.  For game g let L = min(lengths[g], max_steps) (at least
 * 1), b = steps[(L - 1) * n_games + g], A = keys[(L - 1) * n_games + g] (the last afterstate) and id = board_id0 + g.
 *   CUT -- b has no terminal bit, A holds no nibble 15 and L == max_steps.  The learners skipped move L - 1 (it has no successor), so
 *     the game is taken up on the board that move was made on and the move is decided again:
 *       start[g]        = keys[(L - 2) * n_games + g] with the spawn of Philox4x32-10(env_seed, id, L - 1) words x (cell) and y (tile);
 *       carry_score[g] += total_score[g] - sc, sc the merge score of moving that board by the action b & 3;
 *       carry_moves[g] += L - 1;                finished[5] += 1.
 *     The launch does not check that the move gives A again.
 *   FINISHED -- every other game: it is over, or it stopped at the 32,768 tile.  The whole game has the score
 *     s = carry_score[g] + total_score[g] and carry_moves[g] + L moves, and its largest tile is that of A with the spawn of
 *     Philox4x32-10(env_seed, id, L): the board pulse_tfe_nt_evaluate's game ends on.  Added to `finished`:
 *       [0] games  [1] moves  [2] sum of s  [3] sum of s * s  [4] max of s  [6] games with carry_moves[g] > 0 (continued at least
 *       once)  [7] games whose A holds a nibble 15;  [8 + k] games whose largest tile is 2^k (k = 15: 32,768).
 *     start[g] = 0, carry_score[g] = 0, carry_moves[g] = 0: the next round's game g begins at its reset.
 * env_seed and board_id0 are those of the launch that RECORDED the round.  One lane per game; no other launch need have finished
 * but the recording one.  Zero-initialise the struct: reserved0 must be 0.  sizeof == 96.
 *
 * PULSE_EINVAL, before anything is launched: null options, n_games < 1, max_steps outside 2..65,535, reserved0 not 0, a null
 * pointer, keys / total_score / start / carry_score / finished not 8-byte or lengths / carry_moves not 4-byte aligned. */
typedef struct PulseTfeNtContinuePick {
    int32_t n_games, max_steps;         /* max_steps: the segment length K of the round that recorded */
    uint64_t env_seed, board_id0;       /* of the round that recorded */
    int64_t reserved0;
    const uint64_t* keys;               /* uint64[max_steps * n_games] */
    const uint8_t* steps;               /* uint8[max_steps * n_games] */
    const int32_t* lengths;             /* int32[n_games] */
    const int64_t* total_score;         /* int64[n_games] */
    uint64_t* start;                    /* uint64[n_games], written */
    int64_t* carry_score;               /* int64[n_games], read and written */
    int32_t* carry_moves;               /* int32[n_games], read and written */
    int64_t* finished;                  /* int64[24], added to (word 4: a maximum) */
} PulseTfeNtContinuePick;
int pulse_tfe_nt_continue_pick(const PulseTfeNtContinuePick* o, void* stream);

/* ---- ... and rank-parallel rounds: R ranks play disjoint games of one round, each learns into its own accumulators, and the
 * accumulators are summed before the apply launch runs, replicated, on every rank.  The learners' adds are integers, so the sum is
 * bit for bit the accumulator of one process that played all the games.  A round touches few of the cells, so what travels is a
 * list of the touched cells.  Opt-in: a caller that never calls these keeps every launch above unchanged.
 *
 * The list: int64[4 + 4 * capacity], a header {found, written, 0, 0} and then 32-byte entries {index, sum, cnt, abs}.
 *
 * pulse_tfe_nt_acc_pack: the header is zeroed on the stream; then every cell i < n_entries with acc[i].cnt > 0 -- cnt, not sum: a
 * cell whose differences cancel was visited all the same -- becomes the entry {i, acc[i].sum, acc[i].cnt, acc_abs ? acc_abs[i] : 0}
 * at a slot of its own.  found = the number of such cells; an entry whose slot is >= capacity is not written; written =
 * min(found, capacity), set by a one-lane launch behind the first.  Nothing is written outside list[0, 4 + 4 * capacity); acc and
 * acc_abs are only read; `stats` is not used.  The ORDER of the entries follows the order of the launch's atomics and is not
 * defined; with found <= capacity the SET of entries is.  One returning atomic per workgroup and pass that found a live cell.
 *
 * pulse_tfe_nt_acc_unpack: the header's `written` is read on the device.  written > capacity: nothing is added and stats[1] +=
 * capacity.  Otherwise, for every slot below written: an entry with index < n_entries and cnt > 0 is added -- acc[index].sum +=
 * sum, acc[index].cnt += cnt, and with acc_abs, acc_abs[index] += abs -- by 64-bit atomics, so the lists of several ranks may be
 * added by launches that run together; any other entry adds nothing.  stats[0] += entries added, stats[1] += entries refused.  The
 * list is only read.
 *
 * n_entries covers all stages of a network with weight sets by stage.  Zero-initialise the struct: reserved0 must be 0.  sizeof == 56.
 *
 * PULSE_EINVAL, before anything is launched: null options, n_entries outside 1..2^32, acc null or not 16-byte aligned, acc_abs not
 * 8-byte aligned, capacity 0, list null or not 32-byte aligned, stats null (unpack) or not 8-byte aligned, reserved0 not 0. */
typedef struct PulseTfeNtAccList {
    uint64_t n_entries;                 /* accumulator cells covered: total weights, all stages */
    int64_t* acc;                       /* int64[n_entries][2] = {sum, cnt}, 16-byte aligned; pack: read, unpack: added to */
    int64_t* acc_abs;                   /* int64[n_entries] or NULL; pack: read, unpack: added to */
    uint64_t capacity;                  /* entries the list has room for, >= 1 */
    int64_t* list;                      /* int64[4 + 4 * capacity], 32-byte aligned; pack: written, unpack: read */
    int64_t* stats;                     /* unpack only, int64[2], ADDED TO: [0] entries added, [1] entries refused */
    int64_t reserved0;
} PulseTfeNtAccList;
int pulse_tfe_nt_acc_pack(const PulseTfeNtAccList* o, void* stream);
int pulse_tfe_nt_acc_unpack(const PulseTfeNtAccList* o, void* stream);

/* ---- the learner's action selection (environments/Poker/Player.py:178-253) ---------------------
 * PokerQNetwork.network in eval mode: Linear(state_dim,128) GELU Linear(128,128) GELU [Dropout] Linear(128,64)
 * GELU [Dropout] Linear(64,32) GELU Linear(32,n_actions) (:189-201).  Weights are the module's own tensors:
 * torch.nn.Linear layout w[out][in] row-major fp32 on the device, 16-byte aligned; nothing is packed or cached
 * between calls, so an optimizer step is visible to the next call. */
typedef struct PulseQNet {
    int32_t state_dim, n_actions;                       /* n_actions <= 32 */
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4, *w5, *b5;
} PulseQNet;
/* q_out[r, :] = network(states[r, :]) (Player.py:235-240); states fp32 rows of state_dim at row_stride floats. */
int pulse_qnet_forward(const PulseQNet* net, const float* states, int64_t row_stride, int32_t n_rows, float* q_out,
                       void* stream);
/* PokerQNetwork.get_actions (Player.py:242-253) fused with build_actions' mask (utils.py:108-119): for every row
 * r with seat_idx[r] == q_seat (seat_idx NULL: every row) actions[r] = uniform{0..n_actions-1} with probability
 * epsilon, else the first argmax of the Q row; other rows are left untouched.  Draws are words x (explore) and y
 * (action) of Philox4x32-10(seed, table_id0 + r, step), the stream pulse_poker_policy uses for scripted seats.
 * q_out NULL or fp32[n_rows, n_actions] (selected rows written).  row_mask_out (NULL or device uint8[n_rows], needs
 * seat_idx): row_mask_out[r] = (seat_idx[r] == q_seat) && !terminated[r] (terminated NULL = none) for EVERY row --
 * the trainer's `q_mask & ~terminated` (scripts/Poker/trainGPU.py:85), the row_mask of pulse_qnet_train_step.
 * Kernels: with seat_idx, state_dim a multiple of 4 in 13..64, n_actions <= 16 and 16-byte aligned rows (the Poker shapes)
 * sixteen rows per wavefront with the activations in registers (csrc/qnet_rows16.h); otherwise cooperative 32-row tiles
 * (csrc/qnet_device.h).  The two sum a layer's inputs in different orders: Q values agree to rounding (2e-5 at |Q| = O(1)),
 * actions wherever the two best Q values of a row are further apart than that. */
int pulse_qnet_act(const PulseQNet* net, const float* states, int64_t row_stride, int32_t n_rows,
                   const int32_t* seat_idx, int32_t q_seat, float epsilon, uint64_t seed, uint64_t step,
                   uint64_t table_id0, int64_t* actions, float* q_out, const uint8_t* terminated,
                   uint8_t* row_mask_out, void* stream);
/* The same (seat_idx and row_mask_out required) for a trainer that will call pulse_qnet_train_step / _grads next with
 * THIS `states` as its states and THIS row_mask_out as its row_mask: the rows that call trains on (row_mask & seat
 * status ACTIVE / ALLIN) are known already, so their lists are written to the trainer's select_scratch here and the
 * training call skips its selection launch -- set PulseQNetTrain.select_from_act = 1 for that call (and only that one).
 * select_words: at least 259 per 256 rows + 512.  (Shapes that take the 32-row-tile kernels, see pulse_qnet_act: with 517 per
 * 256 rows + 512 and 262,144 rows or more the selection runs as TWO launches -- the windows only list the learner's rows (in
 * the extra words), a second launch runs them in full tiles -- same results.) */
int pulse_qnet_act_select(const PulseQNet* net, const float* states, int64_t row_stride, int32_t n_rows,
                          const int32_t* seat_idx, int32_t q_seat, float epsilon, uint64_t seed, uint64_t step,
                          uint64_t table_id0, int64_t* actions, const uint8_t* terminated, uint8_t* row_mask_out,
                          int32_t* select_scratch, int64_t select_words, void* stream);

/* PokerQNetwork.train_step (Player.py:255-294) as up to three launches: (0) the row filter as lists of row ids per
 * window (skipped when pulse_qnet_act_select wrote them); (1) the listed rows in tiles of 32, dealt to the workgroups: TD target +
 * forward (train mode) + backward on the matrix cores, gradient sums accumulated per workgroup; (2) reduction of the
 * workgroups' slices, then -- in the same launch -- gradient mean / clip_grad_norm_ / AdamW / target sync.
 * The network and its target each live in ONE flat fp32 buffer of pulse_qnet_param_count() floats laid out
 * w1,b1,w2,b2,w3,b3,w4,b4,w5,b5 (torch layouts); `net` / `target` hold the ten views.  grad, exp_avg, exp_avg_sq: flat
 * buffers of the same length (moments zero before the first call).  partials: device fp32[max_blocks *
 * pulse_qnet_slice_floats()] scratch (max_blocks = number of persistent workgroups, 256 = one per CU; a workgroup's
 * slice is laid out for its own stores, not in parameter order).  step: device int64 optimizer step count
 * (bias correction, target sync every update_freq steps).  stats: device fp32[4] scratch.  report: device fp32[4] out:
 * [0] rows trained on, [1] the MSE loss, [2] gradient norm before clipping, [3] 0, or -1: the reduce + AdamW launch's
 * workgroups did not all gather within meet_wait_ticks (a co-tenant on the GPU), the meeting was called off AS A WHOLE and no
 * parameter, moment or step count moved; the next pulse_qnet_train_* call then returns PULSE_EINTERNAL once.  The in-launch
 * meeting is only used where the device holds the launch's whole grid at once (asked once per device), never with
 * separate_apply = 1 (AdamW as a launch of its own, what pulse_qnet_train_grads / _apply always do).
 * Row filter: row_mask[r] != 0 (NULL: all) and states[r][12] in {0, 2} (:261); if no row passes, nothing changes (:262).
 * Trainer bookkeeping folded in (both optional, scripts/Poker/trainGPU.py:86,96): terminated (device uint8[n_rows],
 * NULL = skip) gets terminated[r] |= dones[r]; reward_sum (device double, NULL = skip) += sum of rewards over the
 * row_mask rows (before the status filter).
 * Dropout(.1) after the 2nd and 3rd GELU draws 16-bit uniforms from Philox4x32-10(seed ^ 0xD50F0D50F0, table_id0 + r,
 * 32 * step_counter + unit / 8); dropout_p = 0 disables it.  Sums over rows run in a fixed order: deterministic for
 * a given n_rows and max_blocks (whichever launch made the row lists). */
typedef struct PulseQNetTrain {
    PulseQNet net, target;
    float *params, *target_params, *grad, *exp_avg, *exp_avg_sq;
    int64_t* step;
    float *stats, *report, *partials;
    float lr, weight_decay, beta1, beta2, eps, max_grad_norm, gamma, dropout_p;
    int32_t update_freq, max_blocks;
    int32_t* select_scratch;        /* device int32[select_words]: the row-selection launch's lists */
    int64_t select_words;           /* >= 259 * ceil(n_rows / 256) + 512 for the largest n_rows passed */
    int32_t select_from_act;        /* 1: the lists in select_scratch were written by pulse_qnet_act_select (see there) */
    int32_t separate_apply;         /* 1: AdamW in a launch of its own (no in-launch meeting of the reduce launch's workgroups) */
    int64_t meet_wait_ticks;        /* how long a workgroup waits at that meeting, in ticks of the 100 MHz clock; 0 = 5 s */
    int32_t debug_meet_extra;       /* test hook: arrivals the meeting expects beyond the grid's own (> 0: it never comes about) */
    int32_t reserved0;
    float* stability;               /* NULL: off (the launches are exactly those without it); else device fp32[16], below */
} PulseQNetTrain;
/* Training-stability metrics (PulseQNetTrain.stability; the reference's utils/stability.py), taken inside the launches above:
 * the training launch totals |td| and Q(s, a) (the train-mode, dropout value) over the rows next to the loss terms, the
 * reduce / AdamW launch writes
 *   per-call block, every call that launches:  [0] rows, [1] mean |td|, [2] mean Q(s, a), [3] min Q(s, a), [4] max Q(s, a),
 *                  [5] gradient norm before clipping, [6] clipped (1 if [5] > max_grad_norm, else 0), [7] loss;
 *                  all 0 when rows is 0 or the meeting was called off (report[3] = -1)
 *   accumulator, added to only by calls with rows > 0:  [8] measured steps, [9] sum of [1], [10] sum of [2], [11] min of [3],
 *                  [12] max of [4], [13] sum of [6], [14] sum of [7], [15] 0.
 * Cleared state of the accumulator: [11] = +inf, [12] = -inf, everything else 0 (PokerQNetwork.clear_stability_metrics); the
 * per-call block needs no clearing.  An episode's values are then td_error = [9] / [8], q_mean = [10] / [8] (the mean of the
 * per-step means, not over rows), q_min = [11], q_max = [12], clip_rate = [13] / [8] (0 everywhere while [8] == 0).
 * pulse_qnet_train_grads (data-parallel) leaves the UNNORMALISED totals of its rows in [0..4] = {rows, sum |td|, sum Q,
 * min Q, max Q}; the caller all-reduces [0..2] with SUM, [3] with MIN and [4] with MAX (one MAX all-reduce of {-[3], [4]} does
 * both), then pulse_qnet_train_apply normalises them and accumulates: the metrics of the job-wide batch, as the gradient. */
int pulse_qnet_param_count(int32_t state_dim, int32_t n_actions);
int pulse_qnet_slice_floats(void);
/* How many reduce + AdamW launches of this process have called their meeting off so far (a count in pinned host memory the
 * launches add to: reading it waits for nothing; it is behind by the launches still in flight). */
int64_t pulse_qnet_called_off_meetings(void);
int pulse_qnet_train_step(const PulseQNetTrain* t, const float* states, int64_t row_stride, const int64_t* actions,
                          const float* rewards, const float* next_states, int64_t next_stride, const uint8_t* dones,
                          const uint8_t* row_mask, int32_t n_rows, uint64_t seed, uint64_t step_counter,
                          uint64_t table_id0, uint8_t* terminated, double* reward_sum, void* stream);
/* The same in two halves, for data-parallel training (one process per GPU): pulse_qnet_train_grads runs launches 1-2
 * and leaves the UNNORMALISED gradient sum in t->grad and {sum g^2, rows, sum td^2} in t->stats[0..2] without touching
 * t->step; the caller all-reduces t->grad and t->stats[1..2] over the ranks (RCCL), stores the squared norm of the
 * reduced gradient in t->stats[0], adds 1 to *t->step if the reduced row count is positive, and calls
 * pulse_qnet_train_apply (launch 3) -- every rank then applies the identical update. */
int pulse_qnet_train_grads(const PulseQNetTrain* t, const float* states, int64_t row_stride, const int64_t* actions,
                           const float* rewards, const float* next_states, int64_t next_stride, const uint8_t* dones,
                           const uint8_t* row_mask, int32_t n_rows, uint64_t seed, uint64_t step_counter,
                           uint64_t table_id0, uint8_t* terminated, double* reward_sum, void* stream);
int pulse_qnet_train_apply(const PulseQNetTrain* t, void* stream);

/* The first half of the trainer's step with the learner in it as ONE launch (scripts/Poker/trainGPU.py:79-83 with the learner at
 * a seat: build_actions -> env.step): pulse_qnet_act_select on the observation act->states (the learner's actions into
 * `actions`, the trainer's mask into act->row_mask_out, the training launch's row lists into act->select_scratch) followed by
 * pulse_poker_policy_step on `v` -- the same results word for word; the workgroup that picks the actions of a window of 128
 * tables steps those tables itself, so nothing grid-wide lies between the two and the tables' state travels from HBM while
 * the forward runs.  Needs n_games % 128 == 0, max_players <= 10, 16-byte aligned fp32 rows of 16..40 inputs (a multiple of
 * 8); PULSE_EINVAL otherwise: make the two calls instead.  act->states must NOT be the buffer v->obs writes (the trainer's
 * double-buffered observations).  stoprule: as pulse_poker_rollout (the done tables after the step are counted for it by the
 * launch itself), or NULL. */
typedef struct PulseQNetAct {
    const float* states; int64_t row_stride;     /* device fp32 rows, row_stride floats apart: the observation the learner acts (and trains) on */
    const int32_t* seat_idx; int32_t q_seat;     /* rows with seat_idx[r] == q_seat are the learner's */
    float epsilon;
    uint64_t seed, step, table_id0;              /* the learner's exploration stream (pulse_qnet_act) */
    const uint8_t* terminated; uint8_t* row_mask_out;
    int32_t* select_scratch; int64_t select_words;
} PulseQNetAct;
int pulse_poker_act_policy_step(const PulsePokerView* v, const uint8_t* agent_types, uint64_t seed, uint64_t step_counter,
                                uint64_t table_id0, int64_t* actions, float* rewards, const PulseQNet* net,
                                const PulseQNetAct* act, void* stoprule, void* stream);

/* ---- Particle2D (environments/Particle2D/Particle2D.py:22-30) ---------------------------------- */
int pulse_particle2d_step(float* state, const float* action, int32_t* steps, float* obs_out, float* rewards,
                          uint8_t* terminated, int32_t n, float dt, int32_t max_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PULSE_ENV_H */
