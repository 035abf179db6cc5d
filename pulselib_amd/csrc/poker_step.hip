// poker_step.hip -- the fused hold'em step for gfx950: one launch per PokerGPU.step, or ONE launch for a whole
// chunk of roll-out steps with the tables' state held in registers in between.
//
// Replaces the ~1,700 eager torch dispatches of one PokerGPU.step (environments/Poker/PokerGPU.py:527-633).
//
// Mapping: a table is owned by LPT adjacent lanes (4 = one DPP quad; the code also compiles for 2), lane j owns the SPL
// consecutive seats SPL*j .. SPL*j+SPL-1: 64/LPT tables per 64-wide wavefront.  Per-table scalars are replicated in the
// table's lanes, so the scalar part of the state machine costs 1/LPT wave-instruction per table; a lane's cells of a
// per-seat row ([N,P] int32, the reference's own layout) are one 12- or 16-byte load.  Seat sets (ACTIVE seats,
// contenders, winners) are bitmasks OR-reduced across the table's lanes with DPP quad_perm modifiers (no LDS); "first
// ACTIVE seat after x" is a rotate + ffs on the mask; side-pot layers are min/max butterflies.  Single steps run with
// LPT = 4, chunks with LPT = 2 up to ten seats (see lanes_for below for the measurements).  All integer arithmetic is the reference's; the fp32 reward keeps torch's
// op order (no contraction; tanh rounded once from double).
//
// Memory: single step -- state is read once and only the words that changed are written back, in the reference's
// own SoA tensors, so the drop-in class exposes them unchanged.  Chunk (pulse_poker_rollout) -- state is read once
// per chunk, the steps store observation / reward / done flag into ping-pong buffers so that memory is exactly what n
// single launches leave behind -- only the last two steps before a possible end of the launch are visible there, and only
// those compute and store them ("live steps", at the step loop) -- and the changed state words and the action are written
// once at the end.  The 130 MB hand-rank
// table is only touched when a poked state misses the evaluation cache the reset kernel fills.
#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "poker_device.h"
#include "poker_launch.h"
#include "qnet_device.h"

using namespace pulse_dev;
using pulse::ChunkArgs;
using pulse::PolicyArgs;

namespace {

// threads per workgroup of the step kernel.  Its wavefronts do not cooperate (only the stop rule's sum in workgroup 0
// does), so smaller workgroups only change how finely the dispatcher refills a CU: measured per 5-step chunk at 65,536 /
// 1,048,576 tables, 256 threads: 39.5 / 421 us, 128: 39.6 / 404, 64: 40.5 / 400.
#ifndef PULSE_STEP_BLOCK
#define PULSE_STEP_BLOCK 128
#endif
constexpr int kStepBlock = PULSE_STEP_BLOCK;

// dwords of LDS per wavefront of a chunk launch: the observation staging block + the staged read-only rows
// (hole cards [T][P_][2], 7-card rank | hand class << 16 [T][P_], flop and turn equities [T][2][P_], deck window [T][8]);
// 16-byte aligned so that the observation block of the next wavefront is.
// SLIM (MULTI == 2): the river's equities are not staged (they follow from the 7-card rank) and the hand class shares
// a word with the rank: 5 instead of 7 dwords per seat, which is what lets three two-lane wavefronts per SIMD fit the LDS at large batches.
__host__ __device__ constexpr int chunk_lds_dwords(int obs_size, int seats, int tables, bool slim) { return (tables * (obs_size + seats * (slim ? 5 : 7) + 8) + 3) & ~3; }

constexpr int kVerdictStride = 16;                          // long longs between the 64 copies of a relayed verdict word (one 128-byte line each)

// The kernel-argument segment as the kernel below receives it.  Values needed once inside (or after) the long step loop
// are re-read from it through a constant-address-space pointer (scalar loads) instead of being kept in scalar
// registers across the loop, where they were spilled to vector lanes.
struct StepKernargs { PulsePokerView v; int64_t* actions; const int32_t* actor_idx_in; float* rewards; PolicyArgs pa; ChunkArgs ca; };
typedef const __attribute__((address_space(4))) StepKernargs* StepKernargsPtr;
static_assert(offsetof(StepKernargs, v) == 0 && offsetof(StepKernargs, actions) == sizeof(PulsePokerView), "the view is the first kernel argument");
static_assert(offsetof(StepKernargs, pa) == sizeof(PulsePokerView) + 24 && offsetof(StepKernargs, ca) == offsetof(StepKernargs, pa) + sizeof(PolicyArgs), "kernel arguments");
// (PolicyArgs' two carried check points are pulse::StopRuleCarry records: the same words, in the same places, as when they were eight loose fields)
static_assert(sizeof(pulse::StopRuleCarry) == 32 && offsetof(PolicyArgs, wave_done) == 32 && offsetof(PolicyArgs, carry) == 40 &&
              offsetof(PolicyArgs, wave_done_mid) == 104 && offsetof(PolicyArgs, verdict_host) == 120 && offsetof(PolicyArgs, lng) == 160 &&
              sizeof(pulse::StopRuleLong) == 72 && sizeof(PolicyArgs) == 232, "PolicyArgs layout");

// ---- long launches (pulse_internal.h: StopRuleLong): the check points a launch takes itself.
// The arrival words are agent-scope atomics (performed at the memory side: the per-XCD L2s are not coherent), the verdict
// words RELAXED system-scope accesses like the relayed word of a paired launch: every word carries its own key {launch
// id, check point}, and a wavefront's count travels inside its arrival, so no other data needs ordering with them.
typedef __attribute__((address_space(1))) long long GlobalLL;
constexpr int kLongSetWords = (1 + pulse::kLongWords) * kVerdictStride;      // long longs of one set of arrival words

// Settles the verdict of check point r with `word` (a decision, or "called off") unless the other word landed first: a
// compare-and-swap on the slot's first copy from whatever an earlier check point left there (a word with another key:
// "pending"), then the remaining copies.  Returns the word that stands.  Whoever wrote it tells the host, where it
// settles the launch's length.  Called by every active lane of the wavefront (the lanes are 0 .. n - 1).
__device__ __forceinline__ long long long_settle(StepKernargsPtr ka, int r, long long word) {
    GlobalLL* slot = (GlobalLL*)ka->pa.lng.verdicts + (size_t)(r & (pulse::kLongSlots - 1)) * 64 * kVerdictStride;
    const int lane = threadIdx.x & 63;
    long long stands = 0; int won = 0;
    if (lane == 0) {
        long long cur = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (;;) {
            if ((cur >> 8) == (word >> 8)) { stands = cur; break; }
            if (__hip_atomic_compare_exchange_strong(slot, &cur, word, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { stands = word; won = 1; break; }
        }
    }
    won = __builtin_amdgcn_readfirstlane(won);
    stands = ((long long)__builtin_amdgcn_readfirstlane((int)(stands >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)stands);
    if (won) {
        const int n_act = __popcll(__ballot(1));
        for (int k = lane; k < 64; k += n_act)
            if (k) __hip_atomic_store(slot + k * kVerdictStride, stands, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const int flags = (int)(stands & 3), m = ka->pa.lng.n_chunks;
        // (ONE such word per launch: behind an "over" or "called off" nobody arrives at a later check point -- long_check_point.
        // The host holds it to that: the second word counts the writes.)
        if (lane == 0 && (flags || r == m - 3)) {
            __hip_atomic_store((GlobalLL*)ka->pa.lng.host, (ka->pa.verdict_id << 16) | (long long)((flags ? r + 2 : m) << 8) | flags, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_fetch_add((GlobalLL*)ka->pa.lng.host + 1, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    return stands;
}

// The check point behind the launch's q-th chunk (q >= 1): `c` = this wavefront's done tables, `wid` = its number in the
// launch.  Stores the count in the ring, reads the verdict of check point q - 2 where another chunk would follow, and --
// only if that verdict lets the launch go on -- arrives (check points the launch decides: r = q - 1 <= m - 3; the last two
// are the next launch's carries, as after a pair).  The order matters: every wavefront reads the same verdict word, so behind
// an "over" or a "called off" NO wavefront arrives again, no later verdict is decided, and the word that told the host how
// many chunks the launch runs stays the only one (arriving first, the next check point was decided "over" too and its word
// overwrote the host's a chunk later).  true: the launch ends here.
// `taken`: the wavefront has that verdict from its early look (long_peek below; 0: it has not) -- 1 = "go on", 2 = "over" or
// "called off".  It is the word the read here would find (a settled word stays until its slot's next check point, four later,
// which nobody decides before this wavefront has arrived three more times), so the read is skipped and the rest is the same:
// behind a 2 the wavefront does not arrive.
__device__ __forceinline__ bool long_check_point(StepKernargsPtr ka, int q, int c, uint32_t wid, bool arrives, int taken) {
    const int m = ka->pa.lng.n_chunks, r = q - 1;
    const bool lane0 = (threadIdx.x & 63) == 0;
    if (lane0) stg(ka->pa.lng.partials, ((uint32_t)((ka->pa.lng.slot0 + r) & 3) * (uint32_t)ka->pa.lng.max_partials + wid) * 4u, (uint32_t)c);
    if (q >= 2 && q < m && taken == 2) return true;
    if (q >= 2 && q < m && taken == 0) {
        const int rv = q - 2;
        const GlobalLL* copy = (const GlobalLL*)ka->pa.lng.verdicts + ((size_t)(rv & (pulse::kLongSlots - 1)) * 64 + (wid & 63u)) * kVerdictStride;
        const long long key = (ka->pa.verdict_id << 8) | (long long)rv;
        const long long t0 = wall_clock64();
        long long w;
        for (;;) {
            w = __hip_atomic_load(copy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((w >> 8) == key) break;
            if (wall_clock64() - t0 > ka->pa.lng.wait_ticks) { w = long_settle(ka, rv, (key << 8) | 2); break; }      // waited long enough: call it off (or read what landed first)
            __builtin_amdgcn_s_sleep(32);
        }
        if ((__builtin_amdgcn_readfirstlane((int)w) & 3) != 0) return true;
    }
    if (arrives && r <= m - 3) {
        long long word = 0;
        if (lane0) {
            const int W = ka->pa.lng.n_words, k = (int)(wid % (uint32_t)W);
            GlobalLL* top = (GlobalLL*)ka->pa.lng.arrive + (r & 1) * kLongSetWords;
            GlobalLL* mine = top + (1 + k) * kVerdictStride;
            const long long old = __hip_atomic_fetch_add(mine, (1ll << 32) | (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)(old >> 32) + 1 == (ka->pa.lng.n_waves + W - 1 - k) / W) {        // this word's last arrival: on to the second level
                const long long sum = (old & 0xFFFFFFFFll) + c;
                __hip_atomic_store(mine, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the word is zero again before anybody can learn that it is complete
                const long long old2 = __hip_atomic_fetch_add(top, (1ll << 32) | sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((int)(old2 >> 32) + 1 == W) {
                    const long long total = (old2 & 0xFFFFFFFFll) + sum;
                    __hip_atomic_store(top, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (r != ka->pa.lng.skip_cp)
                        word = (ka->pa.verdict_id << 16) | (long long)(r << 8) | (total >= (long long)ka->pa.lng.over_from ? 1 : 0);
                }
            }
        }
        const int has = __builtin_amdgcn_readfirstlane(word != 0 ? 1 : 0);
        if (has) {
            word = ((long long)__builtin_amdgcn_readfirstlane((int)(word >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)word);
            (void)long_settle(ka, r, word);
        }
    }
    return false;
}

// The early look at the verdict of check point rv = q - 2, at the bottom of step cp_at - 3, two steps before check point q reads
// it (the step loop): ONE relaxed system-scope load of this wavefront's copy of the slot, compared with the key long_check_point
// compares; no loop, no time-out, no store.  0 = pending (another key), 1 = "go on", 2 = "over" or "called off", wave-uniform
// (scalar: what it decides, end_at and n_steps, stays scalar).  `early` >= 2 counts the outcome (lane 0, one non-returning
// agent-scope add into the kLongWords lines behind the arrival words, {settled, pending} in line wavefront mod kLongWords -- on one
// line the adds of 2,048 wavefronts, performed at the memory side, queued for longer than a check interval and the count changed
// what it counted; a wave-uniform branch, the product executes none); 3 makes odd wavefronts find nothing.
__device__ __forceinline__ int long_peek(StepKernargsPtr ka, int rv, uint32_t wid, int early) {
    const GlobalLL* copy = (const GlobalLL*)ka->pa.lng.verdicts + ((size_t)(rv & (pulse::kLongSlots - 1)) * 64 + (wid & 63u)) * kVerdictStride;
    const long long w = __hip_atomic_load(copy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int lo = __builtin_amdgcn_readfirstlane((int)w), hi = __builtin_amdgcn_readfirstlane((int)(w >> 32));
    const long long word = ((long long)hi << 32) | (unsigned)lo, key = (ka->pa.verdict_id << 8) | (long long)rv;
    int taken = (word >> 8) != key ? 0 : (lo & 3) != 0 ? 2 : 1;
    if (early >= 2) {
        const int w_ = __builtin_amdgcn_readfirstlane((int)wid);      // (as a lane's value the wavefront number made everything behind it a vector)
        if (early == 3 && (w_ & 1)) taken = 0;
        if ((threadIdx.x & 63) == 0)
            (void)__hip_atomic_fetch_add((GlobalLL*)ka->pa.lng.arrive + 2 * kLongSetWords + (w_ & (pulse::kLongWords - 1)) * kVerdictStride + (taken ? 0 : 1), 1ll,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return taken;
}

// In-kernel timeline (diagnostic build only, -DPULSE_STAMPS=1 -> libpulse_hip_stamps.so; no stamp executes
// in the product): lane 0 of every wavefront stores s_memtime at phase boundaries into a buffer of its own.
#ifndef PULSE_STAMPS
#define PULSE_STAMPS 0
#endif
#if PULSE_STAMPS
__device__ unsigned long long* g_stamp_buf = nullptr;
#define STAMP(i) do { if ((threadIdx.x & 63) == 0 && g_stamp_buf) { __builtin_amdgcn_sched_barrier(0); \
    g_stamp_buf[((size_t)blockIdx.x * (kStepBlock / 64) + (threadIdx.x >> 6)) * 16 + (i)] = clock64(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// tanh rounded once from double: 1 - 2/(exp(2x)+1), everything in double (abs. error ~1e-16, far below the fp32 ulp:
// the result is the correctly rounded fp32 tanh except in ~1e-8 of cases).  The exponential is written out -- the
// library's exp + IEEE division carry special-case handling this argument range never needs, and double-precision
// vector instructions issue at half rate, so they were a sixth of the kernel's vector work: k = rint(y log2 e),
// r = y - k ln 2 (two-part constant), e^r by its Taylor series to r^13 (|r| <= 0.347: remainder < 5e-18), 2^k by
// ldexp; the reciprocal is v_rcp_f64 + two Newton steps.  Below |x| = 1e-3 the difference 1 - 2/(..) cancels, and
// x (1 - x^2/3) is exact to double rounding instead.  Against libm's tanh rounded to fp32: 2 of 4e7 arguments differ.
__device__ __forceinline__ float tanh_rn(float x) {
    const double xd = (double)x;
    double y = 2.0 * xd;
    y = fmin(fmax(y, -40.0), 40.0);                       // tanh is +-1 in fp32 long before; keeps 2^k finite
    const double k = rint(y * 1.4426950408889634);
    double r = fma(-k, 6.93147180369123816490e-01, y);
    r = fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                    // 1/13!
    p = fma(p, r, 2.08767569878681e-09);                  // 1/12!
    p = fma(p, r, 2.505210838544172e-08);                 // 1/11!
    p = fma(p, r, 2.755731922398589e-07);                 // 1/10!
    p = fma(p, r, 2.7557319223985893e-06);                // 1/9!
    p = fma(p, r, 2.48015873015873e-05);                  // 1/8!
    p = fma(p, r, 1.984126984126984e-04);                 // 1/7!
    p = fma(p, r, 1.388888888888889e-03);                 // 1/6!
    p = fma(p, r, 8.333333333333333e-03);                 // 1/5!
    p = fma(p, r, 4.1666666666666664e-02);                // 1/4!
    p = fma(p, r, 1.6666666666666666e-01);                // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const double d = ldexp(p, (int)k) + 1.0;              // exp(2x) + 1
    double q = __builtin_amdgcn_rcp(d);
    q = fma(fma(-d, q, 1.0), q, q);
    q = fma(fma(-d, q, 1.0), q, q);
    const double big = fma(-2.0, q, 1.0), small = xd * fma(-xd * xd, 0.3333333333333333, 1.0);
    return (float)(fabs(xd) < 1e-3 ? small : big);
}

// SPL consecutive int32 cells of a row, loaded as one 4-byte-aligned vector (global_load_dwordx3 / x4 take any dword address)
template <int N_> struct alignas(4) SeatCells { int32_t v[N_]; };

// WOBS (n_games % 16 == 0): the observation rows of a wavefront's 16 tables are one contiguous
// 16 x obs_size x 4 B block in HBM.  Written column by column they cost thirteen store instructions that each
// touch sixteen cache lines; with WOBS the lanes drop their values into the wavefront's LDS slice and the
// block leaves as three 1-KiB bursts (16 B per lane).  A wavefront's LDS operations retire in order, so no
// workgroup barrier is involved.
// MULTI: ca.n_steps steps in one launch (fused policy only); step i writes observation / done flag / reward into
// the even (i even) or odd buffers, as n single launches on the two ping-pong views would.
// ACT (the learner in the loop): the workgroup -- 256 threads, 128 tables at two lanes each -- first picks
// the learner's actions for its own window of tables (pulse_qnet::act_window, the body of the stand-alone act launch: masks,
// row lists for the training launch, forward on the matrix cores, argmax / epsilon draw) and then steps those tables: act ->
// env step has no grid-wide dependence, so the two launches of the trainer's step are one, and the tables' state is already
// on its way from HBM while the forward runs.  `qa` = the act launch's arguments (ACT only).
template <uint32_t PH, bool POLICY, int LPT, int SPL, bool WOBS, int MULTI, bool ACT>
__device__ __forceinline__ void poker_step_body(const PulsePokerView& v, int64_t* __restrict__ actions, const int32_t* __restrict__ actor_idx_in,
                                                float* __restrict__ rewards, const PolicyArgs& pa, const ChunkArgs& ca, const pulse_qnet::QNetArgs* qa) {
    static_assert((LPT == 4 && (SPL == 3 || SPL == 4)) || (LPT == 2 && (SPL == 5 || SPL == 8)), "lanes per table x seats per lane: 4x3, 4x4, 2x5, 2x8");
    constexpr int TPW = 64 / LPT;                                        // tables per wavefront
    constexpr int BLK = ACT ? 256 : kStepBlock;                          // threads per workgroup
    static_assert(!MULTI || (POLICY && PH == PULSE_PH_STEP), "a chunk is fused policy + full step");
    static_assert(!ACT || (MULTI == 1 && LPT == 2), "the act + step launch is a one-step chunk at two lanes per table");
    extern __shared__ int4 smem4[];
    if (POLICY && pa.carry[0].n > 0 && blockIdx.x == 0) {
        // The stop rule's previous check point: workgroup 0 sums its per-wavefront counts and publishes the total to
        // the host BEFORE its own tables.  (A separate last workgroup did this in the first version; at 65,536 tables
        // the grid fills the chip exactly, so that workgroup only got a slot when the first one retired and the host
        // learned the count ~35 us later than it could -- too late to keep the queue fed at an episode boundary.)
        sum_and_publish<BLK>(pa.carry[0].partials, pa.carry[0].n, nullptr, pa.carry[0].host, pa.carry[0].seq);
        if (pa.carry[1].n > 0) { __syncthreads(); sum_and_publish<BLK>(pa.carry[1].partials, pa.carry[1].n, nullptr, pa.carry[1].host, pa.carry[1].seq); }
    }
    if (ACT) {
        // the learner's actions of this workgroup's 128 tables first (the act window owns the workgroup's whole LDS block; the
        // step's staging reuses it behind the barrier).  Measured: with the step's state loads issued BEFORE the forward -- in
        // flight underneath it -- the kernel needs 256 registers and spills (42.6 us against 22.7 + 15.2 for the two launches).
        pulse_qnet::act_window<true, 128, 5>(*qa, reinterpret_cast<float*>(smem4), (int)blockIdx.x);
        __syncthreads();
    }
    const int gt = blockIdx.x * BLK + threadIdx.x;
    const int t = gt / LPT;
    const int j = gt % LPT;
    if (!ACT && t >= v.n_games) return;   // the lanes of a table leave together (ACT: the host launches whole windows only -- every thread meets the barriers)
    STAMP(0);
    const int P = v.n_players, A = v.active_players;
    const int32_t* __restrict__ hr = v.hand_ranks;
    const uint32_t hr_len = (uint32_t)v.hand_ranks_len;

    // ---- load (every load is independent: all in flight at once).  n_games <= 2^24 (check_view): 24-bit multiplies.
    const uint32_t ut = (uint32_t)t, so = ut * 4u, bo = ut * 20u;      // byte offsets into [N] int32 / board
    int idx = ldo(v.idx, so), button = ldo(v.button, so), pot = ldo(v.pots, so), stage = ldo(v.stages, so), dpos = ldo(v.deck_positions, so);
    int highest = ldo(v.highest, so), agg = ldo(v.agg, so), acted = ldo(v.acted, so), lrs = ldo(v.last_raise_size, so);
    bool done = ldo(v.is_done, ut) != 0;
    bool dirty = ldo(v.equity_dirty, ut) != 0;
    const SeatCells<5> bd_ = ldo(reinterpret_cast<const SeatCells<5>*>(v.board), bo);          // 16 + 4 bytes
    int b0 = bd_.v[0], b1 = bd_.v[1], b2 = bd_.v[2], b3 = bd_.v[3], b4 = bd_.v[4];
    int stack[SPL], bet[SPL], inv[SPL], status[SPL], h0[SPL], h1[SPL];
    float eq[SPL];
    const uint32_t row0 = __umul24(ut, (uint32_t)P), eq0 = __umul24(ut, (uint32_t)A);
    // Seats are dealt to the lanes of a table in blocks: lane j owns seats SPL*j .. SPL*j + SPL-1, i.e. SPL consecutive
    // cells of every [N,P] row -- one 12- or 16-byte load per array instead of SPL dword loads (the prologue is bound by
    // the number of vector-memory instructions a wavefront issues, not by bytes).  The block of a table's last lane runs
    // past the row (P = 10: seats 10, 11 = the next table's first cells: loaded, masked); where it would run past the
    // ARRAY (the last table) the cells are loaded one by one.
#define SEAT(k) (SPL * j + (k))
#define ROW_OFF(k) ((row0 + (uint32_t)SEAT(k)) * 4u)                   /* byte offset of (table, seat) in an [N,P] int32 array */
    const uint32_t cell0 = row0 + (uint32_t)(SPL * j), ecell0 = eq0 + (uint32_t)(SPL * j);     // this lane's first cell
    // (plain 32-bit multiplies: n_games may be 2^24 itself, which a 24-bit multiply truncates to 0)
    const bool vec_ok = cell0 + (uint32_t)SPL <= (uint32_t)v.n_games * (uint32_t)P &&
                        ecell0 + (uint32_t)SPL <= (uint32_t)v.n_games * (uint32_t)A;   // (implies the same for hands and pre_eq)
    // VEC = std::true_type: one vector load; std::false_type: cell by cell.  `limit` = seats that exist in the row.
    auto load_cells = [&](auto VEC, const int32_t* base, uint32_t first_cell, int limit, int (&out)[SPL], int fill) {
        SeatCells<SPL> c;
        if (decltype(VEC)::value) c = ldo(reinterpret_cast<const SeatCells<SPL>*>(base), first_cell * 4u);
        else {
#pragma unroll
            for (int k = 0; k < SPL; ++k) c.v[k] = SEAT(k) < limit ? ldo(base, (first_cell + (uint32_t)k) * 4u) : fill;
        }
#pragma unroll
        for (int k = 0; k < SPL; ++k) out[k] = SEAT(k) < limit ? c.v[k] : fill;
    };
    auto load_hands = [&](auto VEC, int (&o0)[SPL], int (&o1)[SPL]) {
        SeatCells<2 * SPL> c;
        if (decltype(VEC)::value) c = ldo(reinterpret_cast<const SeatCells<2 * SPL>*>(v.hands), cell0 * 8u);
        else {
#pragma unroll
            for (int k = 0; k < SPL; ++k) {
                int2 h = make_int2(-1, -1);
                if (SEAT(k) < P) h = ldo(reinterpret_cast<const int2*>(v.hands), ROW_OFF(k) * 2u);
                c.v[2 * k] = h.x; c.v[2 * k + 1] = h.y;
            }
        }
#pragma unroll
        for (int k = 0; k < SPL; ++k) { o0[k] = SEAT(k) < P ? c.v[2 * k] : -1; o1[k] = SEAT(k) < P ? c.v[2 * k + 1] : -1; }
    };
    const bool cache_on = (PH & (PULSE_PH_EQUITY | PULSE_PH_SHOWDOWN)) && v.pre_board;
    int ph_[SPL], pr_[SPL], e1_[SPL], e2_[SPL], e3_[SPL];            // chunk only: the evaluation cache's rows (staged in LDS below)
    auto load_rows = [&](auto VEC) {
        load_cells(VEC, v.stacks, cell0, P, stack, 0); load_cells(VEC, v.current_round_bet, cell0, P, bet, 0);
        load_cells(VEC, v.total_invested, cell0, P, inv, 0); load_cells(VEC, v.status, cell0, P, status, PULSE_SITOUT);
        int ei[SPL];
        load_cells(VEC, reinterpret_cast<const int32_t*>(v.equities), ecell0, A, ei, 0x3f000000 /* 0.5f */);
#pragma unroll
        for (int k = 0; k < SPL; ++k) eq[k] = __int_as_float(ei[k]);
        load_hands(VEC, h0, h1);          // (a chunk keeps them in LDS: they never change inside an episode)
        if (MULTI) {
#pragma unroll
            for (int k = 0; k < SPL; ++k) { ph_[k] = 0; pr_[k] = 0; e1_[k] = 0; e2_[k] = 0; e3_[k] = 0; }
            if (cache_on) {
                load_cells(VEC, v.pre_hands, cell0, P, ph_, 0); load_cells(VEC, v.pre_rank, cell0, P, pr_, 0);
                const int32_t* pe = reinterpret_cast<const int32_t*>(v.pre_eq);     // [N,3,P]: three rows of P per table
                const uint32_t c0 = __umul24(ut, 3u * (uint32_t)P) + (uint32_t)(SPL * j);     // (ut * 3 leaves 24 bits above 5.59 M tables; 3 P <= 48 does not)
                load_cells(VEC, pe, c0, P, e1_, 0); load_cells(VEC, pe, c0 + (uint32_t)P, P, e2_, 0);
                if (MULTI != 2) load_cells(VEC, pe, c0 + 2u * (uint32_t)P, P, e3_, 0);          // (SLIM: the river row is not read)
            }
        }
    };
    if (vec_ok) load_rows(std::true_type{}); else load_rows(std::false_type{});
    // ---- chunk only: the read-only rows the steps consult (hole cards, the evaluation cache, the next cards of the deck)
    // are staged in the wavefront's LDS slice ONCE.  A global load inside the step loop would have to be waited for
    // with s_waitcnt vmcnt, which counts stores too -- i.e. for every observation / reward / done store of the
    // previous step (the profile showed wavefronts parked there half of their life); LDS reads wait for nothing.
    constexpr int P_ = LPT * SPL;                                       // seats per table as staged (10, 12 or 16)
    const int wave = threadIdx.x >> 6, q = (threadIdx.x & 63) / LPT;     // wavefront of the workgroup, table of the wavefront
    constexpr bool SLIM = MULTI == 2;                                   // chunk for large batches: see chunk_lds_dwords
    constexpr int EQROWS = SLIM ? 2 : 3;
    int32_t* const lw = reinterpret_cast<int32_t*>(smem4) + wave * chunk_lds_dwords(v.obs_size, P_, TPW, SLIM);
    int32_t* const l_hands = lw + TPW * v.obs_size;                      // [TPW][P_][2]
    int32_t* const l_prerank = l_hands + TPW * P_ * 2;                   // [TPW][P_]: 7-card rank (SLIM: its 16 bits | hand class of the seat << 16)
    float* const l_preeq = reinterpret_cast<float*>(l_prerank + TPW * P_);  // [TPW][EQROWS][P_]: flop, turn (and, not SLIM, river) equities
    int32_t* const l_deck = reinterpret_cast<int32_t*>(l_preeq + TPW * EQROWS * P_);  // [TPW][8]: cards at deck position dpos0 + 0..7
    int32_t* const l_class = l_deck + TPW * 8;                            // [TPW][P_] (not SLIM): hand class of every seat (scripted players)
    constexpr int DPL = 8 / LPT;                                         // deck-window entries each lane stages
    const int dpos0 = dpos;
    bool seat_hit[SPL];               // chunk: the cache entry of this lane's seat k was made from the hole cards it holds now
#pragma unroll
    for (int k = 0; k < SPL; ++k) seat_hit[k] = false;
    if (MULTI) {
#pragma unroll
        for (int k = 0; k < SPL; ++k) {
            const int seat = SEAT(k);
            *reinterpret_cast<int2*>(l_hands + (q * P_ + seat) * 2) = make_int2(h0[k], h1[k]);
            seat_hit[k] = PULSE_CACHE_HIT((uint32_t)ph_[k], h0[k], h1[k]);   // hole cards are fixed for the episode
            uint32_t cls = (uint32_t)ph_[k] >> kClsShift;                    // the reset kernel classified the cards the tag names
            if (POLICY && !seat_hit[k]) {          // seats outside the hand hold (-1, -1): a constant; anything else (no cache, poked cards) is classified here
                const bool empty = h0[k] == -1 && h1[k] == -1;
                cls = hand_class(-1, -1);
                if (!empty) cls = hand_class(h0[k], h1[k]);
            }
            if (SLIM) l_prerank[q * P_ + seat] = (int32_t)(((uint32_t)pr_[k] & 0xFFFFu) | cls << 16);      // a valid rank is below 2^16 (PokerGPU.py:13-18)
            else { l_prerank[q * P_ + seat] = pr_[k]; l_class[q * P_ + seat] = (int32_t)cls; }
            l_preeq[(q * EQROWS + 0) * P_ + seat] = __int_as_float(e1_[k]); l_preeq[(q * EQROWS + 1) * P_ + seat] = __int_as_float(e2_[k]);
            if (!SLIM) l_preeq[(q * EQROWS + 2) * P_ + seat] = __int_as_float(e3_[k]);
        }
        const int32_t* dk = v.decks + (size_t)t * 52;
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            const int at = dpos0 + DPL * j + e;
            l_deck[q * 8 + DPL * j + e] = (uint32_t)at < 52u ? dk[at] : 0;
        }
        wave_sync();
    }
    // Paired launch: the host answers the carried counts with this launch's verdict word; thread 0 of the launch relays
    // it from pinned memory into device memory (one poller on PCIe), everybody reads it there before the first step --
    // nothing has been stored yet: if the episode turns out to have ended before this launch, the launch leaves no
    // trace.  (The answer takes the host ~5 us from the launch's start; the load burst above takes the wavefronts longer.)
    bool stop_mid = false;                 // the previous launch's final count ends the episode after this launch's first chunk
    if (MULTI && pa.verdict_dev) {
        // All accesses to the relayed word are RELAXED system-scope atomics: they bypass the (per-XCD, mutually
        // non-coherent) L2s without the cache-wide invalidate / write-back an acquire / release at agent scope costs --
        // 2,048 wavefronts invalidating their L2 in a spin loop tripled the launch time.  The word carries its own
        // launch id, so no other data needs ordering with it.  It is replicated over 64 cache lines (one store
        // instruction of the relaying wavefront); wavefront w polls copy w mod 64.
        if (blockIdx.x == 0 && threadIdx.x < 64) {
            int flags = 0;
            if (threadIdx.x == 0) {
                const long long t0 = wall_clock64();
                for (;;) {
                    const long long w = __hip_atomic_load(pa.verdict_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if ((w >> 8) == pa.verdict_id) { flags = (int)(w & 0xFF); break; }
                    if (wall_clock64() - t0 > pa.verdict_ticks) {                              // too late: run nothing, and tell the host
                        flags = 0x81;
                        if (pa.verdict_err) __hip_atomic_store(pa.verdict_err, pa.verdict_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                    __builtin_amdgcn_s_sleep(16);
                }
            }
            flags = __builtin_amdgcn_readfirstlane(flags);
            __hip_atomic_store(pa.verdict_dev + (threadIdx.x & 63) * kVerdictStride, (pa.verdict_id << 8) | (long long)flags, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
        const long long* mine = pa.verdict_dev + (((blockIdx.x * BLK + threadIdx.x) >> 6) & 63) * kVerdictStride;
        const long long t0 = wall_clock64();
        long long w;
        for (;;) {
            w = __hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((w >> 8) == pa.verdict_id) break;
            if (wall_clock64() - t0 > 2 * pa.verdict_ticks + 100000000ll) { w = 0x81; break; }
            __builtin_amdgcn_s_sleep(32);
        }
        const int flags = __builtin_amdgcn_readfirstlane((int)w);
        if (flags & 1) return;
        stop_mid = (flags & 2) != 0;
    }
    // hole cards of one seat, as every lane of the table may ask: what SEAT_PICK(h0/h1, seat) yields (seat in 0..15)
    auto hand_of_seat = [&](int seat) -> int2 {
        if (seat < P_) return *reinterpret_cast<const int2*>(l_hands + (q * P_ + seat) * 2);
        return make_int2(0, 0);
    };
    // card at deck position `at`: from the staged window.  A hand deals at most 8 positions past its first street, so
    // only a poked state can leave the window; it is then refilled from `at` on -- inside this branch, loads waited for
    // here -- so that the ordinary path holds no global load (and no vmcnt wait at the join) at all.
    int dwin0 = dpos0;
    auto deck_card = [&](int at) -> int {
        if (!MULTI) return (uint32_t)at < 52u ? v.decks[(size_t)t * 52 + at] : 0;
        if ((uint32_t)(at - dwin0) >= 8u) {                         // table-uniform: the table's lanes compute the same `at`
            dwin0 = at;
            const int32_t* dk = v.decks + (size_t)t * 52;
            int c[DPL];
#pragma unroll
            for (int e = 0; e < DPL; ++e) { const int a = at + DPL * j + e; c[e] = (uint32_t)a < 52u ? dk[a] : 0; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
            for (int e = 0; e < DPL; ++e) l_deck[q * 8 + DPL * j + e] = c[e];
            wave_sync();
        }
        return l_deck[q * 8 + (at - dwin0)];
    };
    long long act64 = 0;
    if ((PH & (PULSE_PH_EXECUTE | PULSE_PH_REWARD)) && actions) act64 = ldo(actions, ut * 8u);
    // the Philox draws depend on no load: issue them now, they execute under the load latency.  In a chunk lane j
    // of the table computes call (first + j): LPT calls = 2 * LPT steps of draws in the time of one.
    const uint64_t tid = pa.table_id0 + (uint64_t)t;
    uint64_t pool_base = pa.step_counter >> 1;
    U4 pool{0, 0, 0, 0};
    if (POLICY) pool = philox4x32(pa.seed, tid, pool_base + (MULTI ? (uint64_t)j : 0u));
    const float w1 = *v.w1, w2 = *v.w2;
    const int Kdiv = *v.K, alpha = *v.alpha;
    uint32_t pre_tag = 0;
    if ((PH & (PULSE_PH_EQUITY | PULSE_PH_SHOWDOWN)) && v.pre_board) pre_tag = (uint32_t)ldo(v.pre_board, so);

    // What the launch changes is written back once, after the last step; only changed records are stored (a table's
    // seat rows change in one or two cells per step; writing everything back doubles the store traffic).  A flag is
    // raised wherever a group of words is assigned: bit k of cells_dirty = this lane's seat k (its four row cells),
    // bet_dirty = {pot, highest, agg, acted, last_raise_size, idx}, street_dirty = {stage, deck position, dirty flag},
    // board_dirty = the five board cards.
    // Where dead steps put work off (LIVE_RULE, at the step loop) the word also carries what is owed -- a bool of its own is a
    // lane mask, two more scalar registers across the loop: bit 16 = the table finished on a dead step, its payout and the
    // clearing of its bets are still to come ("unsettled"); bits 17..18 = the stage (1..3) the equity flag was raised at or
    // loaded with, 0 = a flag loaded outside the streets (every equity 0.5).
    constexpr uint32_t kUnsettled = 1u << 16;
    constexpr int kEqStageShift = 17;
    uint32_t cells_dirty = 0;
    bool bet_dirty = false, street_dirty = false, board_dirty = false, eq_dirty = false, act_dirty = false;
    int prev_stack = 0, prev_invested = 0;

    // seat-set bitmask of a per-seat predicate / value of one seat, visible to every lane of the table
#define SEAT_BITS(expr) ([&]() { uint32_t m_ = 0; _Pragma("unroll") for (int k = 0; k < SPL; ++k) m_ |= (uint32_t)((expr) ? 1u : 0u) << SEAT(k); return grp_or<LPT>(m_); }())
#define SEAT_PICK(arr, seat_) ([&]() { uint32_t r_ = 0; _Pragma("unroll") for (int k = 0; k < SPL; ++k) r_ |= SEAT(k) == (seat_) ? (uint32_t)(arr)[k] : 0u; return (int)grp_or<LPT>(r_); }())
    // the actor's equity into e_actor (a macro: the single step expands it where it always stood, a chunk inside the reward of a live step)
#define PICK_E_ACTOR() { uint32_t r_ = 0; _Pragma("unroll") for (int k = 0; k < SPL; ++k) r_ |= SEAT(k) == actor ? __float_as_uint(eq[k]) : 0u; \
                         e_actor = __uint_as_float(grp_or<LPT>(r_)); if (actor >= LPT * SPL) e_actor = 0.5f; }

    STAMP(1);   // loads issued
    // The seat to act, as every lane of the table sees it: status / stack / round bet / hole cards.  Nothing changes
    // between the observation a step writes (for the NEXT seat to act) and the following step's capture, so a chunk
    // carries these five values from one step to the next instead of picking them twice.
    int a_status = 0, a_stack = 0, a_bet = 0, a_h0 = 0, a_h1 = 0;
    uint32_t a_cls = 0;                  // chunk: the hand class of the seat to act instead of its two cards
    auto class_of_seat = [&](int seat) -> uint32_t { return seat < P_ ? (SLIM ? (uint32_t)l_prerank[q * P_ + seat] >> 16 : (uint32_t)l_class[q * P_ + seat]) : hand_class(0, 0); };
    if (MULTI) {
        const int seat0 = idx & 15;
        a_status = SEAT_PICK(status, seat0); a_stack = SEAT_PICK(stack, seat0); a_bet = SEAT_PICK(bet, seat0);
        a_cls = class_of_seat(seat0);
    }
    // the caller's action word was loaded with the state; pin its arrival to the prologue's waits: left pending, its one
    // use after the loop (the final store of the action) became an s_waitcnt vmcnt(0) behind every store of the last step
    if (MULTI) asm volatile("" : "+v"(act64));
    int n_steps = MULTI ? (stop_mid ? pa.mid_step : ca.n_steps) : 1;        // (a long launch cuts it at a check point: long_check_point)
    // output buffers of this step / of the next one: swapped at the end of every step (scalar moves; a select on the
    // step's parity made the compiler keep both sets of per-lane addresses alive across the loop -- and spill them)
    float* obs_dst = v.obs; float* obs_nxt = MULTI ? ca.obs_odd : v.obs;
    uint8_t* done_dst = v.is_done_out; uint8_t* done_nxt = v.is_done;
    float* rew_dst = rewards; float* rew_nxt = MULTI ? ca.rewards_odd : rewards;
    int cp_at = MULTI ? pa.mid_step : 0;          // > 0: the launch covers several check intervals, the first check point is behind step cp_at
    // Live steps.  Step i writes its reward, observation and done flag into buffer set i mod 2, so of a launch that ends
    // after e steps only steps e - 2 and e - 1 leave outputs anybody can read: a dead step computes and stores none of them.
    // A launch can end at n_steps and, a long one, behind its check points (the middle check point of a pair only
    // stores a count: its end is known before the loop, stop_mid) -- end_at is the nearest end the wavefront cannot yet rule
    // out, one scalar compare per step.  The single step and the act + step launch store every step: their predicate is a constant.
    // Which check points a wavefront can rule out (early verdicts, pa.lng.early; off, every check point is a possible end):
    //  - the launch's first, q = 1 (cp_at starts at chunk_steps in every long launch, wherever in the episode the call began):
    //    long_check_point reads a verdict for q >= 2 only, so nothing can end the launch there;
    //  - check point q, 2 <= q < m, once the verdict it will read (that of q - 2, settled by the last arrival at q - 1) is known
    //    to be "go on": the wavefront looks for it at the bottom of step cp_at - 3 -- one load, waited for there behind dead steps
    //    that left no store for the wait to count -- and, where it is settled, moves end_at on to the next check point ("go on")
    //    or cuts n_steps here ("over", "called off").  A pending word changes nothing: the two steps in front of q run live and
    //    q reads the word with its bounded wait, as without the look.  (The look is as late as it can be.  Issued at the top of
    //    that step, its latency hidden under the step, it found the word pending too often -- wavefronts of one launch run
    //    steps apart, and the last arrival at q - 1 is the slowest one's: the headline launch 141 -> 136 us, against 124 us with
    //    the look a step later and its latency exposed.  DESIGN.md section 6.0r8.)
    // The look adds no wait and no decision: every wavefront acts on the one settled word, at the look or at the check point.
    // Which steps run live may differ from wavefront to wavefront and from run to run; what a launch leaves in memory does not.
    constexpr bool LIVE_RULE = MULTI != 0 && !ACT;
    int end_at = n_steps;
    if (LIVE_RULE && pa.lng.n_chunks != 0 && cp_at > 0) end_at = min(pa.lng.early ? cp_at + pa.lng.chunk_steps : cp_at, n_steps);
    if (LIVE_RULE) end_at = __builtin_amdgcn_readfirstlane(end_at);      // wave-uniform, and known to be: the compare below is a scalar one
    // Lazy steps.  A dead step runs the betting state machine and the deal only.  Three phases whose results nothing reads
    // before the next live step wait for it -- divergent phases, which a wavefront pays for whenever one of its tables needs one:
    //  - the equity refresh: eq[] is read by a live step's reward and by the store behind the loop.  It refreshes for the stage
    //    the flag was raised at (carried in cells_dirty); a later transition overwrites that stage, and the refresh it skips wrote
    //    values nobody read.
    //  - the payouts (fold-win, showdown) and the clearing of finished tables: a table that finishes on a dead step is marked
    //    unsettled and paid on the next live step, cleared behind the payout as ever.  Exact because all the payouts read is frozen
    //    once a table is done: no action executes (status, inv, bet, stack), stage and dpos advance for running tables only,
    //    cont_bits is recomputed from status.  A table loaded as done is never unsettled (no payout, as before); its bets are
    //    cleared on the first live step.
    // Invariant: every end e the launch can take (n_steps as called, cut by stop_mid, by a check point or by an early look; a check
    // point of a long launch whose verdict this wavefront does not know to be "go on", whatever the cap's remainder) has steps
    // e - 2 and e - 1 live -- end_at is the NEAREST end the wavefront cannot rule out at every step, and it only moves away at the
    // bottom of step e - 3, before either of them.  A table becomes unsettled, or keeps a raised flag unrefreshed, on a dead step
    // only, and a dead step is followed by a live one before any end; so behind the payout phase of step e - 2 nothing is owed, and what the last step's policy reads
    // (pot, the carried a_*) and what is stored behind the loop (prev_stacks, prev_invested, actions, equities, equity_dirty,
    // the state words) are what eager steps leave.
    if (LIVE_RULE && dirty && stage >= 1 && stage <= 3) cells_dirty |= (uint32_t)stage << kEqStageShift;
    for (int i = 0; i < n_steps; ++i) {
        const bool live = !LIVE_RULE || i + 2 >= end_at;
        // In a chunk, everything derived from the lane's position in its table (seat numbers, `seat < A` masks, ...)
        // is re-derived inside the step: hoisted out of the loop those lane masks filled the scalar registers and were
        // spilled (~200 v_readlane per step to fetch them back); a compare is cheaper than its reload.
        int j = gt % LPT;
        if (MULTI) asm volatile("" : "+v"(j));

        // ---- capture (PokerGPU.py:530-539)
        const bool prev_done = done;
        const int actor = ((PH & PULSE_PH_CAPTURE) || !actor_idx_in ? idx : actor_idx_in[t]) & 15;
        if (!MULTI) {
            a_status = SEAT_PICK(status, actor); a_stack = SEAT_PICK(stack, actor); a_bet = SEAT_PICK(bet, actor);
            if (POLICY) { a_h0 = SEAT_PICK(h0, idx & 15); a_h1 = SEAT_PICK(h1, idx & 15); }
        }
        const bool has_legal_actor = a_status != PULSE_FOLDED && a_status != PULSE_ALLIN && a_status != PULSE_SITOUT && !prev_done;
        prev_invested = a_bet;
        if (!(PH & PULSE_PH_CAPTURE)) prev_invested = ldo(v.prev_invested, so);
        prev_stack = a_stack;

        STAMP(2);   // first loads have arrived (actor values picked)
        // ---- scripted opponents (environments/Poker/utils.py:108-123), fused in front of the step
        if (POLICY) {
            const uint64_t step = pa.step_counter + (uint64_t)i;
            PolicyDraw draw;
            if (MULTI) {
                const uint64_t call = step >> 1;
                if (call - pool_base >= (uint64_t)LPT) {              // wave-uniform: the pool of four calls is used up
                    pool_base = call;
                    pool = philox4x32(pa.seed, tid, call + (uint64_t)j);
                }
                const int rel = (int)(call - pool_base);
                const PolicyDraw mine = policy_draw(pool, step);
                draw.pick = grp_or<LPT>(j == rel ? mine.pick : 0u);
                draw.coin = grp_or<LPT>(j == rel ? mine.coin : 0u);
            } else {
                draw = policy_draw(pool, step);
            }
            const int type = (int)((pa.types_packed >> (4 * (idx & 15))) & 15u);
            if (type != PULSE_AGENT_EXTERNAL) {
                act64 = MULTI ? scripted_action_cls(type, a_cls, pot, draw) : scripted_action(type, a_h0, a_h1, pot, draw);
                act_dirty = true;                  // stored once, after the last step (a later step's action overwrites it anyway)
            }
        }
        const int action = act64 < -1 ? -1 : (act64 > 13 ? 13 : (int)act64);   // masks only test ==0, ==1, >=2, 2, 3..11, 12

        STAMP(3);   // policy done
        // ---- 1) equities of dirty tables (PokerGPU.py:455-525)
        if (PH & PULSE_PH_EQUITY) {
            if (live && dirty) {
                // the stage the refresh is FOR: where dead steps put it off, the one the flag was raised at or loaded with (0: no
                // street) -- a table whose river was dealt on a dead step has usually finished (stage 4) by the next live one
                const int rs = LIVE_RULE ? (int)(cells_dirty >> kEqStageShift) & 3 : stage;
                const int c5 = rs >= 2 ? b3 : 0, c6 = rs == 3 ? b4 : 0;
                const bool street = rs >= 1 && rs <= 3;
                const bool cached_board = street && board_matches(pre_tag, rs + 2, b0, b1, b2, b3, b4);
#pragma unroll
                for (int k = 0; k < SPL; ++k) {
                    const int seat = SEAT(k);
                    float e = 0.5f;
                    if (seat < A && street) {
                        bool hit = false;
                        if (cached_board) {       // the cache reads are independent single hops
                            if (MULTI) {
                                hit = seat_hit[k];
                                if (SLIM && rs == 3) {      // the river's equity is the 7-card rank normalised (PokerGPU.py:481), as the reset kernel stored it
                                    e = __fdiv_rn(__fsub_rn((float)(l_prerank[q * P_ + seat] & 0xFFFF), 4109.0f), 32765.0f);
                                    e = fminf(fmaxf(e, 0.0f), 1.0f);
                                } else e = l_preeq[(q * EQROWS + (rs - 1)) * P_ + seat];
                            } else {
                                const uint32_t ph = (uint32_t)ldo(v.pre_hands, ROW_OFF(k));
                                const float pe = ldo(v.pre_eq, (__umul24(ut, 3u * (uint32_t)P) + __umul24((uint32_t)(rs - 1), (uint32_t)P) + (uint32_t)seat) * 4u);
                                hit = PULSE_CACHE_HIT(ph, h0[k], h1[k]);
                                e = pe;
                            }
                        }
                        if (!hit) {               // the reference's literal seven-gather chain
                            int hc0 = h0[k], hc1 = h1[k];
                            if (MULTI) { const int2 h = hand_of_seat(seat); hc0 = h.x; hc1 = h.y; }
                            const float r = (float)walk7(hr, hr_len, hc0, hc1, b0, b1, b2, c5, c6);
                            e = rs == 1 ? __fdiv_rn(__fsub_rn(r, 74359.0f), 749420.0f) : __fdiv_rn(__fsub_rn(r, 4109.0f), 32765.0f);
                            e = fminf(fmaxf(e, 0.0f), 1.0f);
                        }
                    }
                    eq[k] = e;
                }
                dirty = false; street_dirty = true; eq_dirty = true;
            }
        }
        // the actor's equity: only the reward reads it, and nothing between here and there changes eq[] -- where dead steps
        // skip the reward it is picked there
        float e_actor;
        if (!LIVE_RULE) PICK_E_ACTOR();

        STAMP(4);   // equities done
        // ---- 2) execute the action of the seat to act (PokerGPU.py:230-303)
        if (PH & PULSE_PH_EXECUTE) {
            const int call_cost = highest - a_bet;
            const bool active = a_status != PULSE_FOLDED && a_status != PULSE_ALLIN && a_status != PULSE_SITOUT && !done;
            if (active && action >= 0) {
                int n_stack = a_stack, n_bet = a_bet, n_inv_add = 0, n_status = a_status;
                if (action == 0) {
                    n_status = PULSE_FOLDED;
                } else {
                    int raise_amt = 0;
                    if (action == 2) raise_amt = lrs;
                    else if (action == 12) raise_amt = a_stack;
                    else if (action >= 3 && action <= 11) {
                        const float fr = action == 3 ? 0.25f : action == 4 ? 0.33f : action == 5 ? 0.50f : action == 6 ? 0.75f
                                       : action == 7 ? 1.00f : action == 8 ? 1.50f : action == 9 ? 2.00f : action == 10 ? 3.00f : 4.00f;
                        raise_amt = (int)__fmul_rn((float)pot, fr);
                    }
                    const int total = action == 1 ? call_cost : call_cost + raise_amt;
                    const int amt = min(total, a_stack);
                    const bool is_raise = action >= 2 && amt > call_cost;
                    n_stack = a_stack - amt; n_bet = a_bet + amt; n_inv_add = amt; pot += amt;
                    if (n_stack == 0) n_status = PULSE_ALLIN;
                    if (is_raise) {
                        const int raise_size = n_bet - highest;
                        highest = n_bet;
                        if (raise_size >= lrs) { agg = idx; acted = 0; lrs = raise_size; }
                    }
                }
                acted += 1;
                bet_dirty = true;
#pragma unroll
                for (int k = 0; k < SPL; ++k)
                    if (SEAT(k) == (idx & 15)) { stack[k] = n_stack; bet[k] = n_bet; inv[k] += n_inv_add; status[k] = n_status; cells_dirty |= 1u << k; }
            }
        }

        const uint32_t act_bits = SEAT_BITS(status[k] == PULSE_ACTIVE);
        const uint32_t cont_bits = SEAT_BITS(status[k] == PULSE_ACTIVE || status[k] == PULSE_ALLIN);
        const int contenders = __popc(cont_bits);

        STAMP(5);   // action executed, seat masks built
        // ---- 3) next actor, round close, street transition (PokerGPU.py:547-616)
        if (PH & PULSE_PH_ADVANCE) {
            const int truly_active = __popc(act_bits);
            const bool all_acted = acted >= truly_active;
            bool round_over = done || truly_active == 0;
            const uint32_t maskA = (1u << A) - 1u;
            const int next_seat = first_after_near(act_bits & maskA, idx, A);
            const bool has_next = next_seat >= 0;
            const bool closes = all_acted && (idx == agg || (has_next && next_seat == agg));
            round_over = round_over || !has_next || closes;
            if (!round_over && has_next) { idx = next_seat; bet_dirty = true; }
            const bool early_term = contenders <= 1 && round_over;
            if (early_term) done = true;
            if (round_over && !early_term && !done) {
                lrs = 1; stage += 1; highest = 0; agg = mod_near(button + 1, A); acted = 0;
                bet_dirty = true; street_dirty = true;
#pragma unroll
                for (int k = 0; k < SPL; ++k) { cells_dirty |= (bet[k] != 0 ? 1u : 0u) << k; bet[k] = 0; }
                const int first = first_after_near(act_bits & maskA, button, A);
                if (first >= 0) idx = first;
                if (stage > 3) { done = true; stage = 4; }
                else {
                    const int nx0 = deck_card(dpos + 1);
                    if (stage == 1) {                                                // burn + flop (:601-604)
                        b0 = nx0;
                        b1 = deck_card(dpos + 2);
                        b2 = deck_card(dpos + 3);
                        dpos += 4;
                    }
                    else if (stage == 2) { b3 = nx0; dpos += 2; }                    // burn + turn (:607-610)
                    else { b4 = nx0; dpos += 2; }                                    // burn + river (:613-616)
                    dirty = true; board_dirty = true;
                    if (LIVE_RULE) cells_dirty = (cells_dirty & ~(3u << kEqStageShift)) | (uint32_t)stage << kEqStageShift;
                }
            }
        }
        // a chunk fetches the next actor's hole cards now; they are first needed by the observation below (of a live step: the
        // hand class is carried on every step)
        int2 next_hand = make_int2(0, 0);
        uint32_t next_cls = 0;
        if (MULTI) { if (live) next_hand = hand_of_seat(idx & 15); next_cls = class_of_seat(idx & 15); }

        STAMP(6);   // advance / deal done
        // ---- 4) payouts on newly finished tables (PokerGPU.py:619-623)
        bool newly_done = (PH & PULSE_PH_CAPTURE) ? (done && !prev_done) : done;
        if (LIVE_RULE) {               // a dead step leaves the table unsettled; a live one pays what is owed, this step's finish included
            cells_dirty |= newly_done ? kUnsettled : 0u;
            newly_done = live && (cells_dirty & kUnsettled) != 0;
            if (live) cells_dirty &= ~kUnsettled;
        }
        if ((PH & PULSE_PH_FOLDWIN) && live) {                                         // :331-338
            if (newly_done && contenders == 1) {
                const int survivor = __ffs((int)cont_bits) - 1;
#pragma unroll
                for (int k = 0; k < SPL; ++k) if (SEAT(k) == survivor) { stack[k] += pot; cells_dirty |= 1u << k; }
                pot = 0; bet_dirty = true;
            }
        }
        if ((PH & PULSE_PH_SHOWDOWN) && live) {                                 // :380-453
            if (newly_done && stage < 5 && contenders > 1) {
                if (stage == 0) {
                    b0 = deck_card(dpos + 1); b1 = deck_card(dpos + 2); b2 = deck_card(dpos + 3);
                    b3 = deck_card(dpos + 5); b4 = deck_card(dpos + 7);
                    dpos += 8;
                } else if (stage == 1) {
                    b3 = deck_card(dpos + 1); b4 = deck_card(dpos + 3);
                    dpos += 4;
                } else if (stage == 2) {
                    b4 = deck_card(dpos + 1);
                    dpos += 2;
                }
                bool eligible[SPL]; int rank[SPL], payout[SPL];
                const bool cached_board = board_matches(pre_tag, 5, b0, b1, b2, b3, b4);
#pragma unroll
                for (int k = 0; k < SPL; ++k) {
                    const int seat = SEAT(k);
                    eligible[k] = seat < A && (status[k] == PULSE_ACTIVE || status[k] == PULSE_ALLIN);
                    rank[k] = INT_MIN; payout[k] = 0;
                    if (eligible[k]) {
                        bool hit = false;
                        if (cached_board) {
                            if (MULTI) {
                                hit = seat_hit[k];
                                rank[k] = SLIM ? l_prerank[q * P_ + seat] & 0xFFFF : l_prerank[q * P_ + seat];
                            } else {
                                const uint32_t ph = (uint32_t)ldo(v.pre_hands, ROW_OFF(k));
                                hit = PULSE_CACHE_HIT(ph, h0[k], h1[k]);
                                rank[k] = ldo(v.pre_rank, ROW_OFF(k));
                            }
                        }
                        if (!hit) {
                            int hc0 = h0[k], hc1 = h1[k];
                            if (MULTI) { const int2 h = hand_of_seat(seat); hc0 = h.x; hc1 = h.y; }
                            rank[k] = walk7(hr, hr_len, hc0, hc1, b0, b1, b2, b3, b4);
                            asm volatile("" : "+v"(rank[k]));      // the chain's last load is waited for HERE, not at the join every table passes
                        }
                    }
                }
                // side pots, one layer per distinct commitment level (PokerGPU.py:340-378)
                int prev_level = 0;
                for (int l = 0; l < A; ++l) {
                    int lv = INT_MAX;
#pragma unroll
                    for (int k = 0; k < SPL; ++k) if (SEAT(k) < A && inv[k] > prev_level) lv = min(lv, inv[k]);
                    const int level = grp_imin<LPT>(lv);
                    if (level == INT_MAX) break;
                    const int n_contrib = __popc(SEAT_BITS(SEAT(k) < A && inv[k] >= level));
                    int bl = INT_MIN;
#pragma unroll
                    for (int k = 0; k < SPL; ++k) if (SEAT(k) < A && inv[k] >= level && eligible[k]) bl = max(bl, rank[k]);
                    const int best = grp_imax<LPT>(bl);
                    const uint32_t win_bits = SEAT_BITS(SEAT(k) < A && inv[k] >= level && eligible[k] && rank[k] == best);
                    const int n_win = __popc(win_bits);
                    if (n_win > 0) {
                        const int layer_pot = (level - prev_level) * n_contrib;
                        const int share = layer_pot / n_win, rem = layer_pot - share * n_win;
                        const int first_win = __ffs((int)win_bits) - 1;
#pragma unroll
                        for (int k = 0; k < SPL; ++k)
                            if ((win_bits >> SEAT(k)) & 1u) payout[k] += share + (SEAT(k) == first_win ? rem : 0);
                    }
                    prev_level = level;
                }
#pragma unroll
                for (int k = 0; k < SPL; ++k) { stack[k] += payout[k]; cells_dirty |= (payout[k] != 0 ? 1u : 0u) << k; }
                pot = 0; stage = 5;
                bet_dirty = true; street_dirty = true; board_dirty = true;
            }
        }
        if ((PH & PULSE_PH_CLEARDONE) && live) {                                // :625-628 (idempotent: a dead step leaves it to the next live one)
            if (done) {
                bet_dirty = bet_dirty || highest != 0;
                highest = 0;
#pragma unroll
                for (int k = 0; k < SPL; ++k) { cells_dirty |= ((bet[k] | inv[k]) != 0 ? 1u : 0u) << k; bet[k] = 0; inv[k] = 0; }
            }
        }

        STAMP(7);   // payouts done
        // ---- 5) shaped reward (PokerGPU.py:305-329, :631-632)
        if ((PH & PULSE_PH_REWARD) && live) {
            if (LIVE_RULE) PICK_E_ACTOR();
            const float cnt = (float)contenders;
            const float fair = __fdiv_rn(1.0f, fmaxf(cnt, 1.0f));
            const int cc = max(0, highest - prev_invested);
            const float potf = (float)pot;
            const float m = __fmul_rn(e_actor, potf);
            const float o = __fdiv_rn((float)cc, __fadd_rn((float)(pot + cc), 1e-6f));
            float sv = 0.0f;
            if (action == 1) sv = __fmul_rn(__fsub_rn(e_actor, o), potf);
            else if (action == 0) sv = __fmul_rn(__fsub_rn(o, e_actor), potf);
            else if (action >= 2) sv = __fmul_rn(__fsub_rn(e_actor, fair), potf);
            const float x = __fdiv_rn(__fadd_rn(__fmul_rn(w1, m), __fmul_rn(w2, sv)), (float)Kdiv);
            float r = __fmul_rn((float)alpha, tanh_rn(x));
            if ((PH & PULSE_PH_CAPTURE) && (!has_legal_actor || prev_done)) r = 0.0f;
            if (j == 0) sto_in_loop(rew_dst, so, r);
        }

        STAMP(8);   // reward done
        // ---- 6) observation for the next seat to act (PokerGPU.py:159-179)
        if (PH & PULSE_PH_OBS) {
            const int wlane = threadIdx.x & 63;
            float* const l_obs = MULTI ? reinterpret_cast<float*>(lw) : reinterpret_cast<float*>(smem4) + (threadIdx.x >> 6) * TPW * v.obs_size;
            float* __restrict__ o = WOBS ? l_obs + q * v.obs_size
                                         : reinterpret_cast<float*>(reinterpret_cast<char*>(obs_dst) + __umul24(ut, (uint32_t)v.obs_size) * 4u);
            const int seat_i = idx & 15;
            const int n_h0 = MULTI ? next_hand.x : SEAT_PICK(h0, seat_i), n_h1 = MULTI ? next_hand.y : SEAT_PICK(h1, seat_i);
            const int n_stack = SEAT_PICK(stack, seat_i), n_status = SEAT_PICK(status, seat_i), n_bet = SEAT_PICK(bet, seat_i);
            if (MULTI) { a_status = n_status; a_stack = n_stack; a_bet = n_bet; a_cls = next_cls; }   // the next step's actor: carried on every step, live or not
            if (live) {
                const int idxm = mod_near(idx, A);
                const int pos = mod_near(idx - button, A);
                // columns 0..12, LPT per pass: lane j writes column LPT*pass + j (an LPT-way select per pass)
                if (LPT == 4) {
                    const int h0v = j == 0 ? b0 : j == 1 ? b1 : j == 2 ? b2 : b3;
                    const int h1v = j == 0 ? b4 : j == 1 ? n_h0 : j == 2 ? n_h1 : stage;
                    const int h2v = j == 0 ? pos : j == 1 ? pot : j == 2 ? highest - n_bet : n_stack;
                    o[j] = (float)h0v; o[4 + j] = (float)h1v; o[8 + j] = (float)h2v;
                    if (j == 0) o[12] = (float)n_status;
                } else {
                    o[j] = (float)(j == 0 ? b0 : b1); o[2 + j] = (float)(j == 0 ? b2 : b3); o[4 + j] = (float)(j == 0 ? b4 : n_h0);
                    o[6 + j] = (float)(j == 0 ? n_h1 : stage); o[8 + j] = (float)(j == 0 ? pos : pot);
                    o[10 + j] = (float)(j == 0 ? highest - n_bet : n_stack);
                    if (j == 0) o[12] = (float)n_status;
                }
                // opponents: seat (idx+1+k)%A -> columns 13+3k..; seats >= A zero-fill the padding slots
#pragma unroll
                for (int k = 0; k < SPL; ++k) {
                    const int seat = SEAT(k);
                    if (seat < v.max_players && seat != idxm) {
                        int slot; float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
                        if (seat < A) { slot = seat - idxm - 1; if (slot < 0) slot += A; f0 = (float)stack[k]; f1 = (float)status[k]; f2 = (float)bet[k]; }
                        else slot = seat - 1;
                        float* dst = o + 13 + 3 * slot;
                        dst[0] = f0; dst[1] = f1; dst[2] = f2;
                    }
                }
                if (WOBS) {
                    wave_sync();
                    const int n4 = TPW / 4 * v.obs_size;                             // int4 per wavefront block
                    const int tw0 = (int)((blockIdx.x * BLK + threadIdx.x) >> 6) * TPW;  // first table of this wavefront
                    const uint32_t blk0 = __umul24((uint32_t)tw0, (uint32_t)v.obs_size) * 4u;      // byte offset of the wavefront's block
                    const int4* src = reinterpret_cast<const int4*>(l_obs);
                    constexpr int kBursts = 5;          // two-lane chunk, 40 columns: 32 rows x 160 B = five 1-KiB bursts
                    if (n4 == kBursts * 64) {
                        // all reads first, then all stores: as a loop over e every pass waited for its own LDS read
                        // (five exposed LDS latencies per step)
                        int4 x[kBursts];
#pragma unroll
                        for (int u = 0; u < kBursts; ++u) x[u] = src[wlane + 64 * u];
#pragma unroll
                        for (int u = 0; u < kBursts; ++u) sto_in_loop(reinterpret_cast<int4*>(obs_dst), blk0 + (uint32_t)(wlane + 64 * u) * 16u, x[u]);
                    } else
                        for (int e = wlane; e < n4; e += 64) sto_in_loop(reinterpret_cast<int4*>(obs_dst), blk0 + (uint32_t)e * 16u, src[e]);
                    if (MULTI) {       // the next step's values must not overtake these reads of the slice
                        wave_sync();
                    }
                }
            }
        }
        STAMP(9);   // observation stores issued
        if ((PH & PULSE_PH_ADVANCE) && live && j == 0) sto_in_loop(done_dst, ut, (uint8_t)(done ? 1 : 0));      // ping-pong buffer: written by every live step
        // the early look at the verdict the coming check point will read.  (Not in the slim image: it is taken above 81,920 tables,
        // where no long launch passes the residency gate, and the pairs it runs there paid 1.2 % for the look's mere presence.
        // A long launch forced onto it looks at nothing and reads every verdict at its check point.)
        if (LIVE_RULE && !SLIM && i + 3 == cp_at) {
            StepKernargsPtr ka = (StepKernargsPtr)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka));
            const int early = ka->pa.lng.early;
            if (early != 0 && cp_at > ka->pa.mid_step && cp_at < ka->ca.n_steps) {      // a long launch's check point q, 2 <= q < m
                const int cs = ka->pa.lng.chunk_steps;
                const int taken = long_peek(ka, cp_at / cs - 2, (uint32_t)(blockIdx.x * (BLK / 64) + (threadIdx.x >> 6)), early);
                if (taken == 2) n_steps = cp_at;                                                        // end_at == cp_at already
                if (taken == 1) end_at = __builtin_amdgcn_readfirstlane(min(cp_at + cs, n_steps));
            }
        }
        if (MULTI && i + 1 == cp_at) {        // the check point in the middle of a paired launch / a check point of a long one
            StepKernargsPtr ka = (StepKernargsPtr)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka));
            const int c = __popcll(__ballot(done && j == 0));
            const uint32_t wid = (uint32_t)(blockIdx.x * (BLK / 64) + (threadIdx.x >> 6));
            if (ka->pa.lng.n_chunks == 0) {
                if ((threadIdx.x & 63) == 0) stg(ka->pa.wave_done_mid, wid * 4u, (uint32_t)c);
            } else {
                const int cs = ka->pa.lng.chunk_steps;
#if PULSE_STAMPS
                const long long cp_t0 = clock64();
#endif
                // (what an early look took: it moved end_at past this check point, or cut n_steps to it -- a launch's last check
                // point, where n_steps is cp_at as called, reads no verdict)
                const int taken = !LIVE_RULE ? 0 : end_at > cp_at ? 1 : n_steps == cp_at ? 2 : 0;
                if (long_check_point(ka, cp_at / cs, c, wid, !stop_mid, taken)) n_steps = i + 1;
#if PULSE_STAMPS
                if ((threadIdx.x & 63) == 0 && g_stamp_buf) {       // slots 12..14: ticks inside the check points, their number, the longest one
                    const long long dt = clock64() - cp_t0;
                    unsigned long long* s = g_stamp_buf + (size_t)wid * 16;
                    s[12] += (unsigned long long)dt; s[13] += 1; if ((unsigned long long)dt > s[14]) s[14] = (unsigned long long)dt;
                }
#endif
                cp_at += cs;
                if (LIVE_RULE) end_at = __builtin_amdgcn_readfirstlane(min(cp_at, n_steps));
            }
        }
        if (MULTI) {
            float* fo = obs_dst; obs_dst = obs_nxt; obs_nxt = fo;
            uint8_t* fd = done_dst; done_dst = done_nxt; done_nxt = fd;
            float* fr = rew_dst; rew_dst = rew_nxt; rew_nxt = fr;
        }
    }

    // ---- store: the groups whose flag was raised (one test per seat / per group instead of one branch per word).
    // In a chunk the ~25 state pointers would have to stay in scalar registers across the whole step loop (they were
    // spilled, 95 of them); the kernel argument block is re-read here through a pointer the compiler cannot see through.
    // The pointer stays in the constant address space (scalar loads of the array pointers, lgkmcnt only -- as a generic
    // pointer they became vector loads waited for with vmcnt(0), i.e. behind every store in flight), and the stores go
    // out as global stores (stg).
    StepKernargsPtr ka = (StepKernargsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    if (MULTI) asm volatile("" : "+s"(ka));
#define VS(field) (MULTI ? ka->v.field : v.field)
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const int seat = SEAT(k);
        if (seat < P && ((cells_dirty >> k) & 1u)) {
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_FOLDWIN | PULSE_PH_SHOWDOWN)) stg(VS(stacks), ROW_OFF(k), stack[k]);
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_ADVANCE | PULSE_PH_CLEARDONE)) stg(VS(current_round_bet), ROW_OFF(k), bet[k]);
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_CLEARDONE)) stg(VS(total_invested), ROW_OFF(k), inv[k]);
            if (PH & PULSE_PH_EXECUTE) stg(VS(status), ROW_OFF(k), status[k]);
        }
    }
    if ((PH & PULSE_PH_EQUITY) && eq_dirty) {          // the equities as the last step that recomputed them left them (PokerGPU.py:455-525)
#pragma unroll
        for (int k = 0; k < SPL; ++k) if (SEAT(k) < A) stg(VS(equities), (eq0 + (uint32_t)SEAT(k)) * 4u, eq[k]);
    }
    if (POLICY && act_dirty && j == 0) stg(MULTI ? ka->actions : actions, ut * 8u, (int64_t)act64);
    if (PH & (PULSE_PH_ADVANCE | PULSE_PH_SHOWDOWN)) {
        if (board_dirty) {
            static_assert(LPT == 4 || LPT == 2, "board store");
            if (LPT == 4) {
                stg(VS(board), bo + (uint32_t)j * 4u, j == 0 ? b0 : j == 1 ? b1 : j == 2 ? b2 : b3);
                if (j == 0) stg(VS(board), bo + 16u, b4);
            } else {
                stg(VS(board), bo + (uint32_t)j * 4u, j == 0 ? b0 : b1);
                stg(VS(board), bo + 8u + (uint32_t)j * 4u, j == 0 ? b2 : b3);
                if (j == 0) stg(VS(board), bo + 16u, b4);
            }
        }
    }
    if (j == 0) {
        if (PH & PULSE_PH_CAPTURE) { stg(VS(prev_stacks), so, prev_stack); stg(VS(prev_invested), so, prev_invested); }
        if (bet_dirty) {
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_FOLDWIN | PULSE_PH_SHOWDOWN)) stg(VS(pots), so, pot);
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_ADVANCE | PULSE_PH_CLEARDONE)) stg(VS(highest), so, highest);
            if (PH & (PULSE_PH_EXECUTE | PULSE_PH_ADVANCE)) { stg(VS(agg), so, agg); stg(VS(acted), so, acted); stg(VS(last_raise_size), so, lrs); }
            if (PH & PULSE_PH_ADVANCE) stg(VS(idx), so, idx);
        }
        if (street_dirty) {
            if (PH & (PULSE_PH_ADVANCE | PULSE_PH_SHOWDOWN)) { stg(VS(stages), so, stage); stg(VS(deck_positions), so, dpos); }
            if (PH & (PULSE_PH_EQUITY | PULSE_PH_ADVANCE)) stg(VS(equity_dirty), ut, (uint8_t)(dirty ? 1 : 0));
        }
    }
    if (POLICY && pa.wave_done) {
        // the roll-out's stop rule (trainGPU.py:27-33) rides on the launch: every wavefront stores how many of its
        // tables are done -- a plain store, summed on a side stream (atomics onto shared counters cost this launch
        // as much as the separate counting kernel they would replace)
        const int c = __popcll(__ballot(done && j == 0));
        if ((threadIdx.x & 63) == 0) pa.wave_done[blockIdx.x * (BLK / 64) + (threadIdx.x >> 6)] = (uint32_t)c;
    }
    STAMP(10);  // state stores issued
#if PULSE_STAMPS
    __builtin_amdgcn_s_waitcnt(0);                      // vmcnt(0): all stores acknowledged
    STAMP(11);
#endif
#undef SEAT_BITS
#undef SEAT_PICK
#undef PICK_E_ACTOR
#undef ROW_OFF
#undef SEAT
#undef VS
}

// (two lanes per table -- chunks only: three wavefronts per SIMD, the 168 VGPRs the residency of the long launches counts on.  With
// two asked for, the lazy steps' bookkeeping came out at 169 / 170 by the compiler's choice alone.)
template <uint32_t PH, bool POLICY, int LPT, int SPL, bool WOBS, int MULTI>
__global__ __launch_bounds__(kStepBlock, LPT == 4 ? 4 : 3) void poker_step_kernel(const PulsePokerView v, int64_t* __restrict__ actions,
                                                           const int32_t* __restrict__ actor_idx_in,
                                                           float* __restrict__ rewards, const PolicyArgs pa, const ChunkArgs ca) {
    poker_step_body<PH, POLICY, LPT, SPL, WOBS, MULTI, false>(v, actions, actor_idx_in, rewards, pa, ca, nullptr);
}

// the learner's action selection + scripted opponents + env step of 128 tables per workgroup (the body's ACT form); the
// leading arguments are the step kernel's (the body re-reads some of them from the kernel-argument segment by position)
template <bool WOBS>
__global__ __launch_bounds__(256, 2) void poker_act_step_kernel(const PulsePokerView v, int64_t* __restrict__ actions,
                                                                const int32_t* __restrict__ actor_idx_in, float* __restrict__ rewards,
                                                                const PolicyArgs pa, const ChunkArgs ca, const pulse_qnet::QNetArgs qa) {
    poker_step_body<PULSE_PH_STEP, true, 2, 5, WOBS, 1, true>(v, actions, actor_idx_in, rewards, pa, ca, &qa);
}

}  // namespace

// ---------------------------------------------------------------- host side
// Lanes per table.  Single-step launches: four.  Chunk launches: two where a lane can hold the table's seats in five
// (max_players <= 10; PULSE_VIEW_FOUR_LANES asks for four), four otherwise.  Two lanes per table replicate the table's
// scalar state machine half as often and issue half the wavefronts; measured per 5-step chunk (4 vs 2 lanes) at
// 65,536 / 262,144 / 1,048,576 tables: 39.6 / 112.4 / 404 us vs 37.3 / 114.9 / 395 us.  (With this round's first chunk
// kernel -- per-seat dword loads, library tanh, policy recomputed from the cards every step -- two lanes lost at every
// size, 46.9 vs 43.6 us and 553 vs 463 us: what it saves is exactly the replicated table-level work those changes cut.
// Tables of 12 / 16 seats at six / eight seats per lane were measured too and lose: 42.7 vs 42.5 and 72.6 vs 59.2 us at
// 65,536 tables, 277 vs 233 and 391 vs 317 us at 524,288 -- registers (168 / 187) and LDS per wavefront grow with the seats.)
int pulse::lanes_for(const PulsePokerView& v, bool chunk) { return chunk && v.max_players <= 10 && !(v.flags & PULSE_VIEW_FOUR_LANES) ? 2 : 4; }

namespace {

inline dim3 step_grid(const PulsePokerView& v, int lpt) { return dim3((unsigned)(((long long)v.n_games * lpt + kStepBlock - 1) / kStepBlock)); }
inline bool obs_staging(const PulsePokerView& v, const float* obs_odd, int lpt) {
    return !(v.flags & PULSE_VIEW_NO_OBS_STAGING) && (v.n_games % (64 / lpt)) == 0 && ((uintptr_t)v.obs & 15u) == 0 && ((uintptr_t)obs_odd & 15u) == 0;
}

template <uint32_t PH, bool POLICY, int LPT, int SPL, int MULTI>
void launch_one(const PulsePokerView& v, int64_t* actions, const int32_t* actor_idx, float* rewards, const PolicyArgs& pa, const ChunkArgs& ca,
                hipStream_t st) {
    constexpr int TPW = 64 / LPT;
    const bool wobs = (PH & PULSE_PH_OBS) && (MULTI || PH == PULSE_PH_STEP) && obs_staging(v, MULTI ? ca.obs_odd : nullptr, LPT);
    const size_t lds = MULTI ? sizeof(int32_t) * (size_t)(kStepBlock / 64) * (size_t)chunk_lds_dwords(v.obs_size, LPT * SPL, TPW, MULTI == 2)
                             : (wobs ? sizeof(float) * (size_t)(kStepBlock / 64) * TPW * (size_t)v.obs_size : 0);
    constexpr bool W = PH == PULSE_PH_STEP;          // only the full step is instantiated with observation staging
    const auto fn = wobs ? &poker_step_kernel<PH, POLICY, LPT, SPL, W, MULTI> : &poker_step_kernel<PH, POLICY, LPT, SPL, false, MULTI>;
    // after a refusal to raise the LDS limit the launch is tried all the same, and it is the launch that reports (finish_launch)
    pulse::launch_lds(fn, step_grid(v, LPT).x, kStepBlock, lds, st, true, v, actions, actor_idx, rewards, pa, ca);
}

// the occupancy query for exactly the instantiation and LDS size launch_one takes
template <uint32_t PH, bool POLICY, int LPT, int SPL, int MULTI>
int resident_one(const PulsePokerView& v, const float* obs_odd) {
    constexpr int TPW = 64 / LPT;
    const bool wobs = obs_staging(v, obs_odd, LPT);
    const size_t lds = sizeof(int32_t) * (size_t)(kStepBlock / 64) * (size_t)chunk_lds_dwords(v.obs_size, LPT * SPL, TPW, MULTI == 2);
    const auto fn = wobs ? &poker_step_kernel<PH, POLICY, LPT, SPL, true, MULTI> : &poker_step_kernel<PH, POLICY, LPT, SPL, false, MULTI>;
    return pulse::resident_blocks_per_cu(reinterpret_cast<const void*>(fn), kStepBlock, lds);
}

inline bool chunk_slim(const PulsePokerView& v) { return v.n_games > 81920; }     // the two-lane chunk's slim LDS image (launch_chunk)

template <uint32_t PH, bool POLICY, int MULTI>
void launch_any(const PulsePokerView& v, int64_t* actions, const int32_t* actor_idx, float* rewards, const PolicyArgs& pa, const ChunkArgs& ca,
                hipStream_t st) {
    // seats per lane must cover max_players (the observation's padding slots too)
    if (v.max_players <= 12) launch_one<PH, POLICY, 4, 3, MULTI>(v, actions, actor_idx, rewards, pa, ca, st);
    else launch_one<PH, POLICY, 4, 4, MULTI>(v, actions, actor_idx, rewards, pa, ca, st);
}

template <uint32_t PH>
void launch_phase(const PulsePokerView& v, int64_t* actions, const int32_t* actor_idx, float* rewards, hipStream_t st) {
    launch_any<PH, false, 0>(v, actions, actor_idx, rewards, PolicyArgs{}, ChunkArgs{}, st);
}

}  // namespace

void pulse::launch_policy_step(const PulsePokerView& v, int64_t* actions, float* rewards, const PolicyArgs& pa, hipStream_t st) {
    launch_any<PULSE_PH_STEP, true, 0>(v, actions, nullptr, rewards, pa, ChunkArgs{}, st);
}

void pulse::launch_chunk(const PulsePokerView& v, int64_t* actions, float* rewards_even, const PolicyArgs& pa, const ChunkArgs& ca, hipStream_t st) {
    if (lanes_for(v, true) == 2) {
        // The full LDS image lets 10 two-lane wavefronts live on a CU (2.5 per SIMD = 81,920 tables on the 256 CUs of an
        // MI355X), the slim one 12.  Batches with more wavefronts than that take the slim image -- 67.0 vs 68.9 us per chunk
        // at 131,072 tables, 84.9 vs 91.8 at 196,608, 361 vs 403 at 1,048,576; where every wavefront is resident anyway it
        // only costs the river's divisions (37.7 vs 37.2 us at 65,536 tables).
        if (chunk_slim(v)) launch_one<PULSE_PH_STEP, true, 2, 5, 2>(v, actions, nullptr, rewards_even, pa, ca, st);
        else launch_one<PULSE_PH_STEP, true, 2, 5, 1>(v, actions, nullptr, rewards_even, pa, ca, st);
    } else launch_any<PULSE_PH_STEP, true, 1>(v, actions, nullptr, rewards_even, pa, ca, st);
}

int pulse::chunk_grid(const PulsePokerView& v) { return (int)step_grid(v, lanes_for(v, true)).x; }

int pulse::chunk_resident_blocks(const PulsePokerView& v, const float* obs_odd, int* grid) {
    if (grid) *grid = chunk_grid(v);
    if (lanes_for(v, true) == 2) return chunk_slim(v) ? resident_one<PULSE_PH_STEP, true, 2, 5, 2>(v, obs_odd) : resident_one<PULSE_PH_STEP, true, 2, 5, 1>(v, obs_odd);
    return v.max_players <= 12 ? resident_one<PULSE_PH_STEP, true, 4, 3, 1>(v, obs_odd) : resident_one<PULSE_PH_STEP, true, 4, 4, 1>(v, obs_odd);
}

extern "C" {

int pulse_poker_step(const PulsePokerView* v, const int64_t* actions, float* rewards, void* stream) {
    if (int rc = pulse::check_view(v, "pulse_poker_step")) return rc;
    if (!actions || !rewards) return pulse::fail(PULSE_EINVAL, "pulse_poker_step: null actions/rewards");
    if (v->n_games == 0) return 0;
    launch_phase<PULSE_PH_STEP>(*v, const_cast<int64_t*>(actions), nullptr, rewards, (hipStream_t)stream);
    return pulse::finish_launch("pulse_poker_step");
}

int pulse_poker_policy_step(const PulsePokerView* v, const uint8_t* agent_types, uint64_t seed, uint64_t step_counter,
                            uint64_t table_id0, int64_t* actions, float* rewards, void* stream) {
    if (int rc = pulse::check_view(v, "pulse_poker_policy_step")) return rc;
    if (!actions || !rewards || !agent_types) return pulse::fail(PULSE_EINVAL, "pulse_poker_policy_step: null argument");
    if (v->n_games == 0) return 0;
    pulse::launch_policy_step(*v, actions, rewards, PolicyArgs(pulse::pack_types(agent_types, v->n_players), seed, step_counter, table_id0), (hipStream_t)stream);
    return pulse::finish_launch("pulse_poker_policy_step");
}

int pulse_poker_phases(const PulsePokerView* v, uint32_t phases, const int64_t* actions, const int32_t* actor_idx,
                       float* rewards, void* stream) {
    if (int rc = pulse::check_view(v, "pulse_poker_phases")) return rc;
    if ((phases & (PULSE_PH_EXECUTE | PULSE_PH_REWARD)) && !actions)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_phases: actions required for EXECUTE/REWARD");
    if ((phases & PULSE_PH_REWARD) && !rewards) return pulse::fail(PULSE_EINVAL, "pulse_poker_phases: rewards required for REWARD");
    if (v->n_games == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int64_t* a = const_cast<int64_t*>(actions);
    switch (phases) {
    case PULSE_PH_STEP: launch_phase<PULSE_PH_STEP>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_STEP & ~PULSE_PH_EQUITY: launch_phase<(PULSE_PH_STEP & ~PULSE_PH_EQUITY)>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_EQUITY: launch_phase<PULSE_PH_EQUITY>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_EXECUTE: launch_phase<PULSE_PH_EXECUTE>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_ADVANCE: launch_phase<PULSE_PH_ADVANCE>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_FOLDWIN: launch_phase<PULSE_PH_FOLDWIN>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_SHOWDOWN: launch_phase<PULSE_PH_SHOWDOWN>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_FOLDWIN | PULSE_PH_SHOWDOWN: launch_phase<(PULSE_PH_FOLDWIN | PULSE_PH_SHOWDOWN)>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_CLEARDONE: launch_phase<PULSE_PH_CLEARDONE>(*v, a, nullptr, rewards, st); break;
    case PULSE_PH_REWARD: launch_phase<PULSE_PH_REWARD>(*v, a, actor_idx, rewards, st); break;
    case PULSE_PH_OBS: launch_phase<PULSE_PH_OBS>(*v, a, nullptr, rewards, st); break;
    default: return pulse::fail(PULSE_EINVAL, "pulse_poker_phases: unsupported phase combination");
    }
    return pulse::finish_launch("pulse_poker_phases");
}

/* Diagnostic (tools/ablate_step.py): the fused policy+step with some phases compiled out.
 * Results are NOT a valid transition; used only to price phases. */
int pulse_poker_ablate(const PulsePokerView* v, uint32_t phases, int64_t* actions, float* rewards, uint64_t types_packed,
                       uint64_t step_counter, void* stream) {
    if (int rc = pulse::check_view(v, "pulse_poker_ablate")) return rc;
    if (v->max_players > 12) return pulse::fail(PULSE_EINVAL, "pulse_poker_ablate: max_players <= 12");
    const dim3 grid = step_grid(*v, 4), block(kStepBlock);
    const PolicyArgs pa(types_packed, 1, step_counter, 0);
    const ChunkArgs ca{};
    hipStream_t st = (hipStream_t)stream;
#define PULSE_ABL(MASK) case (MASK): hipLaunchKernelGGL((poker_step_kernel<(MASK), true, 4, 3, false, 0>), grid, block, 0, st, *v, actions, (const int32_t*)nullptr, rewards, pa, ca); break;
    switch (phases) {
    PULSE_ABL(PULSE_PH_STEP)
    PULSE_ABL(PULSE_PH_STEP & ~PULSE_PH_EQUITY)
    PULSE_ABL(PULSE_PH_STEP & ~PULSE_PH_SHOWDOWN)
    PULSE_ABL(PULSE_PH_STEP & ~(PULSE_PH_EQUITY | PULSE_PH_SHOWDOWN))
    PULSE_ABL(PULSE_PH_STEP & ~PULSE_PH_REWARD)
    PULSE_ABL(PULSE_PH_STEP & ~PULSE_PH_OBS)
    PULSE_ABL(PULSE_PH_STEP & ~(PULSE_PH_EQUITY | PULSE_PH_SHOWDOWN | PULSE_PH_REWARD))
    PULSE_ABL(PULSE_PH_STEP & ~(PULSE_PH_EQUITY | PULSE_PH_SHOWDOWN | PULSE_PH_REWARD | PULSE_PH_OBS))
    PULSE_ABL(PULSE_PH_CAPTURE)
    default: return pulse::fail(PULSE_EINVAL, "pulse_poker_ablate: mask not instantiated");
    }
#undef PULSE_ABL
    return pulse::finish_launch("pulse_poker_ablate");
}

#if PULSE_STAMPS
int pulse_debug_set_stamp_buffer(unsigned long long* buf) {
    const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf));
    return e == hipSuccess ? 0 : pulse::fail_hip((int)e, "pulse_debug_set_stamp_buffer");
}
#endif

/* The trainer's step with the learner in it, first half, as ONE launch: pulse_qnet_act_select on the
 * observation `act->states` followed by pulse_poker_policy_step on `v` -- same results, word for word (the workgroup that
 * picks the actions of a window of 128 tables steps those tables itself). */
int pulse_poker_act_policy_step(const PulsePokerView* v, const uint8_t* agent_types, uint64_t seed, uint64_t step_counter, uint64_t table_id0,
                                int64_t* actions, float* rewards, const PulseQNet* net, const PulseQNetAct* act, void* stoprule, void* stream) {
    if (int rc = pulse::check_view(v, "pulse_poker_act_policy_step")) return rc;
    if (!actions || !rewards || !agent_types || !net || !act) return pulse::fail(PULSE_EINVAL, "pulse_poker_act_policy_step: null argument");
    if (v->n_games == 0) return 0;
    const int n = v->n_games;
    if (n % 128 != 0 || v->max_players > 10 || (v->flags & PULSE_VIEW_FOUR_LANES))
        return pulse::fail(PULSE_EINVAL, "pulse_poker_act_policy_step: needs a multiple of 128 tables of at most 10 seats (use pulse_qnet_act_select + pulse_poker_policy_step)");
    if (net->state_dim < 13 || net->state_dim > 40 || net->state_dim % 8 != 0 || net->n_actions < 1 || net->n_actions > 32 || act->row_stride % 4 != 0 ||
        act->row_stride < net->state_dim || ((uintptr_t)act->states & 15u) || ((uintptr_t)net->w1 & 15u) || ((uintptr_t)net->w2 & 15u) || ((uintptr_t)net->w3 & 15u) ||
        ((uintptr_t)net->w4 & 15u) || ((uintptr_t)net->w5 & 15u))
        return pulse::fail(PULSE_EINVAL, "pulse_poker_act_policy_step: needs 16-byte aligned fp32 rows of 16..40 inputs (a multiple of 8) and aligned weights");
    if (!net->w1 || !net->b1 || !net->w2 || !net->b2 || !net->w3 || !net->b3 || !net->w4 || !net->b4 || !net->w5 || !net->b5 || !act->states || !act->seat_idx || !act->row_mask_out)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_act_policy_step: null weight / state / seat_idx / row_mask_out pointer");
    if (!act->select_scratch || act->select_words < (int64_t)((n + 255) / 256) * 259 + 512)
        return pulse::fail(PULSE_EINVAL, "pulse_poker_act_policy_step: select_scratch must hold 259 words per 256 rows + 512");
    hipStream_t st = (hipStream_t)stream;
    pulse_qnet::QNetArgs qa{};
    qa.net = *net; qa.states = act->states; qa.row_stride = act->row_stride; qa.n_rows = n; qa.seat_idx = act->seat_idx; qa.q_seat = act->q_seat;
    qa.epsilon = act->epsilon; qa.seed = act->seed; qa.step = act->step; qa.table_id0 = act->table_id0; qa.actions = actions; qa.q_out = nullptr;
    qa.terminated = act->terminated; qa.row_mask_out = act->row_mask_out;
    qa.tsel_rows = act->select_scratch; qa.tsel_counts = act->select_scratch + (size_t)((n + 255) / 256) * 256;
    PulseStopRule* rule = static_cast<PulseStopRule*>(stoprule);
    const int n_waves = pulse::launch_waves(n, 2);
    PolicyArgs pa(pulse::pack_types(agent_types, v->n_players), seed, step_counter, table_id0);
    if (rule) if (int rc = pulse::stoprule_claim(rule, n_waves, &pa.wave_done, &pa.carry[0])) return rc;
    ChunkArgs ca{v->obs, rewards, 1};
    const bool wobs = obs_staging(*v, v->obs, 2);
    const size_t lds = std::max(pulse_qnet::kActLdsBytes, sizeof(int32_t) * 4 * (size_t)chunk_lds_dwords(v->obs_size, 10, 32, false));
    const auto fn = wobs ? &poker_act_step_kernel<true> : &poker_act_step_kernel<false>;
    const pulse::LdsLaunch r = pulse::launch_lds(fn, (unsigned)(n / 128), 256, lds, st, false, *v, actions, nullptr, rewards, pa, ca, qa);
    if (r.attr != hipSuccess) return pulse::fail_hip(r.attr, "pulse_poker_act_policy_step: LDS size attribute");
    if (int rc = pulse::finish_launch("pulse_poker_act_policy_step")) return rc;
    if (rule) return pulse::stoprule_commit(rule, n_waves, st);
    return 0;
}

}  // extern "C"
