// blackjack_mc.hip -- first-visit Monte-Carlo value estimation for Blackjack as ONE launch (pulse_blackjack_mc_rollout).
//
//   agents/MonteCarlo/FirstVisitMonteCarlo.py:5-31 fed by environments/blackjack/blackjack.py:23-186: the reference resets the
//   env, steps it until every game is over, builds one episode list per game on the host and calls learn() per game.
//
// Here one lane plays one game from the shuffle to the terminal step in registers and LDS (blackjack_device.h: the env kernels'
// own shuffle and card arithmetic, so game (seed, g, episode) IS the game BlackJack.reset() + step() plays) and none of the
// env's state ever reaches memory.  The reward is 0 before the terminal step and +-1 at it, so the first-visit return of the state
// seen k steps before the end is r * gamma^k: learning is counting the visits per (state, k, sign of r) -- integer adds, which
// commute, so the result does not depend on the order of the atomics -- and gamma enters on the host only.
// Every workgroup is persistent: it loops over games, counts into a histogram in its LDS (32-bit LDS atomics, plain: they are 8 % of the
// launch) and adds its non-zero cells to the caller's int64 accumulator once, at the end.
//
// The same kernel, instantiated with CONTROL, counts first visits of (state, ACTION) pairs for on-policy Monte-Carlo control
// (agents/MonteCarlo/OnPolicyFirstVisit.py:24-49, pulse_blackjack_mc_control_rollout): a stand ends the game, so it is only ever
// seen at k = 0, and 2 cells per state beside the 32 of the hits hold it.  pulse_blackjack_mc_improve turns that histogram into
// the next epsilon-soft policy table on the device (:51-71), so roll-out -> improve -> roll-out needs no host round trip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "blackjack_device.h"
#include "pulse_internal.h"

// Diagnostic twin builds only (`make bjmc-ablate ABL=n`, tools/bench_blackjack_mc.py): bit 0 = no histogram adds (the games are still
// played: the counters need them), bit 1 = a two-instruction hash instead of Philox in the shuffle.  The product is built with 0.
#ifndef PULSE_BJMC_ABL
#define PULSE_BJMC_ABL 0
#endif

namespace {

using namespace pulse_bj;

// 512 lanes share one histogram: 46 KB of counts + 27 KB of decks + 4 KB of policy = 77 KB of LDS per workgroup, two workgroups =
// sixteen wavefronts per CU.  (256 lanes per histogram: 64 KB per workgroup, eight wavefronts per CU, 1.39 x the time per game:
// the shuffle is a chain of dependent LDS byte swaps, so the wavefronts in flight set the rate -- DESIGN.md section 11.)
constexpr int kBlock = 512;
constexpr int kMaxActions = PULSE_BJ_MC_MAX_ACTIONS;
// The LDS histogram covers the states a deck of cards 0..51 can reach: player's sum 4..21 x usable ace x upcard 2..11.
constexpr int kSumLo = 4, kSums = 18, kUpLo = 2, kUps = 10;
constexpr int kCompactStates = kSums * 2 * kUps;                       // 360
// The policy's draws are keyed apart from the shuffle's (which uses the caller's seed as it is), the tie coins of the policy
// improvement apart from both (PULSE_BJ_MCC_TIE_KEY).
constexpr uint64_t kPolicyKey = 0xB1AC7AC4D3A1E5ull;
constexpr uint64_t kTieKey = PULSE_BJ_MCC_TIE_KEY;

// Value estimation: hit and stand share the k x sign cells of a state.  Control: the hits' k x sign cells, then the stand's two.
template <bool CONTROL> struct Layout {
    static constexpr int kCellsPerState = CONTROL ? PULSE_BJ_MCC_CELLS : kMaxActions * 2;
    static constexpr int kCompactCells = kCompactStates * kCellsPerState;       // 11,520 cells = 46,080 bytes | 12,240 = 48,960
    static constexpr size_t kProbAt = (size_t)kCompactCells * 4, kStatsAt = kProbAt + PULSE_BJ_MC_STATES * 4, kDeckAt = kStatsAt + 32;
    static constexpr size_t kLdsBytes = kDeckAt + (size_t)kBlock * 53;          // 77,344 | 80,224
};
static_assert(Layout<false>::kLdsBytes == 77344 && Layout<true>::kLdsBytes == 80224, "LDS budget (DESIGN.md section 11)");
static_assert(2 * Layout<true>::kLdsBytes <= 160 * 1024 && Layout<true>::kLdsBytes <= 81920, "two workgroups per CU");

// PULSE_BJ_MC_STATE_INDEX, or -1 for a state outside the public layout (only cards outside 0..51 lead there)
__device__ __forceinline__ int state_index(int sum, bool has, int up) {
    return ((uint32_t)sum < 32u && (uint32_t)up < 16u) ? (sum * 2 + (int)has) * 16 + up : -1;
}

template <bool CONTROL>
__global__ __launch_bounds__(kBlock) void blackjack_mc_kernel(const PulseBlackjackMC o) {
    constexpr int kCellsPerState = Layout<CONTROL>::kCellsPerState, kCompactCells = Layout<CONTROL>::kCompactCells;
    constexpr size_t kProbAt = Layout<CONTROL>::kProbAt, kStatsAt = Layout<CONTROL>::kStatsAt, kDeckAt = Layout<CONTROL>::kDeckAt;
    extern __shared__ __align__(16) uint8_t lds[];       // kLdsBytes: beyond the 64 KB a static allocation may have
    uint32_t* hist = reinterpret_cast<uint32_t*>(lds);
    float* prob = reinterpret_cast<float*>(lds + kProbAt);
    unsigned long long* wg_stats = reinterpret_cast<unsigned long long*>(lds + kStatsAt);
    uint8_t (*deck)[53] = reinterpret_cast<uint8_t (*)[53]>(lds + kDeckAt);     // 53: odd stride, as in the reset kernel
    for (int i = threadIdx.x; i < kCompactCells; i += kBlock) hist[i] = 0u;
    for (int i = threadIdx.x; i < PULSE_BJ_MC_STATES; i += kBlock) prob[i] = o.hit_prob[i];
    if (threadIdx.x < 4) wg_stats[threadIdx.x] = 0ull;
    __syncthreads();

    unsigned long long* acc = reinterpret_cast<unsigned long long*>(o.acc);
    const uint32_t n_games = (uint32_t)o.n_games;
    const uint32_t total = n_games * (uint32_t)o.n_episodes;          // (< 2^32: checked by the host)
    const uint32_t stride = gridDim.x * kBlock;
    uint8_t* d = deck[threadIdx.x];
    uint32_t n_played = 0, n_won = 0, n_actions = 0, n_capped = 0;

    for (uint64_t it = (uint64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += stride) {
        const uint32_t item = (uint32_t)it;               // (the counter itself is 64 bits wide: item + stride may pass 2^32)
        const uint32_t e = item / n_games, g = item - e * n_games;
        const uint64_t episode = o.episode + e;
        const int32_t* src = o.decks_src ? o.decks_src + (size_t)item * 52 : nullptr;
        int c0, c1, c2, c3;
        if (src) { c0 = src[0]; c1 = src[1]; c2 = src[2]; c3 = src[3]; }
        else { bj_shuffle<(PULSE_BJMC_ABL & 2) != 0>(d, o.seed, (uint64_t)g, episode); c0 = d[0]; c1 = d[1]; c2 = d[2]; c3 = d[3]; }
        auto card = [&](int pos) -> int { return (uint32_t)pos < 52u ? (src ? src[pos] : (int)d[pos]) : 0; };   // as the step kernel reads it
        const BjDeal deal = bj_deal(c0, c1, c2, c3);
        int ps = deal.ps, ds = deal.ds, pos = 4;
        bool has = deal.has, dhas = deal.dhas;
        const int up = deal.d1;

        int st[kMaxActions];                              // the state before action t (statically indexed: the loops are unrolled)
        int T = 0, rew = 0;
        uint32_t stands = 0;                              // bit t: action t was a stand
        bool done = false;
        U4 draw{0u, 0u, 0u, 0u};
        int draw_call = -1;
#pragma unroll
        for (int t = 0; t < kMaxActions; ++t) {
            if (!done) {
                const int s = state_index(ps, has, up);
                st[t] = s;
                const float p = s >= 0 ? prob[s] : 0.0f;   // a state outside the table stands
                bool hit = p >= 1.0f;
                if (!hit && p > 0.0f) {                    // one 24-bit uniform per action, drawn only where the table asks for one
                    if (draw_call != (t >> 2)) { draw = philox4x32(o.seed ^ kPolicyKey, (uint64_t)g, episode * 4 + (uint64_t)(t >> 2)); draw_call = t >> 2; }
                    hit = (float)(u4_word(draw, t & 3) >> 8) * (1.0f / 16777216.0f) < p;
                }
                T = t + 1;
                if (hit) {                                                              // blackjack.py:118-135, :166-168
                    bj_draw(card(pos), ps, has); pos += 1;
                    if (ps > 21) { rew = -1; done = true; }
                } else {                                                                // :139-160, :171-177
                    stands |= 1u << t;
                    bool active = ds < 17;
                    while (active) { bj_draw(card(pos), ds, dhas); pos += 1; active = bj_dealer_active(ds, pos); }
                    rew = bj_stand_reward(ps, ds); done = true;
                }
            } else {
                st[t] = -1;
            }
        }
        n_played += 1;
        if (o.trace) {                                    // actions taken (0 = hit, 1 = stand), then -1
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                w[q] = 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int t = 4 * q + b;
                    w[q] |= (t < T ? ((stands >> t) & 1u) : 0xFFu) << (8 * b);
                }
            }
            reinterpret_cast<uint4*>(o.trace)[item] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (!done) { n_capped += 1; continue; }           // the cap: nothing is learnt from a game that did not end
        n_won += rew > 0; n_actions += (uint32_t)T;
        const int sign = rew < 0;
#pragma unroll
        for (int t = 0; t < kMaxActions; ++t) {
            if (t < T) {
                const int s = st[t];
                bool first = s >= 0;
#pragma unroll
                for (int j = 0; j < t; ++j) first = first && st[j] != s;                // first visit (FirstVisitMonteCarlo.py:24-31)
                int cell = (T - 1 - t) * 2 + sign;
                if constexpr (CONTROL) {                  // first visit of the PAIR (OnPolicyFirstVisit.py:30-36): every action before
                    if ((stands >> t) & 1u) {             // a stand was a hit, so the stand -- the last action, k = 0 -- is always one
                        first = s >= 0;
                        cell = kMaxActions * 2 + sign;
                    }
                }
                if (first && !(PULSE_BJMC_ABL & 1)) {
                    const int sum = s >> 5, ace = (s >> 4) & 1, u = s & 15;
                    if ((uint32_t)(sum - kSumLo) < (uint32_t)kSums && (uint32_t)(u - kUpLo) < (uint32_t)kUps)
                        atomicAdd(&hist[(((sum - kSumLo) * 2 + ace) * kUps + (u - kUpLo)) * kCellsPerState + cell], 1u);
                    else
                        atomicAdd(&acc[(size_t)s * kCellsPerState + cell], 1ull);
                }
            }
        }
    }

    atomicAdd(&wg_stats[0], (unsigned long long)n_played); atomicAdd(&wg_stats[1], (unsigned long long)n_won);
    atomicAdd(&wg_stats[2], (unsigned long long)n_actions); atomicAdd(&wg_stats[3], (unsigned long long)n_capped);
    __syncthreads();
    for (int i = threadIdx.x; i < kCompactCells; i += kBlock) {
        const uint32_t n = hist[i];
        if (n) {
            const int c = i / kCellsPerState, cell = i % kCellsPerState;
            const int sum = c / (2 * kUps) + kSumLo, ace = (c / kUps) & 1, u = c % kUps + kUpLo;
            atomicAdd(&acc[(size_t)PULSE_BJ_MC_STATE_INDEX(sum, ace, u) * kCellsPerState + cell], (unsigned long long)n);
        }
    }
    if (threadIdx.x < 4 && wg_stats[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(o.stats) + threadIdx.x, wg_stats[threadIdx.x]);
}

using pulse::device_cus;
using pulse::fail_named;

// Both roll-out entry points: the checks, the grid and the launch.  (PulseBlackjackMCControl has PulseBlackjackMC's fields.)
template <bool CONTROL>
int rollout(const PulseBlackjackMC* o, void* stream, const char* name) {
    if (!o) return fail_named(name, "options are null");
    if (!o->acc) return fail_named(name, "acc is null");
    if (!o->stats) return fail_named(name, "stats is null");
    if (!o->hit_prob) return fail_named(name, "hit_prob is null");
    if (o->n_games <= 0) return fail_named(name, "n_games must be positive");
    if (o->n_episodes <= 0) return fail_named(name, "n_episodes must be positive");
    if ((uint64_t)o->n_games * (uint64_t)o->n_episodes > 0xFFFFFFFFull) return fail_named(name, "n_games * n_episodes must be below 2^32 per launch");
    if (((uintptr_t)o->acc & 7u) || ((uintptr_t)o->stats & 7u)) return fail_named(name, "acc / stats must be 8-byte aligned");
    if (((uintptr_t)o->hit_prob & 3u) || ((uintptr_t)o->decks_src & 3u)) return fail_named(name, "hit_prob / decks_src must be 4-byte aligned");
    if ((uintptr_t)o->trace & 15u) return fail_named(name, "trace must be 16-byte aligned (one row per store)");
    if (o->max_blocks < 0) return fail_named(name, "max_blocks must be >= 0 (0 = two workgroups per CU)");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    char what[96];
    if constexpr (CONTROL) {
        // Two workgroups per CU are what the kernel's time per game rests on (one: 1.39 x): a device or a build that cannot hold
        // them is an error, not a slower run.
        const void* fn = reinterpret_cast<const void*>(blackjack_mc_kernel<true>);
        static bool raised = false;                  // the query counts the LDS only within the function's limit: raise it first, once
        const hipError_t e = raised ? hipSuccess : hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Layout<true>::kLdsBytes);
        if (e != hipSuccess) { (void)hipGetLastError(); std::snprintf(what, sizeof what, "%s: LDS size attribute", name); return pulse::fail_hip(e, what); }
        raised = true;
        const int resident = pulse::resident_blocks_per_cu(fn, kBlock, Layout<true>::kLdsBytes);
        if (resident < 0) return resident;
        if (resident < 2) {
            char text[256];
            std::snprintf(text, sizeof text, "%s: %d workgroup(s) of %d lanes and %zu bytes of LDS fit on a CU, 2 are needed", name, resident, kBlock, Layout<true>::kLdsBytes);
            return pulse::fail(PULSE_ELAUNCH, text);
        }
    }
    const uint64_t total = (uint64_t)o->n_games * (uint64_t)o->n_episodes;
    const uint64_t needed = (total + kBlock - 1) / kBlock;
    // persistent workgroups, two per CU (their LDS); the flush of a workgroup's histogram is paid once per launch
    const uint64_t cap = o->max_blocks > 0 ? (uint64_t)o->max_blocks : 2ull * (uint64_t)device_cus();
    const unsigned grid = (unsigned)(needed < cap ? needed : cap);
    const pulse::LdsLaunch r = pulse::launch_lds(blackjack_mc_kernel<CONTROL>, grid, kBlock, Layout<CONTROL>::kLdsBytes, (hipStream_t)stream, false, *o);
    if (r.attr != hipSuccess) { std::snprintf(what, sizeof what, "%s: LDS size attribute", name); return pulse::fail_hip(r.attr, what); }
    if (r.launch != hipSuccess) { std::snprintf(what, sizeof what, "%s launch", name); return pulse::fail_hip(r.launch, what); }
    return 0;
}

// Policy improvement (OnPolicyFirstVisit.py:51-71) for all states at once, one lane per state: q(s, a) from the control
// histogram in float64 -- gamma^k by repeated multiplication, the sum over ascending k, as the host's returns_from_histogram
// forms them (no contraction: the library is built with -ffp-contract=off) -- then the epsilon-soft table the next roll-out reads.
__global__ __launch_bounds__(256) void blackjack_mc_improve_kernel(const PulseBlackjackMCImprove o) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= PULSE_BJ_MC_STATES) return;
    const int64_t* cells = o.acc + (size_t)s * PULSE_BJ_MCC_CELLS;
    int64_t n_hit = 0;
    double sum_hit = 0.0, pow_k = 1.0;
    for (int k = 0; k < kMaxActions; ++k) {
        const int64_t pos = cells[2 * k], neg = cells[2 * k + 1];
        n_hit += pos + neg;
        sum_hit += (double)(pos - neg) * pow_k;
        pow_k = o.gamma * pow_k;
    }
    const int64_t pos = cells[2 * kMaxActions], neg = cells[2 * kMaxActions + 1];
    const int64_t n_stand = pos + neg;
    const double sum_stand = (double)(pos - neg);                          // k = 0 only
    const double q_hit = n_hit ? sum_hit / (double)n_hit : 0.0;            // an unseen pair reads 0.0, as the reference's defaultdict(float)
    const double q_stand = n_stand ? sum_stand / (double)n_stand : 0.0;
    if (o.q) { o.q[2 * s] = q_hit; o.q[2 * s + 1] = q_stand; }
    if (n_hit + n_stand == 0) return;                                      // a state never visited keeps its probability
    bool stand = q_stand > q_hit;                                          // :52-62, the actions in the order hit, stand
    if (q_stand == q_hit) stand = (philox4x32(o.seed ^ kTieKey, (uint64_t)s, o.round).x & 1u) != 0u;
    const double explore = o.epsilon / 2.0;
    o.hit_prob[s] = (float)(stand ? explore : 1.0 - o.epsilon + explore);  // :65-71
}

}  // namespace

extern "C" int pulse_blackjack_mc_rollout(const PulseBlackjackMC* o, void* stream) {
    return rollout<false>(o, stream, "pulse_blackjack_mc_rollout");
}

extern "C" int pulse_blackjack_mc_control_rollout(const PulseBlackjackMCControl* o, void* stream) {
    static_assert(sizeof(PulseBlackjackMCControl) == sizeof(PulseBlackjackMC), "the two structs share one layout");
    return rollout<true>(reinterpret_cast<const PulseBlackjackMC*>(o), stream, "pulse_blackjack_mc_control_rollout");
}

extern "C" int pulse_blackjack_mc_improve(const PulseBlackjackMCImprove* o, void* stream) {
    const char* name = "pulse_blackjack_mc_improve";
    if (!o) return fail_named(name, "options are null");
    if (!o->acc) return fail_named(name, "acc is null");
    if (!o->hit_prob) return fail_named(name, "hit_prob is null");
    if (((uintptr_t)o->acc & 7u) || ((uintptr_t)o->q & 7u)) return fail_named(name, "acc / q must be 8-byte aligned");
    if ((uintptr_t)o->hit_prob & 3u) return fail_named(name, "hit_prob must be 4-byte aligned");
    if (!(o->epsilon >= 0.0 && o->epsilon <= 1.0)) return fail_named(name, "epsilon must be in [0, 1]");
    if (!std::isfinite(o->gamma)) return fail_named(name, "gamma must be finite");
    if (o->reserved0 != 0 || o->reserved1 != 0) return fail_named(name, "reserved0 / reserved1 must be 0 (zero-initialise the struct)");
    blackjack_mc_improve_kernel<<<PULSE_BJ_MC_STATES / 256, 256, 0, (hipStream_t)stream>>>(*o);
    return pulse::finish_launch("pulse_blackjack_mc_improve launch");
}
