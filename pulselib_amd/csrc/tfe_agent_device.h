// tfe_agent_device.h -- the pieces of a 2048 game loop that the learners share (tfe_mc.hip, tfe_ntuple.hip): the reward of a merge
// score, the per-move byte, the reset draw, the greedy scan with its tie coins and the per-workgroup counters of the roll-out and
// evaluation launches.  One copy each: a change of the tie rule or of a counter lands here.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox_device.h"
#include "tfe_device.h"

namespace pulse_tfe {

// TFE.py:185-187: log2 of the merge score of a move, 0 for 0 (<= 17 for n <= 4: five bits)
__device__ __forceinline__ int tfe_reward(int score) { return score > 0 ? 31 - __clz(score) : 0; }

// one recorded move: the action, the reward and the learner's flag (first visit / terminal) of that move
__device__ __forceinline__ uint8_t tfe_step_byte(int action, int reward, uint32_t flag) {
    return (uint8_t)((uint32_t)action | ((uint32_t)reward & 31u) << 2 | flag << 7);
}

// TFE.py:143-149, as pulse_tfe_reset: game (env_seed, id) starts with two spawns from draw 0 of the environment's stream
template <int NB>
__device__ __forceinline__ void tfe_reset(int (&b)[NB * NB], uint64_t env_seed, uint64_t id) {
#pragma unroll
    for (int i = 0; i < NB * NB; ++i) b[i] = 0;
    const pulse_philox::U4 rnd = pulse_philox::philox4x32(env_seed, id, 0ull);
    tfe_spawn<NB>(b, rnd.x, rnd.y);
    tfe_spawn<NB>(b, rnd.z, rnd.w);
}
__device__ __forceinline__ PackedBoard tfe_reset_packed(uint64_t env_seed, uint64_t id) {
    PackedBoard p{0u, 0u};
    const pulse_philox::U4 rnd = pulse_philox::philox4x32(env_seed, id, 0ull);
    tfe_spawn_packed(p, rnd.x, rnd.y);
    tfe_spawn_packed(p, rnd.z, rnd.w);
    return p;
}

// The greedy action among four q (OnPolicyFirstVisit.py:52-62): the candidates in the order a = 0..3, the first is the best so far,
// a larger q replaces it, an equal q replaces it on bit 31 of word a - 1 of `coins`.  -1: no candidate.  The coins are constant per
// (state, round) and matter only where two q are equal: the caller draws them under any_two_equal, with its own key for the state,
// and passes zeros otherwise.  All: the four moves are candidates and `cand` is not read.
__device__ __forceinline__ bool any_two_equal(const double (&q)[4]) {
    return q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3];
}
template <bool All = true>
__device__ __forceinline__ int greedy_scan(const double (&q)[4], const pulse_philox::U4& coins, const bool* cand = nullptr) {
    const uint32_t coin[4] = {0u, coins.x >> 31, coins.y >> 31, coins.z >> 31};
    int best = -1;
    double best_q = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const bool take = (All || cand[a]) && (best < 0 || q[a] > best_q || (q[a] == best_q && coin[a] != 0u));
        best_q = take ? q[a] : best_q;
        best = take ? a : best;
    }
    return best;
}

// Two per-workgroup counters of a launch (wg: two zeroed LDS words), added to the caller's stats[at0] and stats[at1] once per
// workgroup.  Called by every thread of the workgroup.
__device__ __forceinline__ void add_stats(unsigned long long* wg, int64_t* stats, int at0, unsigned long long v0, int at1, unsigned long long v1) {
    if (v0) atomicAdd(&wg[0], v0);                        // LDS
    if (v1) atomicAdd(&wg[1], v1);
    __syncthreads();
    if (threadIdx.x == 0 && wg[0]) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + at0, wg[0]);
    if (threadIdx.x == 1 && wg[1]) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + at1, wg[1]);
}

// An evaluation launch's counters: summary[8] then max_tile_hist[16], reduced in LDS (wg: kEvalBins zeroed words) and added once
// per workgroup and non-zero word.  Word kEvalMax is a maximum, the others are sums; what the words mean is the caller's.
constexpr int kEvalSummary = 8, kEvalBins = kEvalSummary + 16, kEvalMax = 4;
__device__ __forceinline__ void add_game(unsigned long long* wg, const unsigned long long (&v)[kEvalSummary], int bin) {
#pragma unroll
    for (int i = 0; i < kEvalSummary; ++i)
        if (v[i]) { if (i == kEvalMax) atomicMax(&wg[i], v[i]); else atomicAdd(&wg[i], v[i]); }       // LDS
    atomicAdd(&wg[kEvalSummary + bin], 1ull);
}
__device__ __forceinline__ void flush_bins(unsigned long long* wg, int64_t* summary, int64_t* hist) {
    __syncthreads();
    const int i = (int)threadIdx.x;
    if (i < kEvalBins && wg[i]) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(i < kEvalSummary ? summary + i : hist + (i - kEvalSummary));
        if (i == kEvalMax) atomicMax(dst, wg[i]); else atomicAdd(dst, wg[i]);          // (scores are not negative)
    }
}

}  // namespace pulse_tfe
