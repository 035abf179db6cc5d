// tfe_ntuple_search_adaptive.hip -- the 2048 n-tuple network under expectimax search whose depth the board chooses, per move (DESIGN.md
// section 13.11), two launches: pulse_tfe_nt_search_adaptive and pulse_tfe_nt_evaluate_search_adaptive (include/pulse_env.h).
//
// For the board B a move is made from, n = its empty cells: with n <= deep_empty_max the four q are those of the two-layer search
// (section 13.4: search_q2), otherwise those of the one-layer search (section 13.1: search_q), bit for bit.  One board or game per
// workgroup of 256 lanes = 8 groups of 32, the two-layer mapping.  A deep move runs search_q2 as it stands.  On a shallow move the
// four candidate moves go side by side: group a < 4 runs the chance layer of move a (search_q_move, the one copy) and its lane 0
// stores q_a into four doubles of LDS of their own; groups 4..7 only meet the barriers; after a workgroup barrier every lane reads
// the four q.  n depends on the board alone, which the 256 lanes carry alike, so they take the branch alike and nothing
// lane-dependent encloses a barrier (search_q_adaptive, tfe_ntuple_search_device.h).  The game kernel is play_game, untouched, under
// that q; the closure counts the moves at each depth and thread 0 adds the two counts once, at the game's end.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

// one board per workgroup; o: the entry point's struct as it came, after the checks
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search_adaptive_kernel(const PulseTfeNtSearch o, const NtDev net, const uint32_t* __restrict__ lut,
                                                                              const int deep_empty_max) {
    __shared__ double terms[4 * kGroup];
    __shared__ double qs[4];
    const int g = (int)blockIdx.x;                                                      // (grid = n_boards)
    const uint64_t key_b = o.boards[g];
    uint64_t ka[4];
    int sc[4];
    moves4(key_b, lut, ka, sc);
    double q[4];
    search_q_adaptive<IMG>(net, o.net.weights, lut, o.gamma, key_b, ka, sc, deep_empty_max, terms, qs, q);
    uint32_t bits;
    const int best = greedy_of(q, key_b, ka, o.tie_seed, o.round, &bits);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) o.q[(size_t)g * 4 + a] = q[a];
        o.action[g] = (int8_t)best;
        o.candidates[g] = (uint8_t)bits;
    }
}

// One game per workgroup, as tfe_nt_play_kernel at 256 lanes: g is blockIdx.x (grid = n_games), the 256 lanes play the game alike and
// thread 0 writes and counts.  depth_stats: [0] += the game's moves whose q came from two layers, [1] += those from one; or null.
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_play_adaptive_kernel(const Games o, const NtDev net, const int deep_empty_max,
                                                                            unsigned long long* __restrict__ depth_stats) {
    __shared__ unsigned long long wg[kEvalBins];
    __shared__ double terms[4 * kGroup];
    __shared__ double qs[4];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t n_deep = 0u, n_shallow = 0u;                                               // (a game has at most 65,535 moves)
    play_game<false>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                     [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&)[4], double (&q)[4]) {
                         const bool deep = search_q_adaptive<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, deep_empty_max, terms, qs, q);
                         n_deep += deep ? 1u : 0u;
                         n_shallow += deep ? 0u : 1u;
                     });
    if (threadIdx.x == 0 && depth_stats) {
        atomicAdd(depth_stats, (unsigned long long)n_deep);
        atomicAdd(depth_stats + 1, (unsigned long long)n_shallow);
    }
}

}  // namespace

extern "C" int pulse_tfe_nt_search_adaptive(const PulseTfeNtSearch* o, int32_t deep_empty_max, void* stream) {
    const char* name = "pulse_tfe_nt_search_adaptive";
    NtDev dev;
    const uint32_t* lut = nullptr;
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_deep_empty_max(deep_empty_max, name)) return rc;     // (before the struct's: a threshold in range is seen to pass)
    if (int rc = check_search(o, name, &dev)) return rc;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    const dim3 grid((unsigned)o->n_boards), block(kSearchBlock);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search_adaptive_kernel<8>, grid, block, 0, (hipStream_t)stream, *o, dev, lut, (int)deep_empty_max);
    else hipLaunchKernelGGL(tfe_nt_search_adaptive_kernel<1>, grid, block, 0, (hipStream_t)stream, *o, dev, lut, (int)deep_empty_max);
    return finish_launch("pulse_tfe_nt_search_adaptive launch");
}

extern "C" int pulse_tfe_nt_evaluate_search_adaptive(const PulseTfeNtEval* o, int32_t deep_empty_max, int64_t* depth_stats, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_search_adaptive";
    NtDev dev;
    Games g;
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_deep_empty_max(deep_empty_max, name)) return rc;     // (these two before the struct's, as above)
    if ((uintptr_t)depth_stats & 7u) return fail_named(name, "depth_stats must be 8-byte aligned");
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    const dim3 grid((unsigned)g.n_games), block(kSearchBlock);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(depth_stats);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_play_adaptive_kernel<8>, grid, block, 0, (hipStream_t)stream, g, dev, (int)deep_empty_max, stats);
    else hipLaunchKernelGGL(tfe_nt_play_adaptive_kernel<1>, grid, block, 0, (hipStream_t)stream, g, dev, (int)deep_empty_max, stats);
    return finish_launch("pulse_tfe_nt_evaluate_search_adaptive launch");
}
