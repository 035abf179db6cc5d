// tfe_ntuple_adaptive_rollout.hip -- the 2048 n-tuple network's training roll-out under the search whose depth the board chooses
// (DESIGN.md section 13.13), one launch: pulse_tfe_nt_rollout_adaptive (include/pulse_env.h).
//
// pulse_tfe_nt_evaluate_search_adaptive's policy (section 13.11: two chance layers on a board with at most deep_empty_max empty cells,
// one on the others) with pulse_tfe_nt_rollout_search's records (section 13.5), where asked pulse_tfe_nt_rollout_backed's value
// (section 13.6) of the q at the depth the board chose, and where asked from the boards of `start` (section 13.7).  The game loop is
// play_game<true, Backed, From>, untouched, on the two-layer mapping: one game per workgroup of 256 lanes, which play it alike, and
// thread 0 writes and counts.  What a move records beside the key and the byte is the NETWORK's V of the chosen afterstate, formed
// before the search starts as in tfe_nt_play_kernel; the closure counts the moves at each depth as tfe_nt_play_adaptive_kernel's does.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

static_assert(sizeof(PulseTfeNtRollout) == 232, "struct layouts are part of the ABI");

// One game per workgroup: g is blockIdx.x (grid = n_games), so `g < n_games` holds in every lane and the 256 lanes play the game
// alike -- the same boards, draws and length.  Barriers: search_q_adaptive meets two workgroup barriers a call on either side of a
// branch that the board alone decides; nothing lane-dependent encloses q_of -- `writer` guards stores only, with Record, Backed and
// From alike -- and the 256 lanes leave the loop at the same move, as in tfe_nt_play_kernel<256, IMG, true, ...>.
// From: thread 0 stores 0 into an unusable start[g] while a slower wavefront may not have read the word yet.  The word is 8-byte
// aligned (checked below) and read and written as one 64-bit access, so such a lane reads either the unusable word as it was or 0;
// 0 is itself unusable (play_game tests key0 != 0 first), so every lane falls back to the reset board: the four wavefronts decide
// alike whichever they read.  A usable word is never written.
// depth_stats: [0] += the game's moves whose q came from two layers, [1] += those from one; or null.
template <int IMG, bool Backed, bool From>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_record_adaptive_kernel(const Games o, const NtDev net, const int deep_empty_max,
                                                                              unsigned long long* depth_stats) {
    __shared__ unsigned long long wg[2];
    __shared__ double terms[4 * kGroup];
    __shared__ double qs[4];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t n_deep = 0u, n_shallow = 0u;                                               // (a game has at most 65,535 moves)
    play_game<true, Backed, From>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                                  [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                      values4<IMG>(net, o.weights, ka, v);
                                      const bool deep = search_q_adaptive<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, deep_empty_max, terms, qs, q);
                                      n_deep += deep ? 1u : 0u;
                                      n_shallow += deep ? 0u : 1u;
                                  });
    if (threadIdx.x == 0 && depth_stats) {
        atomicAdd(depth_stats, (unsigned long long)n_deep);
        atomicAdd(depth_stats + 1, (unsigned long long)n_shallow);
    }
}

template <bool Backed, bool From>
void launch_record(const Games& g, const NtDev& dev, const bool symmetric, const int deep_empty_max, unsigned long long* stats, void* stream) {
    const dim3 grid((unsigned)g.n_games), block(kSearchBlock);
    if (symmetric) hipLaunchKernelGGL((tfe_nt_record_adaptive_kernel<8, Backed, From>), grid, block, 0, (hipStream_t)stream, g, dev, deep_empty_max, stats);
    else hipLaunchKernelGGL((tfe_nt_record_adaptive_kernel<1, Backed, From>), grid, block, 0, (hipStream_t)stream, g, dev, deep_empty_max, stats);
}

}  // namespace

extern "C" int pulse_tfe_nt_rollout_adaptive(const PulseTfeNtRollout* o, int32_t deep_empty_max, double* backed, uint64_t* start,
                                             int64_t* depth_stats, void* stream) {
    const char* name = "pulse_tfe_nt_rollout_adaptive";
    NtDev dev;
    Games g;
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_deep_empty_max(deep_empty_max, name)) return rc;     // (these before the struct's: a threshold in range is seen to pass)
    if ((uintptr_t)depth_stats & 7u) return fail_named(name, "depth_stats must be 8-byte aligned");
    if ((uintptr_t)backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if ((uintptr_t)start & 7u) return fail_named(name, "start must be 8-byte aligned");
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    g.backed = backed;
    g.start = start;
    const bool symmetric = o->net.symmetric != 0;
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(depth_stats);
    if (backed && start) launch_record<true, true>(g, dev, symmetric, (int)deep_empty_max, stats, stream);
    else if (backed) launch_record<true, false>(g, dev, symmetric, (int)deep_empty_max, stats, stream);
    else if (start) launch_record<false, true>(g, dev, symmetric, (int)deep_empty_max, stats, stream);
    else launch_record<false, false>(g, dev, symmetric, (int)deep_empty_max, stats, stream);
    return finish_launch("pulse_tfe_nt_rollout_adaptive launch");
}
