// tfe_ntuple_search_rollout.hip -- the 2048 n-tuple network's training roll-out under expectimax search, one
// launch: pulse_tfe_nt_rollout_search (include/pulse_env.h).  pulse_tfe_nt_rollout's games, draws and records with the greedy
// action taken on the q of the search, one chance layer deep (section 13.1) or two (section 13.4).
//
// The game loop is play_game<true>, as tfe_ntuple.hip's roll-out runs it; the mapping of a game to lanes is the evaluation's under
// the same policy: at one layer 32 lanes play a game alike and lane 0 of the group writes (tfe_ntuple_search.hip), at two a workgroup
// of 256 does and thread 0 writes (tfe_ntuple_search_deep.hip).  What is recorded beside the key and the byte is the NETWORK's V of
// the chosen afterstate, not the search's backed-up value: q_of fills v with values4 of the four afterstates before the search
// starts, so that its indices and loaded words are dead by then and eight registers (the four doubles) live across the search.
// Every lane of a group (of the workgroup, at two layers) holds the same four afterstates: the gathers are uniform and every lane
// has the same v.  Nothing lane-dependent encloses q_of -- search_q2's two barriers per move are reached by the 256 lanes of a game
// together, which leave the loop at the same move -- and `writer` guards stores only.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::finish_launch;

// one game per group of 32 lanes: g < n_games is the same in the 32, and a group beyond the batch only meets the barrier of the counts
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search_rollout_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    play_game<true>(o, wg, g, s == 0,
                    [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                        values4<IMG>(net, o.weights, ka, v);
                        search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                    });
}

// one game per workgroup: g is blockIdx.x (grid = n_games), so the 256 lanes play the game alike and reach search_q2's barriers together
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search2_rollout_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[2];
    __shared__ double terms[4 * kGroup];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    play_game<true>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                    [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                        values4<IMG>(net, o.weights, ka, v);
                        search_q2<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, terms, q);
                    });
}

}  // namespace

extern "C" int pulse_tfe_nt_rollout_search(const PulseTfeNtRollout* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_rollout_search";
    NtDev dev;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    const dim3 block(kSearchBlock);
    hipStream_t st = (hipStream_t)stream;
    if (layers == 1) {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock));
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search_rollout_kernel<8>, grid, block, 0, st, g, dev);
        else hipLaunchKernelGGL(tfe_nt_search_rollout_kernel<1>, grid, block, 0, st, g, dev);
    } else {
        const dim3 grid((unsigned)g.n_games);
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search2_rollout_kernel<8>, grid, block, 0, st, g, dev);
        else hipLaunchKernelGGL(tfe_nt_search2_rollout_kernel<1>, grid, block, 0, st, g, dev);
    }
    return finish_launch("pulse_tfe_nt_rollout_search launch");
}
