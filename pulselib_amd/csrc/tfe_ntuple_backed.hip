// tfe_ntuple_backed.hip -- the 2048 n-tuple network's search-backed TD targets, two entry points:
// pulse_tfe_nt_rollout_backed and pulse_tfe_nt_learn_backed (include/pulse_env.h).
//
// pulse_tfe_nt_rollout_search plays a round's games on the q of the search and then drops them: the learners bootstrap from the
// network's one-ply V of the next record.  Here a move also records the value the search backed up for the board it was made on,
// backed[t] = the largest q over the moves that change the board, and the learner's difference of a move is backed[t + 1] - V_t: the
// search's estimate, for the spawn that happened, of what V(afterstate_t) estimates.
//
// The recording kernels are tfe_ntuple_search_rollout.hip's four, mapped as those are (32 lanes per game and 8 games per workgroup at
// one layer, one game per workgroup of 256 at two; values4 before the search, so that only the four doubles live across it), running
// play_game<true, true>: the maximum is formed from the q and the afterstates every lane of a game holds alike, and `writer` guards
// one more store.  Nothing lane-dependent encloses q_of: search_q2's two barriers per move are reached by the 256 lanes of a game
// together.  The learner is two launches: the walk of tfe_ntuple_device.h with Backed set, which leaves D_t in deltas, and the
// learners' one scatter with the differences given (launch_scatter, or launch_scatter_tc where acc_abs is set).
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

static_assert(sizeof(PulseTfeNtLearnBacked) == 208 && sizeof(PulseTfeNtRollout) == 232, "struct layouts are part of the ABI");

// one game per group of 32 lanes: g < n_games is the same in the 32, and a group beyond the batch only meets the barrier of the counts
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_backed_rollout_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    play_game<true, true>(o, wg, g, s == 0,
                          [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                              values4<IMG>(net, o.weights, ka, v);
                              search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                          });
}

// one game per workgroup: g is blockIdx.x (grid = n_games), so the 256 lanes play the game alike and reach search_q2's barriers together
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_backed2_rollout_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[2];
    __shared__ double terms[4 * kGroup];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    play_game<true, true>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                          [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                              values4<IMG>(net, o.weights, ka, v);
                              search_q2<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, terms, q);
                          });
}

}  // namespace

namespace pulse_tfe {

// the launch of the walk with Backed set (declared in tfe_ntuple_device.h: pulse_tfe_nt_learn_staged launches it too)
void launch_backed_walk(const WalkBacked& o, void* stream) {
    hipLaunchKernelGGL(tfe_nt_lambda_walk_kernel<true>, dim3((unsigned)((o.n_games + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, (hipStream_t)stream, o);
}

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_rollout_backed(const PulseTfeNtRollout* o, int32_t layers, double* backed, void* stream) {
    const char* name = "pulse_tfe_nt_rollout_backed";
    NtDev dev;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (!backed) return fail_named(name, "backed is null");
    if ((uintptr_t)backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    g.backed = backed;
    const dim3 block(kSearchBlock);
    hipStream_t st = (hipStream_t)stream;
    if (layers == 1) {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock));
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_backed_rollout_kernel<8>, grid, block, 0, st, g, dev);
        else hipLaunchKernelGGL(tfe_nt_backed_rollout_kernel<1>, grid, block, 0, st, g, dev);
    } else {
        const dim3 grid((unsigned)g.n_games);
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_backed2_rollout_kernel<8>, grid, block, 0, st, g, dev);
        else hipLaunchKernelGGL(tfe_nt_backed2_rollout_kernel<1>, grid, block, 0, st, g, dev);
    }
    return finish_launch("pulse_tfe_nt_rollout_backed launch");
}

extern "C" int pulse_tfe_nt_learn_backed(const PulseTfeNtLearnBacked* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_backed";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (!(o->lambda >= 0.0 && o->lambda <= 1.0)) return fail_named(name, "lambda must be in [0, 1]");
    if (!o->deltas) return fail_named(name, "deltas is null");
    if (!o->backed) return fail_named(name, "backed is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->deltas & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / deltas / stats must be 8-byte aligned");
    if ((uintptr_t)o->backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if ((uintptr_t)o->acc_abs & 7u) return fail_named(name, "acc_abs must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    WalkBacked w{};                                                                     // the walk, then the adds of what it left
    w.n_games = o->n_games; w.max_steps = o->max_steps; w.gamma = o->gamma; w.lambda = o->lambda;
    w.values = o->values; w.steps = o->steps; w.lengths = o->lengths; w.deltas = o->deltas; w.backed = o->backed;
    launch_backed_walk(w, stream);
    m.deltas = o->deltas;
    if (o->acc_abs) {
        m.acc_abs = o->acc_abs;
        launch_scatter_tc(m, dev, o->net.symmetric != 0, stream);
    } else {
        launch_scatter(m, dev, o->net.symmetric != 0, stream);
    }
    return finish_launch("pulse_tfe_nt_learn_backed launch");
}
