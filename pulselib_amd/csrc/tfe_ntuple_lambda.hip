// tfe_ntuple_lambda.hip -- the 2048 n-tuple network's TD(lambda) learner, one entry point and two launches:
// pulse_tfe_nt_learn_lambda (include/pulse_env.h).
//
// The roll-out recorded per move the afterstate's key, its V as float64, the reward and the terminal bit, so the lambda-differences
// are one backward recurrence per game over data already in memory: D_t = delta_t + (gamma * lambda) * D_{t+1}.  The first kernel
// walks every game from its end, one lane per game, and writes D_t step-major beside the values; the second is pulse_tfe_nt_learn's
// scatter, one lane per recorded move, with D_t read instead of formed (the target, the clamp, the fixed-point conversion and the
// adds are tfe_ntuple_device.h's, one copy for both learners).  The recurrence carries the unclamped D; a move's add is clamped.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256, kWalkBlock = 64, kRows = 8;
static_assert(sizeof(PulseTfeNtLearnLambda) == 192, "struct layouts are part of the ABI");

// One lane per game, one wavefront per workgroup, t downwards from the wavefront's longest game: every lane of the wavefront is at
// the same row t, so a row's loads and stores are one 512-byte and one 64-byte segment, and a lane whose game is shorter waits with
// `t < length` as its predicate.  A lane reads its column of every row from the wavefront's first (what a row at or beyond its own
// length holds is loaded and not used); rows of kRows are loaded together, the next kRows before the chain of these is run, so the
// chain is one multiply and one add per move and no memory latency.  V and the byte of row t + 1 stay in registers for row t.
__global__ __launch_bounds__(kWalkBlock) void tfe_nt_lambda_walk_kernel(const PulseTfeNtLearnLambda o) {
    const int g = (int)blockIdx.x * kWalkBlock + (int)threadIdx.x;
    const size_t B = (size_t)o.n_games;
    int length = 0;
    if (g < o.n_games) {
        length = o.lengths[g];
        length = length > o.max_steps ? o.max_steps : length;                          // (the buffers hold max_steps rows)
    }
    int longest = length;
#pragma unroll
    for (int d = 1; d < kWalkBlock; d <<= 1) longest = max(longest, __shfl_xor(longest, d, kWalkBlock));
    if (longest < 1) return;
    const size_t col = (size_t)(g < o.n_games ? g : o.n_games - 1);                    // a lane beyond the batch reads the last column, and writes nothing
    const double gl = __dmul_rn(o.gamma, o.lambda);
    double v[kRows], nv[kRows];
    uint32_t s[kRows], ns[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const size_t at = (size_t)max(longest - 1 - j, 0) * B + col;
        v[j] = o.values[at]; s[j] = o.steps[at];
    }
    double above_v = 0.0, big = 0.0;                                                   // row t + 1's V and byte; D_{t+1}
    uint32_t above_s = 0u;
    for (int top = longest - 1; top >= 0; top -= kRows) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const size_t at = (size_t)max(top - kRows - j, 0) * B + col;
            nv[j] = o.values[at]; ns[j] = o.steps[at];
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int t = top - j;
            const bool last = t == length - 1;
            const double target = last ? 0.0 : td_target(above_s, above_v, o.gamma);
            const double delta = __dsub_rn(target, v[j]);
            const double carried = __dadd_rn(delta, __dmul_rn(gl, big));
            big = last ? ((s[j] & 0x80u) != 0u ? delta : 0.0) : carried;              // (a cut game's last move is skipped: +0.0)
            if (t >= 0 && t < length) o.deltas[(size_t)t * B + col] = big;
            above_v = v[j]; above_s = s[j];
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) { v[j] = nv[j]; s[j] = ns[j]; }
    }
}

// pulse_tfe_nt_learn's mapping and counters: blockIdx.y = t, blockIdx.x * kBlock + threadIdx.x = g
template <int IMG>
__global__ __launch_bounds__(kBlock) void tfe_nt_lambda_scatter_kernel(const PulseTfeNtLearnLambda o, const NtDev net) {
    __shared__ unsigned long long wg[3];
    if (threadIdx.x < 3) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = blockIdx.x * kBlock + threadIdx.x, t = (int)blockIdx.y;
    const size_t B = (size_t)o.n_games;
    if (g < o.n_games) {
        int length = o.lengths[g];
        length = length > o.max_steps ? o.max_steps : length;
        if (t < length) {
            const size_t at = (size_t)t * B + (size_t)g;
            const bool skip = t == length - 1 && (o.steps[at] & 0x80u) == 0u;
            if (skip) {
                atomicAdd(&wg[1], 1ull);                                                // LDS
            } else {
                bool clamp;
                const unsigned long long d = td_fixed(o.deltas[at], clamp);
                add_features<IMG>(net, reinterpret_cast<unsigned long long*>(o.acc), o.keys[at], d);
                atomicAdd(&wg[0], 1ull);
                if (clamp) atomicAdd(&wg[2], 1ull);
            }
        }
    }
    __syncthreads();
    const int i = (int)threadIdx.x;
    if (i < 3 && wg[i]) atomicAdd(reinterpret_cast<unsigned long long*>(o.stats) + (i == 0 ? 1 : i == 1 ? 2 : 4), wg[i]);
}

}  // namespace

extern "C" int pulse_tfe_nt_learn_lambda(const PulseTfeNtLearnLambda* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_lambda";
    if (!o) return fail_named(name, "options are null");
    NtDev dev;
    if (int rc = check_net(o->net, false, name, &dev)) return rc;
    if (int rc = check_batch(o, name)) return rc;
    if (!(o->lambda >= 0.0 && o->lambda <= 1.0)) return fail_named(name, "lambda must be in [0, 1]");
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->values) return fail_named(name, "values is null");
    if (!o->steps) return fail_named(name, "steps is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (!o->deltas) return fail_named(name, "deltas is null");
    if (int rc = check_acc(o->acc, name)) return rc;
    if (!o->stats) return fail_named(name, "stats is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->deltas & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / deltas / stats must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tfe_nt_lambda_walk_kernel, dim3((unsigned)((o->n_games + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, st, *o);
    const dim3 grid((unsigned)((o->n_games + kBlock - 1) / kBlock), (unsigned)o->max_steps), block(kBlock);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_lambda_scatter_kernel<8>, grid, block, 0, st, *o, dev);
    else hipLaunchKernelGGL(tfe_nt_lambda_scatter_kernel<1>, grid, block, 0, st, *o, dev);
    return finish_launch("pulse_tfe_nt_learn_lambda launch");
}
