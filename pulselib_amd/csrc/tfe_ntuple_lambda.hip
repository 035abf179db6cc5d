// tfe_ntuple_lambda.hip -- the 2048 n-tuple network's TD(lambda) learner, one entry point and two launches:
// pulse_tfe_nt_learn_lambda (include/pulse_env.h).  This unit holds the first launch's kernel; the second is tfe_ntuple.hip's.
// launch_lambda_walk is that first launch alone, which pulse_tfe_nt_learn_tc (tfe_ntuple_tc.hip) runs too.
//
// The roll-out recorded per move the afterstate's key, its V as float64, the reward and the terminal bit, so the lambda-differences
// are one backward recurrence per game over data already in memory: D_t = delta_t + (gamma * lambda) * D_{t+1}.  The first kernel
// walks every game from its end, one lane per game, and writes D_t step-major beside the values; the second is pulse_tfe_nt_learn's
// scatter (tfe_nt_scatter_kernel through launch_scatter), one lane per recorded move, with D_t read instead of formed.  The recurrence carries the unclamped D; a move's add is clamped.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kWalkBlock = 64, kRows = 8;
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

}  // namespace

namespace pulse_tfe {

void launch_lambda_walk(const PulseTfeNtLearnLambda& o, void* stream) {
    hipLaunchKernelGGL(tfe_nt_lambda_walk_kernel, dim3((unsigned)((o.n_games + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, (hipStream_t)stream, o);
}

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_learn_lambda(const PulseTfeNtLearnLambda* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_lambda";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (!(o->lambda >= 0.0 && o->lambda <= 1.0)) return fail_named(name, "lambda must be in [0, 1]");
    if (!o->deltas) return fail_named(name, "deltas is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->deltas & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / deltas / stats must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    launch_lambda_walk(*o, stream);
    m.deltas = o->deltas;
    launch_scatter(m, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn_lambda launch");
}
