// tfe_ntuple_tc.hip -- the 2048 n-tuple network's temporal-coherence step sizes, two entry points:
// pulse_tfe_nt_learn_tc and pulse_tfe_nt_apply_tc (include/pulse_env.h).
//
// Every weight carries the running sum of its rounds' mean errors, E, and of their mean absolute errors, A, and moves by
// step * rho, rho = |E| / A: a weight whose errors keep their sign keeps the full step, one whose errors cancel stands still.  The
// learn launch is the learners' one scatter text (tfe_ntuple_device.h: tfe_nt_scatter_kernel) with its third accumulator,
// acc_abs += |d|, behind tfe_ntuple_lambda.hip's walk where lambda > 0; the apply launch is this unit's one kernel of its own.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256;
static_assert(sizeof(PulseTfeNtLearnTc) == 200 && sizeof(PulseTfeNtApplyTc) == 160, "struct layouts are part of the ABI");

// One lane per weight.  A weight no move visited leaves after the one 16-byte load; a visited one reads its third accumulator, E
// and A, takes rho from E and A as they stood, moves, and adds the round's means to them.  wg: the workgroup's count of weights
// moved and the sum of their rho as 32.32 fixed point -- integers, so tc_stats does not depend on scheduling.
__global__ __launch_bounds__(kBlock) void tfe_nt_tc_apply_kernel(float* __restrict__ weights, longlong2* __restrict__ acc, long long* __restrict__ acc_abs,
                                                                  double* __restrict__ e, double* __restrict__ a, unsigned long long* __restrict__ tc_stats,
                                                                  uint64_t n_weights, double step) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_weights) {
        const longlong2 s = acc[i];                                                     // {sum, cnt}
        if (s.y > 0) {
            const double cnt = (double)s.y, unit = 1.0 / (double)(1 << PULSE_TFE_NT_FRAC_BITS);
            const double mean = __dmul_rn(__ddiv_rn((double)s.x, cnt), unit);
            const double mean_abs = __dmul_rn(__ddiv_rn((double)acc_abs[i], cnt), unit);
            const double E = e[i], A = a[i];
            const double rho = A > 0.0 ? __ddiv_rn(fabs(E), A) : 1.0;                   // before this round's E and A
            weights[i] = (float)__dadd_rn((double)weights[i], __dmul_rn(__dmul_rn(step, rho), mean));
            e[i] = __dadd_rn(E, mean);
            a[i] = __dadd_rn(A, mean_abs);
            acc[i] = make_longlong2(0, 0);
            acc_abs[i] = 0;
            atomicAdd(&wg[0], 1ull);                                                    // LDS
            atomicAdd(&wg[1], (unsigned long long)llrint(ldexp(rho, 32)));              // (|E| <= A: rho is in [0, 1])
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && wg[threadIdx.x]) atomicAdd(tc_stats + threadIdx.x, wg[threadIdx.x]);
}

}  // namespace

namespace pulse_tfe {

// launch_scatter's counterpart with the third accumulator (declared in tfe_ntuple_device.h: pulse_tfe_nt_learn_backed launches it too)
void launch_scatter_tc(const Moves& m, const NtDev& dev, bool symmetric, void* stream) { launch_scatter_as<true>(m, dev, symmetric, stream); }

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_learn_tc(const PulseTfeNtLearnTc* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_tc";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (int rc = check_learner(o, name, kNeedAccAbs)) return rc;
    launch_walk(o, &m, stream);
    launch_scatter_tc(m, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn_tc launch");
}

extern "C" int pulse_tfe_nt_apply_tc(const PulseTfeNtApplyTc* o, void* stream) {
    const char* name = "pulse_tfe_nt_apply_tc";
    if (!o) return fail_named(name, "options are null");
    NtDev dev;
    if (int rc = check_net(o->net, true, name, &dev)) return rc;
    if (!(o->step > 0.0 && o->step <= 1.0)) return fail_named(name, "step must be in (0, 1]");
    if (int rc = check_acc(o->acc, name)) return rc;
    if (!o->acc_abs) return fail_named(name, "acc_abs is null");
    if (!o->e) return fail_named(name, "e is null");
    if (!o->a) return fail_named(name, "a is null");
    if (!o->tc_stats) return fail_named(name, "tc_stats is null");
    if (((uintptr_t)o->acc_abs & 7u) || ((uintptr_t)o->e & 7u) || ((uintptr_t)o->a & 7u) || ((uintptr_t)o->tc_stats & 7u))
        return fail_named(name, "acc_abs / e / a / tc_stats must be 8-byte aligned");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    const dim3 grid((unsigned)((o->net.n_weights + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(tfe_nt_tc_apply_kernel, grid, block, 0, (hipStream_t)stream, o->net.weights, reinterpret_cast<longlong2*>(o->acc),
                       reinterpret_cast<long long*>(o->acc_abs), o->e, o->a, reinterpret_cast<unsigned long long*>(o->tc_stats), o->net.n_weights, o->step);
    return finish_launch("pulse_tfe_nt_apply_tc launch");
}
