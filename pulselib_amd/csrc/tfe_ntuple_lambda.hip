// tfe_ntuple_lambda.hip -- the 2048 n-tuple network's TD(lambda) learner, one entry point and two launches:
// pulse_tfe_nt_learn_lambda (include/pulse_env.h).  This unit instantiates the first launch's kernel (tfe_ntuple_device.h:
// tfe_nt_lambda_walk_kernel<false>; tfe_ntuple_backed.hip runs the same text on other targets); the second is tfe_ntuple.hip's.
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

static_assert(sizeof(PulseTfeNtLearnLambda) == 192, "struct layouts are part of the ABI");

}  // namespace

namespace pulse_tfe {

void launch_lambda_walk(const PulseTfeNtLearnLambda& o, void* stream) {
    hipLaunchKernelGGL(tfe_nt_lambda_walk_kernel<false>, dim3((unsigned)((o.n_games + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, (hipStream_t)stream, o);
}

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_learn_lambda(const PulseTfeNtLearnLambda* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_lambda";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (int rc = check_learner(o, name, kNeedDeltas)) return rc;
    launch_walk(o, &m, stream);
    launch_scatter(m, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn_lambda launch");
}
