// tfe_ntuple_backed.hip -- the 2048 n-tuple network's search-backed TD targets, two entry points:
// pulse_tfe_nt_rollout_backed and pulse_tfe_nt_learn_backed (include/pulse_env.h).
//
// pulse_tfe_nt_rollout_search plays a round's games on the q of the search and then drops them: the learners bootstrap from the
// network's one-ply V of the next record.  Here a move also records the value the search backed up for the board it was made on,
// backed[t] = the largest q over the moves that change the board, and the learner's difference of a move is backed[t + 1] - V_t: the
// search's estimate, for the spawn that happened, of what V(afterstate_t) estimates.
//
// The recording kernels are tfe_ntuple_search_rollout.hip's four with Backed set (tfe_nt_play_kernel running play_game<true, true>):
// the maximum is formed from the q and the afterstates every lane of a game holds alike, and `writer` guards one more store.  The
// learner is two launches: the walk of tfe_ntuple_device.h with Backed set, which leaves D_t in deltas, and the learners' one scatter
// with the differences given (launch_scatter, or launch_scatter_tc where acc_abs is set).
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
    g.backed = backed;
    if (int rc = launch_play<true, 1, 2, true>(layers, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout_backed launch");
}

extern "C" int pulse_tfe_nt_learn_backed(const PulseTfeNtLearnBacked* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn_backed";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (int rc = check_learner(o, name, kNeedDeltas | kNeedBacked)) return rc;
    launch_walk(o, &m, stream);
    if (m.acc_abs) launch_scatter_tc(m, dev, o->net.symmetric != 0, stream);
    else launch_scatter(m, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn_backed launch");
}
