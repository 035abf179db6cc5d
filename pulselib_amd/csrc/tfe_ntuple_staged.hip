// tfe_ntuple_staged.hip -- the 2048 n-tuple network with weight sets by tile stage (multi-stage TD), four entry
// points: pulse_tfe_nt_rollout_staged, pulse_tfe_nt_learn_staged, pulse_tfe_nt_evaluate_staged and pulse_tfe_nt_search_staged
// (include/pulse_env.h).
//
// One table has to serve the openings and the boards with a 2,048 tile on them alike.  Here the network is S copies of its tables and
// a board reads, and a recorded move adds to, the copy of its stage: the number of thresholds the board's largest nibble has reached.
// The stage is an offset on a feature's index (tfe_ntuple_device.h: NtStagedDev, stage_of, stage_base), so nothing else of the
// network's units is new: the game loop (play_game), the chance layer (search_q), V of four afterstates (values4), the adds
// (add_features inside scatter_moves), the greedy scan and the kernels around them (tfe_nt_play_kernel at one lane and at 32 per game,
// tfe_nt_search_kernel, tfe_nt_scatter_kernel) are the one copy each, instantiated here on the staged network; what this file holds
// is the checks of the stages.  The stage of a key is about thirty integer operations on its two halves beside the few hundred of
// its feature indices; values4 forms the four stages once, before its loop over the tuples.  The backward walks touch neither weights
// nor features and are the launches they were, and so are the apply launches, called once per stage on that stage's slices.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

static_assert(sizeof(PulseTfeNtStages) == 16 && sizeof(PulseTfeNtLearnBacked) == 208 && sizeof(PulseTfeNtRollout) == 232 && sizeof(PulseTfeNtEval) == 208 &&
              sizeof(PulseTfeNtSearch) == 176, "struct layouts are part of the ABI");
static_assert(sizeof(NtStagedDev) == sizeof(NtDev) + 16, "the staged network is the network and four words");

// The checks of the stages, after those of the network; fills the kernels' form of the staged network from that of the network.
int check_stages(const PulseTfeNtStages* s, const PulseTfeNtNet& n, const NtDev& dev, const char* name, NtStagedDev* out) {
    if (!s) return fail_named(name, "stages are null");
    if (s->n_stages < 1 || s->n_stages > PULSE_TFE_NT_MAX_STAGES) return fail_named(name, "n_stages must be in 1..4");
    if (s->reserved0 != 0) return fail_named(name, "stages.reserved0 must be 0 (zero-initialise the struct)");
    *out = NtStagedDev{};
    static_cast<NtDev&>(*out) = dev;
    int below = 0;
    for (int i = 0; i < 4; ++i) {
        const int th = s->threshold[i];
        if (i >= s->n_stages - 1) {
            if (th != 0) return fail_named(name, "a threshold at or beyond n_stages - 1 must be 0");
            continue;
        }
        if (th < 1 || th > 15) return fail_named(name, "a threshold must be a nibble in 1..15");
        if (th <= below) return fail_named(name, "the thresholds must be strictly increasing");
        below = th;
        out->reach[i] = (uint32_t)(16 - th) * 0x01010101u;
    }
    out->n_weights = (uint32_t)n.n_weights;                                             // (check_net: at most 8 * 16^6 = 2^27, so 4 stages end at 2^29)
    return 0;
}

constexpr const char* kStagedLayers = "layers must be 0 or 1 (two layers are not built on stages)";

}  // namespace

extern "C" int pulse_tfe_nt_rollout_staged(const PulseTfeNtRollout* o, const PulseTfeNtStages* stages, int32_t layers, double* backed, uint64_t* start,
                                           void* stream) {
    const char* name = "pulse_tfe_nt_rollout_staged";
    NtDev dev;
    NtStagedDev net;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = check_start(layers, backed, start, name, kStagedLayers)) return rc;
    if (int rc = launch_play_from<0, 1, true>(layers, g, backed, start, net, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout_staged launch");
}

extern "C" int pulse_tfe_nt_learn_staged(const PulseTfeNtLearnBacked* o, const PulseTfeNtStages* stages, void* stream) {
    const char* name = "pulse_tfe_nt_learn_staged";
    NtDev dev;
    NtStagedDev net;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = check_learner(o, name, 0u)) return rc;
    launch_walk(o, &m, stream);
    if (m.acc_abs) launch_scatter_as<true>(m, net, o->net.symmetric != 0, stream);
    else launch_scatter_as<false>(m, net, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn_staged launch");
}

extern "C" int pulse_tfe_nt_evaluate_staged(const PulseTfeNtEval* o, const PulseTfeNtStages* stages, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_staged";
    NtDev dev;
    NtStagedDev net;
    Games g;
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (layers != 0 && layers != 1) return fail_named(name, kStagedLayers);
    if (int rc = launch_play<false, 0, 1>(layers, g, net, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_staged launch");
}

extern "C" int pulse_tfe_nt_search_staged(const PulseTfeNtSearch* o, const PulseTfeNtStages* stages, void* stream) {
    const char* name = "pulse_tfe_nt_search_staged";
    NtDev dev;
    NtStagedDev net;
    const uint32_t* lut = nullptr;
    if (int rc = check_search(o, name, &dev)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    launch_boards(1, *o, net, lut, stream);
    return finish_launch("pulse_tfe_nt_search_staged launch");
}
