// tfe_ntuple_search_rollout.hip -- the 2048 n-tuple network's training roll-out under expectimax search, two launches
// (include/pulse_env.h): pulse_tfe_nt_rollout_search and pulse_tfe_nt_rollout_adaptive (section 13.13).
// pulse_tfe_nt_rollout's games, draws and records with the greedy action taken on the q of the search: one chance layer deep (section
// 13.1) or two (section 13.4) as the caller says, or as the board's empty cells say (section 13.11: pulse_tfe_nt_evaluate_search_adaptive's
// policy -- two layers on a board with at most deep_empty_max empty cells, one on the others).
//
// The game loop is play_game<true, ...>, as tfe_ntuple.hip's roll-out runs it, in tfe_nt_play_kernel (tfe_ntuple_search_device.h) with
// Record set; the mapping of a game to lanes is the evaluation's under the same policy: 32 lanes per game at one layer, a workgroup
// of 256 at two and at the adaptive depth.  What is recorded beside the key and the byte is the NETWORK's V of the chosen afterstate,
// not the search's backed-up value.  The adaptive launch also records, where asked, pulse_tfe_nt_rollout_backed's value (section
// 13.6) of the q at the depth the board chose, starts, where asked, from the boards of `start` (section 13.7), and counts the moves at
// each depth as the evaluation does.
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

}  // namespace

extern "C" int pulse_tfe_nt_rollout_search(const PulseTfeNtRollout* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_rollout_search";
    NtDev dev;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (int rc = launch_play<true, 1, 2>(layers, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout_search launch");
}

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
    if (int rc = launch_play_from<2, 2, false>(2, g, backed, start, adaptive_of(dev, deep_empty_max, depth_stats), o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout_adaptive launch");
}
