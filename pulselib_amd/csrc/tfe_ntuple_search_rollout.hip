// tfe_ntuple_search_rollout.hip -- the 2048 n-tuple network's training roll-out under expectimax search, one
// launch: pulse_tfe_nt_rollout_search (include/pulse_env.h).  pulse_tfe_nt_rollout's games, draws and records with the greedy
// action taken on the q of the search, one chance layer deep (section 13.1) or two (section 13.4).
//
// The game loop is play_game<true>, as tfe_ntuple.hip's roll-out runs it, in tfe_nt_play_kernel (tfe_ntuple_search_device.h) with
// Record set; the mapping of a game to lanes is the evaluation's under the same policy: 32 lanes per game at one layer, a workgroup
// of 256 at two.  What is recorded beside the key and the byte is the NETWORK's V of the chosen afterstate, not the search's
// backed-up value.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::finish_launch;

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
