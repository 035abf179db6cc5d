// tfe_ntuple_search.hip -- the 2048 n-tuple network under expectimax search, one chance layer deep, two launches:
// pulse_tfe_nt_search (q, the greedy action and the candidates of given boards) and pulse_tfe_nt_evaluate_search (whole games under
// that policy, counted as pulse_tfe_nt_evaluate counts its own) (include/pulse_env.h).  The kernels are tfe_ntuple_search_device.h's
// tfe_nt_search_kernel and tfe_nt_play_kernel at 32 lanes per game, instantiated here on the one-stage network.
//
// q_a = r_a + gamma * E_a, E_a = the mean over the empty cells of B_a and the two tiles of the best one-ply value of the board after
// the spawn.  32 lanes play one board (two boards per wavefront, eight per workgroup): lane s owns the chance board of slot
// s = 2 * cell + (tile - 1) of the move in hand, makes its four moves, reads their values (values4, 4 F gathers) and takes the
// maximum; the 32 terms meet in an xor butterfly (five __shfl_xor of width 32), which is the order the definition sums in and
// leaves the sum in every lane.  The board, the draws and the four moves are carried by all 32 lanes alike, so the game loop has
// no broadcast, and the network's words stay scalar.  Two games of a wavefront differ in length: the one still playing shuffles
// among its own 32 lanes only, which are active together.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

static_assert(sizeof(PulseTfeNtSearch) == 176, "struct layouts are part of the ABI");

}  // namespace

// the launches (tfe_ntuple_search_device.h): pulse_tfe_nt_search_deep and pulse_tfe_nt_evaluate_search_deep take them at one layer
namespace pulse_tfe {

void launch_search(const PulseTfeNtSearch& o, const NtDev& dev, const uint32_t* lut, void* stream) { launch_boards(o, dev, lut, stream); }

int launch_search_games(Games& g, const NtDev& dev, const bool symmetric, void* stream) { return launch_play<false, 1, 1>(1, g, dev, symmetric, stream); }

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_search(const PulseTfeNtSearch* o, void* stream) {
    NtDev dev;
    const uint32_t* lut = nullptr;
    if (int rc = check_search(o, "pulse_tfe_nt_search", &dev)) return rc;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    launch_search(*o, dev, lut, stream);
    return finish_launch("pulse_tfe_nt_search launch");
}

extern "C" int pulse_tfe_nt_evaluate_search(const PulseTfeNtEval* o, void* stream) {
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, "pulse_tfe_nt_evaluate_search", &dev, &g)) return rc;
    if (int rc = launch_search_games(g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_search launch");
}
