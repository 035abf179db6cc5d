// tfe_ntuple_search.hip -- the 2048 n-tuple network under expectimax search: q, the greedy action and the candidates of given boards
// (pulse_tfe_nt_search*) and whole games under that policy, counted as pulse_tfe_nt_evaluate counts its own
// (pulse_tfe_nt_evaluate_search*), at three depths: one chance layer, one or two as the caller says (_deep,
// section 13.4), one or two as the board's empty cells say (_adaptive, section 13.11) (include/pulse_env.h).  The kernels are
// tfe_ntuple_search_device.h's tfe_nt_search_kernel and tfe_nt_play_kernel, instantiated here on the one-stage network at 32 lanes per
// board or game, at 256, and at 256 on NtAdaptiveDev.
//
// One layer.  q_a = r_a + gamma * E_a, E_a = the mean over the empty cells of B_a and the two tiles of the best one-ply value of the
// board after the spawn.  32 lanes play one board (two boards per wavefront, eight per workgroup): lane s owns the chance board of slot
// s = 2 * cell + (tile - 1) of the move in hand, makes its four moves, reads their values (values4, 4 F gathers) and takes the
// maximum; the 32 terms meet in an xor butterfly (five __shfl_xor of width 32), which is the order the definition sums in and
// leaves the sum in every lane.  The board, the draws and the four moves are carried by all 32 lanes alike, so the game loop has
// no broadcast, and the network's words stay scalar.  Two games of a wavefront differ in length: the one still playing shuffles
// among its own 32 lanes only, which are active together.
//
// Two layers.  q_a = r_a + gamma * E_a as above, with the best q of the ONE-LAYER search of the board after the spawn where one layer
// has its best one-ply value.  One board or game per workgroup of 256 lanes = 8 groups of 32.  The live children (a, slot) of the
// board -- a candidate move and an empty cell of B_a with one of the two tiles -- are counted from the empty-cell masks of the four
// B_a, numbered a-major and slot-ascending, and dealt to the groups in turn: child n goes to group n % 8.  A group forms the chance
// board C, makes its four moves and runs search_q on it -- the one copy of the chance layer, lane s owning slot s of C's move in
// hand -- takes the scan-maximum over C's candidates, and its lane 0 stores P_k * W2(C) into terms[a][slot] in LDS.  After a
// workgroup barrier every group reads the four rows -- +0.0 where the slot is not live, so the rows are never cleared -- and sums each
// by the xor butterfly among its 32 lanes: every lane of the workgroup holds the same four q.  Every lane carries the board, the
// draws and the four moves alike; they depend on blockIdx alone.
//
// The depth the board chooses.  For the board B a move is made from, n = its empty cells: with n <= deep_empty_max the four q are
// those of the two-layer search (search_q2), otherwise those of the one-layer search (search_q), bit for bit.  One board or game per
// workgroup of 256 lanes, the two-layer mapping.  A deep move runs search_q2 as it stands.  On a shallow move the four candidate
// moves go side by side: group a < 4 runs the chance layer of move a (search_q_move, the one copy) and its lane 0 stores q_a into
// four doubles of LDS of their own; groups 4..7 only meet the barriers; after a workgroup barrier every lane reads the four q.  n
// depends on the board alone, which the 256 lanes carry alike, so they take the branch alike and nothing lane-dependent encloses a
// barrier (search_q_adaptive).  The game kernel is play_game, untouched, under that q; the closure counts the moves at each depth
// and thread 0 adds the two counts once, at the game's end.
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

// what the three board launches do after their checks
template <class Net>
int search_boards(const int layers, const PulseTfeNtSearch& o, const Net& net, void* stream, const char* what) {
    const uint32_t* lut = nullptr;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    launch_boards(layers, o, net, lut, stream);
    return finish_launch(what);
}

}  // namespace

extern "C" int pulse_tfe_nt_search(const PulseTfeNtSearch* o, void* stream) {
    NtDev dev;
    if (int rc = check_search(o, "pulse_tfe_nt_search", &dev)) return rc;
    return search_boards(1, *o, dev, stream, "pulse_tfe_nt_search launch");
}

extern "C" int pulse_tfe_nt_search_deep(const PulseTfeNtSearch* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_search_deep";
    NtDev dev;
    if (int rc = check_search(o, name, &dev)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    return search_boards(layers, *o, dev, stream, "pulse_tfe_nt_search_deep launch");
}

extern "C" int pulse_tfe_nt_search_adaptive(const PulseTfeNtSearch* o, int32_t deep_empty_max, void* stream) {
    const char* name = "pulse_tfe_nt_search_adaptive";
    NtDev dev;
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_deep_empty_max(deep_empty_max, name)) return rc;     // (before the struct's: a threshold in range is seen to pass)
    if (int rc = check_search(o, name, &dev)) return rc;
    return search_boards(2, *o, adaptive_of(dev, deep_empty_max, nullptr), stream, "pulse_tfe_nt_search_adaptive launch");
}

extern "C" int pulse_tfe_nt_evaluate_search(const PulseTfeNtEval* o, void* stream) {
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, "pulse_tfe_nt_evaluate_search", &dev, &g)) return rc;
    if (int rc = launch_play<false, 1, 2>(1, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_search launch");
}

extern "C" int pulse_tfe_nt_evaluate_search_deep(const PulseTfeNtEval* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_search_deep";
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (int rc = launch_play<false, 1, 2>(layers, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_search_deep launch");
}

extern "C" int pulse_tfe_nt_evaluate_search_adaptive(const PulseTfeNtEval* o, int32_t deep_empty_max, int64_t* depth_stats, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_search_adaptive";
    NtDev dev;
    Games g;
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_deep_empty_max(deep_empty_max, name)) return rc;     // (these two before the struct's, as above)
    if ((uintptr_t)depth_stats & 7u) return fail_named(name, "depth_stats must be 8-byte aligned");
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = launch_play<false, 2, 2>(2, g, adaptive_of(dev, deep_empty_max, depth_stats), o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_search_adaptive launch");
}
