// tfe_ntuple_search_deep.hip -- the 2048 n-tuple network under expectimax search two chance layers deep, two
// launches: pulse_tfe_nt_search_deep and pulse_tfe_nt_evaluate_search_deep (include/pulse_env.h).  At layers = 1 they launch the
// kernels of tfe_ntuple_search.hip; the kernels here are those of layers = 2: the board kernel below and tfe_nt_play_kernel
// (tfe_ntuple_search_device.h) at 256 lanes per game.
//
// q_a = r_a + gamma * E_a as in section 13.1, with the best q of the ONE-LAYER search of the board after the spawn where that section
// has its best one-ply value.  One board or game per workgroup of 256 lanes = 8 groups of 32.  The live children (a, slot) of the
// board -- a candidate move and an empty cell of B_a with one of the two tiles -- are counted from the empty-cell masks of the four
// B_a, numbered a-major and slot-ascending, and dealt to the groups in turn: child n goes to group n % 8.  A group forms the chance
// board C, makes its four moves and runs search_q on it -- the one copy of the chance layer, lane s owning slot s of C's move in
// hand -- takes the scan-maximum over C's candidates, and its lane 0 stores P_k * W2(C) into terms[a][slot] in LDS.  After a
// workgroup barrier every group reads the four rows -- +0.0 where the slot is not live, so the rows are never cleared -- and sums each
// by the xor butterfly among its 32 lanes: every lane of the workgroup holds the same four q.  Every lane carries the board, the
// draws and the four moves alike; they depend on blockIdx alone.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

// one board per workgroup; o: the entry point's struct as it came, after the checks
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search2_kernel(const PulseTfeNtSearch o, const NtDev net, const uint32_t* __restrict__ lut) {
    __shared__ double terms[4 * kGroup];
    const int g = (int)blockIdx.x;                                                      // (grid = n_boards)
    const uint64_t key_b = o.boards[g];
    uint64_t ka[4];
    int sc[4];
    moves4(key_b, lut, ka, sc);
    double q[4];
    search_q2<IMG>(net, o.net.weights, lut, o.gamma, key_b, ka, sc, terms, q);
    uint32_t bits;
    const int best = greedy_of(q, key_b, ka, o.tie_seed, o.round, &bits);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) o.q[(size_t)g * 4 + a] = q[a];
        o.action[g] = (int8_t)best;
        o.candidates[g] = (uint8_t)bits;
    }
}

}  // namespace

extern "C" int pulse_tfe_nt_search_deep(const PulseTfeNtSearch* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_search_deep";
    NtDev dev;
    const uint32_t* lut = nullptr;
    if (int rc = check_search(o, name, &dev)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    if (layers == 1) {
        launch_search(*o, dev, lut, stream);
    } else {
        const dim3 grid((unsigned)o->n_boards), block(kSearchBlock);
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search2_kernel<8>, grid, block, 0, (hipStream_t)stream, *o, dev, lut);
        else hipLaunchKernelGGL(tfe_nt_search2_kernel<1>, grid, block, 0, (hipStream_t)stream, *o, dev, lut);
    }
    return finish_launch("pulse_tfe_nt_search_deep launch");
}

extern "C" int pulse_tfe_nt_evaluate_search_deep(const PulseTfeNtEval* o, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_search_deep";
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = check_layers(layers, name)) return rc;
    if (int rc = layers == 1 ? launch_search_games(g, dev, o->net.symmetric != 0, stream) : launch_play<false, 2, 2>(2, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate_search_deep launch");
}
