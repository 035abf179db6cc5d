// tfe_ntuple_search.hip -- the 2048 n-tuple network under expectimax search, one chance layer deep, two launches:
// pulse_tfe_nt_search (q, the greedy action and the candidates of given boards) and pulse_tfe_nt_evaluate_search (whole games under
// that policy, counted as pulse_tfe_nt_evaluate counts its own) (include/pulse_env.h).
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

constexpr int kBlock = kSearchBlock;
static_assert(sizeof(PulseTfeNtSearch) == 176, "struct layouts are part of the ABI");

// pulse_tfe_nt_search's struct as its kernel takes it
struct Boards {
    const float* weights;
    int32_t n_boards;
    double gamma;
    uint64_t tie_seed, round;
    const uint64_t* boards;
    double* q; int8_t* action; uint8_t* candidates;
    const uint32_t* lut;
};

template <int IMG>
__global__ __launch_bounds__(kBlock) void tfe_nt_search_kernel(const Boards o, const NtDev net) {
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    if (g >= o.n_boards) return;
    const uint64_t key_b = o.boards[g];
    uint64_t ka[4];
    int sc[4];
    moves4(key_b, o.lut, ka, sc);
    double q[4];
    search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
    uint32_t bits;
    const int best = greedy_of(q, key_b, ka, o.tie_seed, o.round, &bits);
    if (s == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) o.q[(size_t)g * 4 + a] = q[a];
        o.action[g] = (int8_t)best;
        o.candidates[g] = (uint8_t)bits;
    }
}

// pulse_tfe_nt_evaluate's game loop with q from the search: the 32 lanes of a group play the game alike, lane 0 writes and counts
template <int IMG>
__global__ __launch_bounds__(kBlock) void tfe_nt_search_games_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[kEvalBins];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    play_game<false>(o, wg, g, s == 0,
                     [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&)[4], double (&q)[4]) {
                         search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                     });
}

}  // namespace

// the launches (tfe_ntuple_search_device.h): pulse_tfe_nt_search_deep and pulse_tfe_nt_evaluate_search_deep take them at one layer
namespace pulse_tfe {

void launch_search(const PulseTfeNtSearch& o, const NtDev& dev, const uint32_t* lut, void* stream) {
    const Boards b{o.net.weights, o.n_boards, o.gamma, o.tie_seed, o.round, o.boards, o.q, o.action, o.candidates, lut};
    const dim3 grid((unsigned)(((int64_t)o.n_boards + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kBlock);
    if (o.net.symmetric) hipLaunchKernelGGL(tfe_nt_search_kernel<8>, grid, block, 0, (hipStream_t)stream, b, dev);
    else hipLaunchKernelGGL(tfe_nt_search_kernel<1>, grid, block, 0, (hipStream_t)stream, b, dev);
}

void launch_search_games(const Games& g, const NtDev& dev, const bool symmetric, void* stream) {
    const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kBlock);
    if (symmetric) hipLaunchKernelGGL(tfe_nt_search_games_kernel<8>, grid, block, 0, (hipStream_t)stream, g, dev);
    else hipLaunchKernelGGL(tfe_nt_search_games_kernel<1>, grid, block, 0, (hipStream_t)stream, g, dev);
}

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
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    launch_search_games(g, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_evaluate_search launch");
}
