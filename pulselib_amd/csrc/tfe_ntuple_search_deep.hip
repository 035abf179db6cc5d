// tfe_ntuple_search_deep.hip -- the 2048 n-tuple network under expectimax search two chance layers deep, two
// launches: pulse_tfe_nt_search_deep and pulse_tfe_nt_evaluate_search_deep (include/pulse_env.h).  At layers = 1 they launch the
// kernels of tfe_ntuple_search.hip; the kernels here are those of layers = 2.
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

// bit s of the result: slot s of B_a = kb holds a child (the cell 2 s and 2 s + 1 share is empty); 0 for a move that is no candidate
__device__ __forceinline__ uint32_t live_slots(const uint64_t kb, const uint64_t key_b) {
    const uint32_t lo = tfe_nz_nibbles((uint32_t)kb) ^ 0x88888888u, hi = tfe_nz_nibbles((uint32_t)(kb >> 32)) ^ 0x88888888u;   // bit 4 c + 3: cell c is empty
    uint32_t m = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        m |= ((lo >> (4 * c + 3)) & 1u) * (3u << (2 * c));
        m |= ((hi >> (4 * c + 3)) & 1u) * (3u << (2 * c + 16));
    }
    return kb != key_b ? m : 0u;
}

// the position of set bit number k (from 0, upwards) of m; k < popc(m)
__device__ __forceinline__ int nth_set_bit(uint32_t m, int k) {
    int pos = 0;
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        const int c = __popc(m & ((1u << w) - 1u));
        const bool up = k >= c;
        k = up ? k - c : k;
        m = up ? m >> w : m;
        pos = up ? pos + w : pos;
    }
    return pos;
}

// The four q of board `key_b` (its moves ka / sc given) under two chance layers, by the 256 lanes of the workgroup together.  Every
// lane of the workgroup must call it, with the same board, the same number of times (two workgroup barriers a call); every lane
// returns the same q.  terms: 4 * 32 doubles of LDS, which need no initial value.
template <int IMG>
__device__ __forceinline__ void search_q2(const NtDev& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                          const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double* terms, double (&q)[4]) {
    const int group = (int)threadIdx.x >> 5, s = (int)threadIdx.x & (kGroup - 1);
    uint32_t live[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) live[a] = live_slots(ka[a], key_b);
    const int n0 = __popc(live[0]), n1 = n0 + __popc(live[1]), n2 = n1 + __popc(live[2]), total = n2 + __popc(live[3]);
    __syncthreads();                                                                    // the rows of the call before have been read
#pragma unroll 1
    for (int n = group; n < total; n += kGroupsPerBlock) {                              // (the same in the 32 lanes of a group)
        const int a = (n >= n0) + (n >= n1) + (n >= n2);
        const int k = n - (a == 0 ? 0 : a == 1 ? n0 : a == 2 ? n1 : n2);
        uint64_t kb = ka[0];
        uint32_t m = live[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) { kb = a == i ? ka[i] : kb; m = a == i ? live[i] : m; }
        const int slot = nth_set_bit(m, k);
        const uint64_t chance = kb | (uint64_t)((slot & 1) + 1) << (4 * (slot >> 1));
        uint64_t kc[4];
        int scc[4];
        moves4(chance, lut, kc, scc);
        double qc[4];
        search_q<IMG>(net, w, lut, gamma, chance, kc, scc, s, qc);
        double best = 0.0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool cand = kc[i] != chance;
            best = cand && (!any || qc[i] > best) ? qc[i] : best;
            any = any || cand;
        }
        if (s == 0) terms[a * kGroup + slot] = __dmul_rn((slot & 1) ? kP2 : kP1, best);  // (a, slot) < 4 * 32: inside the rows
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double term = (live[a] >> s) & 1u ? terms[a * kGroup + s] : 0.0;
#pragma unroll
        for (int d = 1; d < kGroup; d <<= 1) term = __dadd_rn(term, __shfl_xor(term, d, kGroup));
        q[a] = 0.0;
        if (ka[a] != key_b) q[a] = __dadd_rn((double)tfe_reward(sc[a]), __dmul_rn(gamma, __ddiv_rn(term, (double)count_empty(ka[a]))));
    }
}

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

// pulse_tfe_nt_evaluate's game loop with q from the two-layer search, one game per workgroup: g is blockIdx.x, so the 256 lanes play
// the game alike -- the same boards, draws and length -- and reach search_q2's barriers together; lane 0 writes and counts
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search2_games_kernel(const Games o, const NtDev net) {
    __shared__ unsigned long long wg[kEvalBins];
    __shared__ double terms[4 * kGroup];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    play_game<false>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                     [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&)[4], double (&q)[4]) {
                         search_q2<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, terms, q);
                     });
}

int check_layers(const int32_t layers, const char* name) {
    return layers == 1 || layers == 2 ? 0 : fail_named(name, "layers must be 1 or 2");
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
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    if (layers == 1) {
        launch_search_games(g, dev, o->net.symmetric != 0, stream);
    } else {
        const dim3 grid((unsigned)g.n_games), block(kSearchBlock);
        if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search2_games_kernel<8>, grid, block, 0, (hipStream_t)stream, g, dev);
        else hipLaunchKernelGGL(tfe_nt_search2_games_kernel<1>, grid, block, 0, (hipStream_t)stream, g, dev);
    }
    return finish_launch("pulse_tfe_nt_evaluate_search_deep launch");
}
