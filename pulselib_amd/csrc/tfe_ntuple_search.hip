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

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256, kGroup = 32, kGroupsPerBlock = kBlock / kGroup;
static_assert(sizeof(PulseTfeNtSearch) == 176, "struct layouts are part of the ABI");

// the environment's tile odds (tfe_spawn_packed: the nibble is 2 iff r >> 8 > 15099494), exact doubles
constexpr double kP1 = 15099495.0 / 16777216.0, kP2 = 1677721.0 / 16777216.0;

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

__device__ __forceinline__ int count_empty(const uint64_t key) {
    return __popc(tfe_nz_nibbles((uint32_t)key) ^ 0x88888888u) + __popc(tfe_nz_nibbles((uint32_t)(key >> 32)) ^ 0x88888888u);
}

// The four q of board `key_b` (its moves ka / sc given), by the 32 lanes of its group together; s = this lane's slot.  Every lane of
// the group must call it with the same board (the butterfly is among them), and every lane returns the same q.  A move that does
// not change the board has q = +0.0.  The loop over the moves is kept rolled: one copy of the chance layer in the code.
template <int IMG>
__device__ __forceinline__ void search_q(const NtDev& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                         const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], const int s, double (&q)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = 0.0;
    const int cell4 = 4 * (s >> 1);
    const uint64_t tile = (uint64_t)((s & 1) + 1) << cell4;
    const double odds = (s & 1) ? kP2 : kP1;
#pragma unroll 1
    for (int a = 0; a < 4; ++a) {
        uint64_t kb = ka[0];
        int score = sc[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) { kb = a == i ? ka[i] : kb; score = a == i ? sc[i] : score; }
        const bool candidate = kb != key_b;                                             // (the same in the 32 lanes)
        double term = 0.0;
        if (candidate && ((kb >> cell4) & 15ull) == 0ull) {
            const uint64_t chance = kb | tile;
            uint64_t kc[4];
            int scc[4];
            moves4(chance, lut, kc, scc);
            double v[4];
            values4<IMG>(net, w, kc, v);
            double m = 0.0;
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double x = __dadd_rn((double)tfe_reward(scc[i]), __dmul_rn(gamma, v[i]));
                const bool cand = kc[i] != chance;
                m = cand && (!any || x > m) ? x : m;
                any = any || cand;
            }
            term = __dmul_rn(odds, m);
        }
#pragma unroll
        for (int d = 1; d < kGroup; d <<= 1) term = __dadd_rn(term, __shfl_xor(term, d, kGroup));
        double qa = 0.0;
        if (candidate) qa = __dadd_rn((double)tfe_reward(score), __dmul_rn(gamma, __ddiv_rn(term, (double)count_empty(kb))));
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = a == i ? qa : q[i];
    }
}

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

extern "C" int pulse_tfe_nt_search(const PulseTfeNtSearch* o, void* stream) {
    const char* name = "pulse_tfe_nt_search";
    if (!o) return fail_named(name, "options are null");
    NtDev dev;
    if (int rc = check_net(o->net, true, name, &dev)) return rc;
    if (o->n_boards < 1) return fail_named(name, "n_boards must be positive");
    if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (o->reserved0 != 0 || o->reserved1 != 0) return fail_named(name, "reserved0 / reserved1 must be 0 (zero-initialise the struct)");
    if (!o->boards) return fail_named(name, "boards is null");
    if (!o->q) return fail_named(name, "q is null");
    if (!o->action) return fail_named(name, "action is null");
    if (!o->candidates) return fail_named(name, "candidates is null");
    if (((uintptr_t)o->boards & 7u) || ((uintptr_t)o->q & 7u)) return fail_named(name, "boards / q must be 8-byte aligned");
    Boards b{o->net.weights, o->n_boards, o->gamma, o->tie_seed, o->round, o->boards, o->q, o->action, o->candidates, nullptr};
    if (int rc = pulse::tfe_row_lut(&b.lut)) return rc;
    const dim3 grid((unsigned)(((int64_t)o->n_boards + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kBlock);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search_kernel<8>, grid, block, 0, (hipStream_t)stream, b, dev);
    else hipLaunchKernelGGL(tfe_nt_search_kernel<1>, grid, block, 0, (hipStream_t)stream, b, dev);
    return finish_launch("pulse_tfe_nt_search launch");
}

extern "C" int pulse_tfe_nt_evaluate_search(const PulseTfeNtEval* o, void* stream) {
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, "pulse_tfe_nt_evaluate_search", &dev, &g)) return rc;
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kBlock);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_search_games_kernel<8>, grid, block, 0, (hipStream_t)stream, g, dev);
    else hipLaunchKernelGGL(tfe_nt_search_games_kernel<1>, grid, block, 0, (hipStream_t)stream, g, dev);
    return finish_launch("pulse_tfe_nt_evaluate_search launch");
}
