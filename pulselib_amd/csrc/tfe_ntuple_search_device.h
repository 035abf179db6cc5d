// tfe_ntuple_search_device.h -- what the two units of the n-tuple network's expectimax play share (tfe_ntuple_search.hip: one chance
// layer; tfe_ntuple_search_deep.hip: two, section 13.4): the group of 32 lanes, the tile odds, the board
// launch's refusals (check_search), the chance layer itself (search_q) and the launches of the one-layer
// kernels.  One copy each.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace pulse_tfe {

constexpr int kSearchBlock = 256, kGroup = 32, kGroupsPerBlock = kSearchBlock / kGroup;

// the environment's tile odds (tfe_spawn_packed: the nibble is 2 iff r >> 8 > 15099494), exact doubles
constexpr double kP1 = 15099495.0 / 16777216.0, kP2 = 1677721.0 / 16777216.0;

// what pulse_tfe_nt_search and pulse_tfe_nt_search_deep refuse; fills the kernels' form of the network
inline int check_search(const PulseTfeNtSearch* o, const char* name, NtDev* dev) {
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_net(o->net, true, name, dev)) return rc;
    if (o->n_boards < 1) return fail_named(name, "n_boards must be positive");
    if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (o->reserved0 != 0 || o->reserved1 != 0) return fail_named(name, "reserved0 / reserved1 must be 0 (zero-initialise the struct)");
    if (!o->boards) return fail_named(name, "boards is null");
    if (!o->q) return fail_named(name, "q is null");
    if (!o->action) return fail_named(name, "action is null");
    if (!o->candidates) return fail_named(name, "candidates is null");
    if (((uintptr_t)o->boards & 7u) || ((uintptr_t)o->q & 7u)) return fail_named(name, "boards / q must be 8-byte aligned");
    return 0;
}

// The launches of the one-layer kernels (defined in tfe_ntuple_search.hip, where the kernels are), after the checks: of the boards
// of `o` with the row table `lut`, and of the games `g` (g.lut set)
void launch_search(const PulseTfeNtSearch& o, const NtDev& dev, const uint32_t* lut, void* stream);
void launch_search_games(const Games& g, const NtDev& dev, bool symmetric, void* stream);

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

}  // namespace pulse_tfe
