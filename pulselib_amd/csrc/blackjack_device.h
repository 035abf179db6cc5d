// blackjack_device.h -- device code shared by the Blackjack env kernels (envs.hip) and the fused first-visit Monte-Carlo
// roll-out (blackjack_mc.hip): the deck shuffle (on the library's Philox4x32-10, philox_device.h) and the card arithmetic of
// environments/blackjack/blackjack.py (cited as :line).  Both translation units play the same game from the same
// (seed, game, episode) because they run these functions, not restatements of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox_device.h"

namespace pulse_bj {

using pulse_philox::U4;
using pulse_philox::philox4x32;
using pulse_philox::u4_word;

__device__ __forceinline__ int bj_rank(int card) { const int r = card % 13 + 1; return r > 10 ? 10 : r; }

// The deck of game g in episode `episode`: Fisher-Yates with Philox draws (replaces argsort(rand), :24-29); swap q takes word
// q & 3 of Philox4x32-10(seed, g, episode * 16 + (q >> 2)) -- offsets episode * 16 + 0..12.  d: 52 bytes of the lane's own.
// (CheapDraws: diagnostic twin builds only -- `make bjmc-ablate` -- price the generator by putting a two-instruction hash in its place.)
template <bool CheapDraws = false>
__device__ __forceinline__ void bj_shuffle(uint8_t* d, uint64_t seed, uint64_t g, uint64_t episode) {
    for (int c = 0; c < 52; ++c) d[c] = (uint8_t)c;
    for (int call = 0, i = 51; call < 13; ++call) {                  // one generator call per four swaps
        const U4 r = CheapDraws ? U4{0u, 0u, 0u, 0u} : philox4x32(seed, g, episode * 16 + (uint64_t)call);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (i > 0) {                                             // swap q = 4 * call + b, i = 51 - q
                const uint32_t w = CheapDraws ? ((uint32_t)g * 0x9E3779B9u + (uint32_t)episode * 0x85EBCA6Bu + (uint32_t)i * 0xC2B2AE35u) * 0x27D4EB2Fu
                                              : u4_word(r, b);
                const int j = (int)__umulhi(w, (uint32_t)(i + 1));
                const uint8_t tmp = d[i]; d[i] = d[j]; d[j] = tmp;
                --i;
            }
        }
    }
}

// deal_starting_cards (:53-101) from the first four cards of the deck: player, dealer (the upcard), player, dealer.
struct BjDeal {
    int r1, r2, d1, d2;                 // the four cards as rank values (an ace counts 11 here)
    int ps, ds;                         // player's and dealer's sums
    bool has, dhas;                     // usable aces
};
__device__ __forceinline__ BjDeal bj_deal(int c0, int c1, int c2, int c3) {
    BjDeal o;
    o.r1 = bj_rank(c0); const bool a1 = o.r1 == 1; if (a1) o.r1 = 11;                          // :53-59
    o.d1 = bj_rank(c1); const bool da1 = o.d1 == 1; if (da1) o.d1 = 11;                        // :62-69
    o.r2 = bj_rank(c2); const bool a2 = o.r2 == 1; if (a2) o.r2 = 11;                          // :72-78
    o.d2 = bj_rank(c3); const bool dfirst = !da1 && o.d2 == 1; if (o.d2 == 1) o.d2 = 11;       // :81-87
    o.has = a1 || a2; o.dhas = da1 || dfirst;
    o.ps = o.r1 + o.r2; o.ds = o.d1 + o.d2;
    if (o.ps > 21 && o.has) { o.ps -= 10; o.has = false; }                                     // :93-95
    if (o.ds > 21 && o.dhas) { o.ds -= 10; o.dhas = false; }                                   // :99-101
    return o;
}

// One card drawn by the player (:118-135) or by the dealer (:141-158): returns the rank it counts as, updates the hand's sum and
// usable ace.
__device__ __forceinline__ int bj_draw(int card, int& sum, bool& has) {
    int rank = bj_rank(card);
    const bool ace = rank == 1;
    if (ace && !has) rank = 11;
    has = has || ace;   // (ace & ~already) | already
    sum += rank;
    if (sum > 21 && has) { sum -= 10; has = false; }
    return rank;
}
// whether the dealer draws again after a card (:159-160; a deck that runs out ends the loop)
__device__ __forceinline__ bool bj_dealer_active(int ds, int pos) { return ds < 17 && ds <= 21 && pos < 52; }
// the terminal reward of a stand (:171-177)
__device__ __forceinline__ int bj_stand_reward(int ps, int ds) { return (ds > 21 || ps >= ds) ? 1 : -1; }

}  // namespace pulse_bj
