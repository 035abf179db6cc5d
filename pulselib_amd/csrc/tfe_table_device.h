// tfe_table_device.h -- the 2048 hash tables' shared pieces: the state key, its hash and the bounded linear probe, used by the
// Q-learning table (qtable.hip) and the Monte-Carlo table (tfe_mc.hip).  The two entry layouts and probe limits are theirs
// (include/pulse_env.h); an entry type needs an `unsigned long long key` (0 = free).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pulse_tfe {

// board -> key: 4 bits of log2(tile) per cell (0 = empty), row-major, cell 0 in the low nibble.  The cell count is either a
// template argument (pack_cells<16>(b)) or a run-time one (pack_cells(b, cells)).
// (No unroll pragma: qtable.hip's select and update kernels pass a run-time count and compile to other code under one.  And a
// constant count goes in as the template argument where the caller had its loop unrolled by a pragma -- tfe_mc.hip: as a
// function argument it is unrolled later, after inlining, and the roll-out kernel is scheduled differently.)
template <int Cells = 0>
__device__ __forceinline__ uint64_t pack_cells(const int* b, int cells = Cells) {
    const int n = Cells ? Cells : cells;
    uint64_t key = 0;
    for (int i = 0; i < n; ++i) {
        const int v = b[i];
        const uint64_t e = v > 0 ? (uint64_t)min(31 - __clz(v), 15) : 0ull;
        key |= e << (4 * i);
    }
    return key;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}

// Slot of `key` inside [base, base + slots), or -1: absent.  Never inserts.  At most MaxProbe slots are examined -- the limit
// find_or_insert places under, so whatever it placed is found.
template <uint64_t MaxProbe, class Entry>
__device__ __forceinline__ long long find(const Entry* table, uint64_t base, uint64_t slots, uint64_t key) {
    const uint64_t h = mix64(key) & (slots - 1);
    const uint64_t limit = slots < MaxProbe ? slots : MaxProbe;
    for (uint64_t probe = 0; probe < limit; ++probe) {
        const uint64_t s = base + ((h + probe) & (slots - 1));
        const unsigned long long cur = table[s].key;
        if (cur == key) return (long long)s;
        if (cur == 0ull) return -1;
    }
    return -1;
}
// Slot of `key` inside [base, base + slots): inserted (value row already zero) if absent.  -1 = no room.
// At most MaxProbe slots are examined: a table filled to the brim would otherwise turn every lookup of every
// thread into a walk over the whole table (262,144 threads x 2^24 slots: a launch that never ends); past the
// limit the state counts as "no room" like a full region.
// (Tried and dropped, DESIGN.md section 3.4: a "shared by several boards" hint kept in the entry's spare words by plain loads
// and stores at the lookup of the state a move led to, so that the next launch sends the updates of a hot entry straight to the
// combine path instead of racing for a compare-and-swap -- 233 -> 140 us at the second step after a reset, but +8 us at EVERY
// step for dirtying the looked-up line, and the racy visitor count rarely passed 8 across the eight L2s.)
template <uint64_t MaxProbe, class Entry>
__device__ __forceinline__ long long find_or_insert(Entry* table, uint64_t base, uint64_t slots, uint64_t key) {
    const uint64_t h = mix64(key) & (slots - 1);
    const uint64_t limit = slots < MaxProbe ? slots : MaxProbe;
    for (uint64_t probe = 0; probe < limit; ++probe) {
        const uint64_t s = base + ((h + probe) & (slots - 1));
        unsigned long long cur = table[s].key;
        if (cur == key) return (long long)s;
        if (cur == 0ull) {
            cur = atomicCAS(&table[s].key, 0ull, (unsigned long long)key);
            if (cur == 0ull || cur == key) return (long long)s;
        }
    }
    return -1;
}

}  // namespace pulse_tfe
