// meeting_device.h -- the bounded meeting of all workgroups of ONE ordinary launch, used by the fused
// reduce + AdamW launch (qnet.hip) and the Q-table's follow-up launch (qtable.hip).  No state of its own: the caller sees to
// it that the grid is resident at once and that the eight arrival counters are zero when the launch starts.
//
// Workgroup b arrives on counter b & 7 (arrivals on ONE address serialise: 6 us for 282 workgroups).  Lanes 0..7 of wavefront 0
// watch one counter each; "go" = all eight read exactly full.  A wavefront whose wait runs out calls the meeting off by setting
// kOff in a counter that is still short -- with a compare-and-swap from the value it read, so the mark lands either before
// the missing arrival (that counter never reads full again: nobody goes, before or after) or not at all (the counter moved:
// read it again).  All or nothing: a full counter is never marked, a marked one never reads full, so every workgroup reads
// "go" or none does.  Exactly one mark lands per meeting (later readers see kOff and leave); the lane that placed it counts
// the meeting in the host's pinned word.  Every store one workgroup reads here from another goes through agent-scope atomics
// (the per-XCD L2s are not coherent for plain loads); what must be visible BEFORE the arrival is the caller's payload, ordered
// at the call site.
#pragma once
#include <hip/hip_runtime.h>

namespace pulse_meet {

constexpr int kCounters = 8;
constexpr unsigned kOff = 0x80000000u;      // an arrival counter with this bit set: the meeting was called off

__device__ __forceinline__ void arrive(unsigned* counters) {      // by ONE thread of the workgroup, after its payload has left
    __hip_atomic_fetch_add(counters + (blockIdx.x & (kCounters - 1)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// By all 64 lanes of wavefront 0: true (wavefront-uniform) iff the meeting came about.  `extra_arrivals`: arrivals counter 0
// expects beyond the grid's (a test hook: never met); `wait_ticks`: the bound, in ticks of the 100 MHz wall_clock64();
// `gave_up`: nullptr or the pinned host word, += 1 by the lane whose mark called the meeting off; SLEEP: the poll's s_sleep.
template <int SLEEP>
__device__ __forceinline__ bool wait(unsigned* counters, unsigned extra_arrivals, long long wait_ticks, long long* gave_up) {
    const int lane = (int)(threadIdx.x & 63u);
    unsigned want = (gridDim.x + 7 - (lane & 7)) / 8;              // workgroups b with b % 8 == lane
    if (lane == 0) want += extra_arrivals;
    for (const long long t0 = wall_clock64();;) {
        const unsigned got = lane < kCounters ? __hip_atomic_load(counters + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
        if (__ballot((got & kOff) != 0u) != 0ull) return false;
        const unsigned long long short_of = __ballot(got != want);
        if (short_of == 0ull) return true;
        if (wall_clock64() - t0 > wait_ticks) {
            const bool marked = lane == __ffsll((long long)short_of) - 1 && atomicCAS(counters + lane, got, got | kOff) == got;
            if (marked && gave_up) __hip_atomic_fetch_add(gave_up, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (__ballot(marked) != 0ull) return false;
            continue;                                              // the counter moved under the mark: read it again
        }
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

}  // namespace pulse_meet
