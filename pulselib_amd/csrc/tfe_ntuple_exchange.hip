// tfe_ntuple_exchange.hip -- the 2048 n-tuple network's sparse accumulator exchange for rank-parallel rounds (DESIGN.md section
// 13.14), two entry points: pulse_tfe_nt_acc_pack and pulse_tfe_nt_acc_unpack (include/pulse_env.h).
//
// The learners add fixed-point integers into acc = {sum, cnt} per weight (and |d| into acc_abs); integer adds commute, so the sum of
// R ranks' accumulators is the accumulator of one process that played all the games.  A round touches a small share of the cells, so
// a rank sends the cells it touched and not the table: the pack launch compacts the cells with cnt > 0 into a list of 32-byte
// records {index, sum, cnt, abs} behind a 32-byte header {found, written, 0, 0}, and the unpack launch adds a list into acc.
//
// Pack: 256 lanes per workgroup, four cells per lane (four 16-byte loads), a tile of 1,024 cells per workgroup and pass, tiles taken
// grid-stride under a capped grid.  A wavefront takes 256 consecutive cells, lane l the cells l, 64 + l, 128 + l and 192 + l of them:
// every load instruction of a wavefront reads 1,024 consecutive bytes.  (Measured on the default network, DESIGN.md section 13.14: with
// four CONSECUTIVE cells per lane, where a load instruction strides over the lines its siblings read later, 165 us; so, 152 us.)
// A lane's slot is the prefix over its wavefront (one ballot per cell of the four and
// the set bits below the lane), the wavefronts' totals meet in LDS, and ONE lane of a workgroup that found anything takes the
// workgroup's slots from `found` with one returning atomic; a tile without a live cell costs no atomic at all.
// Entries at slots >= capacity are counted and not written.  A one-lane tail kernel behind it sets written = min(found, capacity).
// Unpack: lanes take the slots below the header's `written` grid-stride; the adds are 64-bit atomics without a returned value.
#include <hip/hip_runtime.h>

#include "pulse_internal.h"

namespace {

using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256, kWave = 64, kWaves = kBlock / kWave;
constexpr int kCells = 4;                                                               // cells per lane and pass, kWave apart
constexpr int kTile = kBlock * kCells;                                                  // cells per workgroup and pass
constexpr int kBlocksPerCu = 8;                                                         // the grids' cap: eight workgroups per compute unit, all resident at 64 VGPRs or fewer
constexpr int kHeader = 2;                                                              // the header, in 16-byte words
static_assert(sizeof(PulseTfeNtAccList) == 56, "struct layouts are part of the ABI");

// Cell i, or a cell no move visited where i is beyond the last: the load is of the last cell then, and unconditional, so that the four
// loads of a pass are in flight together (behind a branch each, the compiler waited for every one before it asked for the next).
__device__ __forceinline__ longlong2 cell_or_none(const longlong2* __restrict__ acc, const uint64_t i, const uint64_t n_entries) {
    longlong2 c = acc[i < n_entries ? i : n_entries - 1];
    if (i >= n_entries) c.y = 0;
    return c;
}

// list: the header {found, written} {0, 0}, then per entry {index, sum} {cnt, abs}.  The LDS words are kept twice, by the parity of
// the pass: a wavefront that is a pass ahead writes the other set, so two barriers per pass are enough.
__global__ __launch_bounds__(kBlock) void tfe_nt_acc_pack_kernel(const longlong2* __restrict__ acc, const long long* __restrict__ acc_abs,
                                                                  longlong2* __restrict__ list, uint64_t n_entries, uint64_t capacity, uint64_t n_tiles) {
    __shared__ unsigned wave_total[2][kWaves];
    __shared__ unsigned long long wg_base[2];
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned parity = 0;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, parity ^= 1u) {  // (uniform over the workgroup: every lane meets the barriers)
        const uint64_t first = tile * kTile + (uint64_t)wave * (kWave * kCells) + lane; // the lane's cells: first + k * kWave
        longlong2 c[kCells];
#pragma unroll
        for (int k = 0; k < kCells; ++k) c[k] = cell_or_none(acc, first + k * kWave, n_entries);
        unsigned long long live[kCells];                                                // per cell of the lanes' four: the wavefront's live lanes (uniform: scalar registers)
        unsigned total = 0;                                                             // the wavefront's entries
#pragma unroll
        for (int k = 0; k < kCells; ++k) {
            live[k] = __ballot(c[k].y > 0);
            total += (unsigned)__popcll(live[k]);
        }
        if (lane == 0) wave_total[parity][wave] = total;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned sum = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) sum += wave_total[parity][w];
            if (sum) wg_base[parity] = atomicAdd(reinterpret_cast<unsigned long long*>(list), (unsigned long long)sum);     // found: one per workgroup
        }
        __syncthreads();
        if (total) {                                                                    // (then the workgroup's sum was not 0: wg_base is this pass's)
            unsigned long long slot0 = wg_base[parity];
            for (unsigned w = 0; w < wave; ++w) slot0 += wave_total[parity][w];
#pragma unroll
            for (int k = 0; k < kCells; ++k) {                                          // the wavefront's slots: cell k of every lane, then cell k + 1
                const unsigned long long slot = slot0 + (unsigned)__popcll(live[k] & below);
                slot0 += (unsigned)__popcll(live[k]);
                if (c[k].y > 0 && slot < capacity) {
                    const long long mag = acc_abs ? acc_abs[first + k * kWave] : 0ll;
                    list[kHeader + 2 * slot] = make_longlong2((long long)(first + k * kWave), c[k].x);
                    list[kHeader + 2 * slot + 1] = make_longlong2(c[k].y, mag);
                }
            }
        }
    }
}

// behind the pack kernel on its stream: written = min(found, capacity)
__global__ void tfe_nt_acc_pack_tail_kernel(long long* __restrict__ header, uint64_t capacity) {
    const unsigned long long found = (unsigned long long)header[0];
    header[1] = (long long)(found < capacity ? found : capacity);
}

// A header that says more entries than the list holds is refused whole, by one lane.  Otherwise an entry is tested before anything is
// touched: index < n_entries and cnt > 0, or it adds nothing and is counted as refused.
__global__ __launch_bounds__(kBlock) void tfe_nt_acc_unpack_kernel(unsigned long long* __restrict__ acc, unsigned long long* __restrict__ acc_abs,
                                                                    const longlong2* __restrict__ list, unsigned long long* __restrict__ stats,
                                                                    uint64_t n_entries, uint64_t capacity) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t written = (uint64_t)list[0].y;                                       // (a negative word is a large one)
    if (written > capacity) {                                                           // (uniform over the launch)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(stats + 1, (unsigned long long)capacity);
        return;
    }
    unsigned long long added = 0, refused = 0;
    for (uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x; slot < written; slot += (uint64_t)gridDim.x * kBlock) {
        const longlong2 head = list[kHeader + 2 * slot], tail = list[kHeader + 2 * slot + 1];      // {index, sum} {cnt, abs}
        const uint64_t idx = (uint64_t)head.x;
        if (idx < n_entries && tail.x > 0) {
            atomicAdd(acc + 2 * idx, (unsigned long long)head.y);
            atomicAdd(acc + 2 * idx + 1, (unsigned long long)tail.x);
            if (acc_abs) atomicAdd(acc_abs + idx, (unsigned long long)tail.y);
            ++added;
        } else {
            ++refused;
        }
    }
    if (added) atomicAdd(&wg[0], added);                                                // LDS
    if (refused) atomicAdd(&wg[1], refused);
    __syncthreads();
    if (threadIdx.x < 2 && wg[threadIdx.x]) atomicAdd(stats + threadIdx.x, wg[threadIdx.x]);
}

int check_list(const PulseTfeNtAccList* o, const char* name, bool need_stats) {
    if (!o) return fail_named(name, "options are null");
    if (o->n_entries < 1 || o->n_entries > (1ull << 32)) return fail_named(name, "n_entries must be in 1..2^32");
    if (!o->acc) return fail_named(name, "acc is null");
    if ((uintptr_t)o->acc & 15u) return fail_named(name, "acc must be 16-byte aligned");
    if ((uintptr_t)o->acc_abs & 7u) return fail_named(name, "acc_abs must be 8-byte aligned");
    if (o->capacity < 1) return fail_named(name, "capacity must be positive");
    if (!o->list) return fail_named(name, "list is null");
    if ((uintptr_t)o->list & 31u) return fail_named(name, "list must be 32-byte aligned");
    if (need_stats && !o->stats) return fail_named(name, "stats is null");
    if ((uintptr_t)o->stats & 7u) return fail_named(name, "stats must be 8-byte aligned");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    return 0;
}

unsigned capped_grid(uint64_t blocks) {
    const uint64_t cap = (uint64_t)pulse::device_cus() * kBlocksPerCu;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

extern "C" int pulse_tfe_nt_acc_pack(const PulseTfeNtAccList* o, void* stream) {
    const char* name = "pulse_tfe_nt_acc_pack";
    if (int rc = check_list(o, name, false)) return rc;
    if (hipError_t e = hipMemsetAsync(o->list, 0, 32, (hipStream_t)stream)) return pulse::fail_hip((int)e, "pulse_tfe_nt_acc_pack header");
    const uint64_t n_tiles = (o->n_entries + kTile - 1) / kTile;
    hipLaunchKernelGGL(tfe_nt_acc_pack_kernel, dim3(capped_grid(n_tiles)), dim3(kBlock), 0, (hipStream_t)stream, reinterpret_cast<const longlong2*>(o->acc),
                       reinterpret_cast<const long long*>(o->acc_abs), reinterpret_cast<longlong2*>(o->list), o->n_entries, o->capacity, n_tiles);
    hipLaunchKernelGGL(tfe_nt_acc_pack_tail_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, reinterpret_cast<long long*>(o->list), o->capacity);
    return finish_launch("pulse_tfe_nt_acc_pack launch");
}

extern "C" int pulse_tfe_nt_acc_unpack(const PulseTfeNtAccList* o, void* stream) {
    const char* name = "pulse_tfe_nt_acc_unpack";
    if (int rc = check_list(o, name, true)) return rc;
    const unsigned grid = capped_grid((o->capacity + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(tfe_nt_acc_unpack_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, reinterpret_cast<unsigned long long*>(o->acc),
                       reinterpret_cast<unsigned long long*>(o->acc_abs), reinterpret_cast<const longlong2*>(o->list),
                       reinterpret_cast<unsigned long long*>(o->stats), o->n_entries, o->capacity);
    return finish_launch("pulse_tfe_nt_acc_unpack launch");
}
