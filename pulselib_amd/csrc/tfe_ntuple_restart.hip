// tfe_ntuple_restart.hip -- the 2048 n-tuple network's roll-outs restarted from recorded boards, two entry
// points: pulse_tfe_nt_rollout_from and pulse_tfe_nt_restart_pick (include/pulse_env.h).
//
// Every game of pulse_tfe_nt_rollout, pulse_tfe_nt_rollout_search and pulse_tfe_nt_rollout_backed starts at its reset board, so a
// round spends most of its moves on openings the network already plays well.  Here game g starts on the board packed in start[g]
// where that board is usable and at its reset otherwise (play_game<true, Backed, true>: the one game loop, with the start board its
// only difference), and the pick launch fills `start` for the next round from the round just recorded: the board the game stood on
// at a fraction of its length.
//
// The six game kernels are tfe_nt_play_kernel (tfe_ntuple_search_device.h) with From set: one lane per game on q = r + gamma * V, 32
// lanes per game on search_q without and with the backed value.  At 32 lanes per game every lane of a group reads the same start[g]
// and decides alike; `writer` guards the store of the 0.  The pick is one lane per game: 4 + 8 bytes read and 8 written, one Philox
// block and one spawn.
#include <hip/hip_runtime.h>

#include <cmath>

#include "philox_device.h"
#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256;
static_assert(sizeof(PulseTfeNtRestartPick) == 72 && sizeof(PulseTfeNtRollout) == 232, "struct layouts are part of the ABI");

// One lane per game: the board game g of the recorded round stood on before its move t*, t* = floor(L * fraction) -- the afterstate
// of move t* - 1 with the environment's spawn of draw t* put into it, as the game loop did -- or 0.  t* - 1 <= L - 2 < max_steps:
// inside the rows of keys.
__global__ __launch_bounds__(kBlock) void tfe_nt_restart_pick_kernel(const PulseTfeNtRestartPick o) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    unsigned long long n_picked = 0ull, depth = 0ull;
    if (g < o.n_games) {
        int L = o.lengths[g];
        L = L > o.max_steps ? o.max_steps : L;                                          // (the buffers hold max_steps rows)
        const int at = (int)floor(__dmul_rn((double)L, o.fraction));
        uint64_t board = 0ull;
        if (L >= o.min_length && at >= 1 && at <= L - 1) {
            const uint64_t key = o.keys[(size_t)(at - 1) * (size_t)o.n_games + (size_t)g];
            PackedBoard p{(uint32_t)key, (uint32_t)(key >> 32)};
            const pulse_philox::U4 rnd = pulse_philox::philox4x32(o.env_seed, o.board_id0 + (uint64_t)g, (uint64_t)at);
            tfe_spawn_packed(p, rnd.x, rnd.y);
            board = (uint64_t)p.hi << 32 | p.lo;
            n_picked = 1ull;
            depth = (unsigned long long)at;
        }
        o.start[g] = board;
    }
    add_stats(wg, o.picked, 0, n_picked, 1, depth);
}

}  // namespace

extern "C" int pulse_tfe_nt_rollout_from(const PulseTfeNtRollout* o, int32_t layers, double* backed, uint64_t* start, void* stream) {
    const char* name = "pulse_tfe_nt_rollout_from";
    NtDev dev;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_start(layers, backed, start, name, "layers must be 0 or 1")) return rc;
    if (int rc = launch_play_from<0, 1, true>(layers, g, backed, start, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout_from launch");
}

extern "C" int pulse_tfe_nt_restart_pick(const PulseTfeNtRestartPick* o, void* stream) {
    const char* name = "pulse_tfe_nt_restart_pick";
    if (!o) return fail_named(name, "options are null");
    if (o->n_games < 1) return fail_named(name, "n_games must be positive");
    if (o->max_steps < 1 || o->max_steps > 65535) return fail_named(name, "max_steps must be in 1..65535");
    if (!(o->fraction > 0.0 && o->fraction < 1.0)) return fail_named(name, "fraction must be in (0, 1)");
    if (o->min_length < 2 || o->min_length > 65535) return fail_named(name, "min_length must be in 2..65535");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (!o->start) return fail_named(name, "start is null");
    if (!o->picked) return fail_named(name, "picked is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->start & 7u) || ((uintptr_t)o->picked & 7u)) return fail_named(name, "keys / start / picked must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    const dim3 grid((unsigned)(((int64_t)o->n_games + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(tfe_nt_restart_pick_kernel, grid, block, 0, (hipStream_t)stream, *o);
    return finish_launch("pulse_tfe_nt_restart_pick launch");
}
