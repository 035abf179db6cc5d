// tfe_ntuple_continue.hip -- the 2048 n-tuple network's games continued across rounds, one entry point:
// pulse_tfe_nt_continue_pick (include/pulse_env.h).
//
// A round played with a small max_steps cuts most of its games after K = max_steps moves.  The learners skip the last move of a cut
// game -- it has no successor -- so the next round's game g begins on the board that move was made on (pulse_tfe_nt_rollout_from reads
// it from start[g]) and decides it again under the new weights: every transition is learnt once, none twice, none dropped.  This launch
// fills `start` from the round just recorded, carries the score and the moves of the game so far in carry_score / carry_moves, and
// adds the games that are over -- or stopped at the 32,768 tile -- to `finished`, whole, in the evaluation's layout.
//
// One lane per game, 256 lanes per workgroup, no wait and nothing between workgroups.  Per game 4 + 1 + 8 + 8 bytes read from the
// records (a cut game: 8 more), 8 + 4 read and written in the carries, 8 written in start; one Philox block, one spawn, and for a cut
// game one move through the row table.  The counters are reduced in LDS and added once per workgroup and non-zero word.
#include <hip/hip_runtime.h>

#include "philox_device.h"
#include "pulse_internal.h"
#include "tfe_agent_device.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256;
constexpr int kContinued = 5;                                                           // finished[5]: the games this launch continued
static_assert(sizeof(PulseTfeNtContinuePick) == 96, "struct layouts are part of the ABI");
static_assert(kBlock >= kEvalBins, "flush_bins: one lane per word");

// L = min(lengths[g], max_steps), at least 1: rows L - 1 and (a cut game: L == max_steps >= 2) L - 2 are inside keys and steps.
__global__ __launch_bounds__(kBlock) void tfe_nt_continue_pick_kernel(const PulseTfeNtContinuePick o, const uint32_t* __restrict__ lut) {
    __shared__ unsigned long long wg[kEvalBins];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (g < o.n_games) {
        const size_t B = (size_t)o.n_games;
        int L = o.lengths[g];
        L = L > o.max_steps ? o.max_steps : L;                                          // (the buffers hold max_steps rows)
        L = L < 1 ? 1 : L;                                                              // (a recorded game has a move; a length that is none reads row 0)
        const size_t last = (size_t)(L - 1) * B + (size_t)g;
        const uint32_t b = o.steps[last];
        const uint64_t after = o.keys[last];
        const PackedBoard pa{(uint32_t)after, (uint32_t)(after >> 32)};
        const uint64_t id = o.board_id0 + (uint64_t)g;
        const bool capped = has_nibble15(pa);
        const bool cut = (b >> 7) == 0u && !capped && L == o.max_steps;
        const int64_t total = o.total_score[g], carried = o.carry_score[g];
        const int moves = o.carry_moves[g];
        // the draw that follows the board in hand: move L - 1's own spawn for a cut game (on the afterstate of move L - 2), the last
        // spawn of the game for a finished one (on the afterstate of move L - 1)
        const pulse_philox::U4 rnd = pulse_philox::philox4x32(o.env_seed, id, (uint64_t)(cut ? L - 1 : L));
        if (cut) {
            const uint64_t key = o.keys[(size_t)(L - 2) * B + (size_t)g];
            PackedBoard p{(uint32_t)key, (uint32_t)(key >> 32)};
            tfe_spawn_packed(p, rnd.x, rnd.y);                                          // the board move L - 1 was made on
            o.start[g] = (uint64_t)p.hi << 32 | p.lo;
            const int sc = tfe_move_packed(p, (int)(b & 3u), lut);                      // (p is now the afterstate: the host asserts it is `after`)
            o.carry_score[g] = carried + (total - (int64_t)sc);                         // the cut move is played again: its score is the next round's
            o.carry_moves[g] = moves + (L - 1);
            atomicAdd(&wg[kContinued], 1ull);                                           // LDS
        } else {
            PackedBoard p = pa;
            tfe_spawn_packed(p, rnd.x, rnd.y);                                          // the board the evaluation's game ends on
            uint32_t top = 0u;
#pragma unroll
            for (int i = 0; i < 8; ++i) top = max(top, max((p.lo >> (4 * i)) & 15u, (p.hi >> (4 * i)) & 15u));
            const unsigned long long s = (unsigned long long)(carried + total), n = (unsigned long long)(moves + L);
            add_game(wg, {1ull, n, s, s * s, s, 0ull, moves > 0 ? 1ull : 0ull, capped ? 1ull : 0ull}, (int)top);
            o.start[g] = 0ull;
            o.carry_score[g] = 0;
            o.carry_moves[g] = 0;
        }
    }
    flush_bins(wg, o.finished, o.finished + kEvalSummary);
}

}  // namespace

extern "C" int pulse_tfe_nt_continue_pick(const PulseTfeNtContinuePick* o, void* stream) {
    const char* name = "pulse_tfe_nt_continue_pick";
    if (!o) return fail_named(name, "options are null");
    if (o->n_games < 1) return fail_named(name, "n_games must be positive");
    if (o->max_steps < 2 || o->max_steps > 65535) return fail_named(name, "max_steps must be in 2..65535");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->steps) return fail_named(name, "steps is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (!o->total_score) return fail_named(name, "total_score is null");
    if (!o->start) return fail_named(name, "start is null");
    if (!o->carry_score) return fail_named(name, "carry_score is null");
    if (!o->carry_moves) return fail_named(name, "carry_moves is null");
    if (!o->finished) return fail_named(name, "finished is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->total_score & 7u) || ((uintptr_t)o->start & 7u) || ((uintptr_t)o->carry_score & 7u) ||
        ((uintptr_t)o->finished & 7u))
        return fail_named(name, "keys / total_score / start / carry_score / finished must be 8-byte aligned");
    if (((uintptr_t)o->lengths & 3u) || ((uintptr_t)o->carry_moves & 3u)) return fail_named(name, "lengths / carry_moves must be 4-byte aligned");
    const uint32_t* lut = nullptr;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    const dim3 grid((unsigned)(((int64_t)o->n_games + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(tfe_nt_continue_pick_kernel, grid, block, 0, (hipStream_t)stream, *o, lut);
    return finish_launch("pulse_tfe_nt_continue_pick launch");
}
