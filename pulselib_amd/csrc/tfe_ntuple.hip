// tfe_ntuple.hip -- 2048 on 4 x 4: an n-tuple network trained by batch TD(0) on afterstates, four launches:
// pulse_tfe_nt_rollout, pulse_tfe_nt_learn, pulse_tfe_nt_apply, pulse_tfe_nt_evaluate (include/pulse_env.h).
//
// V(afterstate) = the sum of a few lookup tables, each indexed by the nibbles on a fixed set of cells, read on the board's eight
// images.  One lane plays one game with the board as the packed 64-bit key in two registers (tfe_device.h: the row-table move, the
// spawn and the game-over test of the step kernel, on the environment's own Philox stream); a move is four row-table moves, 4 F
// gathers from the weights and one comparison.  Which cell a feature reads is the same for every lane: the host derives the images'
// cells and hands the kernels 6 shift counts per feature in one 64-bit word, by value, so a nibble is a shift by a scalar and no lane
// indexes an array.  The learner runs one lane per recorded move and adds temporal differences as fixed-point integers, so the
// accumulators do not depend on scheduling; the apply launch moves each weight by step * the mean of its adds.
// The game loop (play_game) and the learner's kernel (tfe_nt_scatter_kernel) are tfe_ntuple_device.h's, the game kernel
// (tfe_nt_play_kernel, here at one lane per game) tfe_ntuple_search_device.h's.  launch_scatter instantiates the scatter without its
// third accumulator, and makes the adds of tfe_ntuple_lambda.hip's and tfe_ntuple_backed.hip's learners too.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"
#include "tfe_ntuple_search_device.h"

namespace {

using namespace pulse_tfe;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256;
static_assert(sizeof(PulseTfeNtNet) == 104 && sizeof(PulseTfeNtRollout) == 232 && sizeof(PulseTfeNtLearn) == 176 && sizeof(PulseTfeNtApply) == 128 &&
              sizeof(PulseTfeNtEval) == 208, "struct layouts are part of the ABI");

__global__ __launch_bounds__(kBlock) void tfe_nt_apply_kernel(float* __restrict__ weights, longlong2* __restrict__ acc, uint64_t n_weights, double step) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_weights) return;
    const longlong2 a = acc[i];                                                         // {sum, cnt}
    if (a.y > 0) {
        const double mean = __dmul_rn(__ddiv_rn((double)a.x, (double)a.y), 1.0 / (double)(1 << PULSE_TFE_NT_FRAC_BITS));
        weights[i] = (float)__dadd_rn((double)weights[i], __dmul_rn(step, mean));
        acc[i] = make_longlong2(0, 0);
    }
}

}  // namespace

namespace pulse_tfe {

// The cell of the board that cell `cell` of T_j(board) shows (include/pulse_env.h, "eight symmetries"): j & 3 rotations by the
// environment's rotation (out[r][c] = in[c][3 - r]), for j >= 4 after a transpose.
int image_cell(int j, int cell) {
    int r = cell / 4, c = cell % 4;
    for (int q = 0; q < (j & 3); ++q) { const int nr = c, nc = 3 - r; r = nr; c = nc; }
    return j >= 4 ? c * 4 + r : r * 4 + c;
}

// The checks of the network, shared by the entry points; fills the kernels' form of it.
int check_net(const PulseTfeNtNet& n, bool need_weights, const char* name, NtDev* dev) {
    if (n.n != 4) return fail_named(name, "board side n must be 4 (the n-tuple network plays the packed 4 x 4 board)");
    if (n.n_tuples < 1 || n.n_tuples > kMaxTuples) return fail_named(name, "n_tuples must be in 1..8");
    if (n.symmetric != 0 && n.symmetric != 1) return fail_named(name, "symmetric must be 0 or 1");
    if (n.reserved0 != 0) return fail_named(name, "net.reserved0 must be 0 (zero-initialise the struct)");
    *dev = NtDev{};
    dev->n_tuples = n.n_tuples;
    const int images = n.symmetric ? 8 : 1;
    uint64_t total = 0;
    for (int t = 0; t < n.n_tuples; ++t) {
        const int len = n.tuple_len[t];
        if (len < 1 || len > kMaxLen) return fail_named(name, "a tuple's length must be in 1..6");
        uint32_t seen = 0u;
        for (int i = 0; i < len; ++i) {
            const int cell = n.cells[t][i];
            if (cell > 15) return fail_named(name, "a tuple's cell must be in 0..15");
            if (seen >> cell & 1u) return fail_named(name, "a cell is repeated within a tuple");
            seen |= 1u << cell;
            for (int j = 0; j < images; ++j) dev->shifts[t * images + j] |= (uint64_t)(4 * image_cell(j, cell)) << (8 * i);
        }
        dev->offset[t] = (uint32_t)total;
        dev->mask[t] = (uint32_t)((1ull << (4 * len)) - 1ull);
        total += 1ull << (4 * len);
    }
    if (n.n_weights != total) return fail_named(name, "n_weights must be the sum of 16^len over the tuples");
    if (need_weights && !n.weights) return fail_named(name, "weights is null");
    if ((uintptr_t)n.weights & 3u) return fail_named(name, "weights must be 4-byte aligned");
    return 0;
}

void launch_scatter(const Moves& m, const NtDev& dev, bool symmetric, void* stream) { launch_scatter_as<false>(m, dev, symmetric, stream); }

int check_rollout(const PulseTfeNtRollout* o, const char* name, NtDev* dev, Games* g) {
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_net(o->net, true, name, dev)) return rc;
    if (int rc = check_batch(o, name)) return rc;
    if (!(o->epsilon >= 0.0 && o->epsilon <= 1.0)) return fail_named(name, "epsilon must be in [0, 1]");
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->values) return fail_named(name, "values is null");
    if (!o->steps) return fail_named(name, "steps is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (!o->total_score) return fail_named(name, "total_score is null");
    if (!o->episode_reward) return fail_named(name, "episode_reward is null");
    if (!o->stats) return fail_named(name, "stats is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->total_score & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / total_score / stats must be 8-byte aligned");
    if (((uintptr_t)o->lengths & 3u) || ((uintptr_t)o->episode_reward & 3u)) return fail_named(name, "lengths / episode_reward must be 4-byte aligned");
    *g = games_of(o);
    g->keys = o->keys; g->values = o->values; g->steps = o->steps; g->lengths = o->lengths; g->total_score = o->total_score;
    g->episode_reward = o->episode_reward; g->stats = o->stats;
    return 0;
}

int check_eval(const PulseTfeNtEval* o, const char* name, NtDev* dev, Games* g) {
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_net(o->net, true, name, dev)) return rc;
    if (int rc = check_batch(o, name)) return rc;
    if (!(o->epsilon >= 0.0 && o->epsilon <= 1.0)) return fail_named(name, "epsilon must be in [0, 1]");
    if (!o->summary) return fail_named(name, "summary is null");
    if (!o->max_tile_hist) return fail_named(name, "max_tile_hist is null");
    if (((uintptr_t)o->summary & 7u) || ((uintptr_t)o->max_tile_hist & 7u)) return fail_named(name, "summary / max_tile_hist must be 8-byte aligned");
    if ((uintptr_t)o->total_score & 7u) return fail_named(name, "total_score must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    *g = games_of(o);
    g->lengths = o->lengths; g->total_score = o->total_score; g->stats = o->summary; g->hist = o->max_tile_hist;
    return 0;
}

}  // namespace pulse_tfe

extern "C" int pulse_tfe_nt_rollout(const PulseTfeNtRollout* o, void* stream) {
    NtDev dev;
    Games g;
    if (int rc = check_rollout(o, "pulse_tfe_nt_rollout", &dev, &g)) return rc;
    if (int rc = launch_play<true, 0, 0>(0, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_rollout launch");
}

extern "C" int pulse_tfe_nt_evaluate(const PulseTfeNtEval* o, void* stream) {
    NtDev dev;
    Games g;
    if (int rc = check_eval(o, "pulse_tfe_nt_evaluate", &dev, &g)) return rc;
    if (int rc = launch_play<false, 0, 0>(0, g, dev, o->net.symmetric != 0, stream)) return rc;
    return finish_launch("pulse_tfe_nt_evaluate launch");
}

extern "C" int pulse_tfe_nt_learn(const PulseTfeNtLearn* o, void* stream) {
    const char* name = "pulse_tfe_nt_learn";
    NtDev dev;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->stats & 7u)) return fail_named(name, "keys / values / stats must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    launch_scatter(m, dev, o->net.symmetric != 0, stream);
    return finish_launch("pulse_tfe_nt_learn launch");
}

extern "C" int pulse_tfe_nt_apply(const PulseTfeNtApply* o, void* stream) {
    const char* name = "pulse_tfe_nt_apply";
    if (!o) return fail_named(name, "options are null");
    NtDev dev;
    if (int rc = check_net(o->net, true, name, &dev)) return rc;
    if (!(o->step > 0.0 && o->step <= 1.0)) return fail_named(name, "step must be in (0, 1]");
    if (int rc = check_acc(o->acc, name)) return rc;
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    const dim3 grid((unsigned)((o->net.n_weights + kBlock - 1) / kBlock)), block(kBlock);
    hipLaunchKernelGGL(tfe_nt_apply_kernel, grid, block, 0, (hipStream_t)stream, o->net.weights, reinterpret_cast<longlong2*>(o->acc), o->net.n_weights, o->step);
    return finish_launch("pulse_tfe_nt_apply launch");
}
