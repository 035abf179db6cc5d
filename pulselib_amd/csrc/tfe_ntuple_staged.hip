// tfe_ntuple_staged.hip -- the 2048 n-tuple network with weight sets by tile stage (multi-stage TD), four entry
// points: pulse_tfe_nt_rollout_staged, pulse_tfe_nt_learn_staged, pulse_tfe_nt_evaluate_staged and pulse_tfe_nt_search_staged
// (include/pulse_env.h).
//
// One table has to serve the openings and the boards with a 2,048 tile on them alike.  Here the network is S copies of its tables and
// a board reads, and a recorded move adds to, the copy of its stage: the number of thresholds the board's largest nibble has reached.
// The stage is an offset on a feature's index (tfe_ntuple_device.h: NtStagedDev, stage_of, stage_base), so nothing else of the
// network's units is new: the game loop (play_game), the chance layer (search_q), V of four afterstates (values4), the adds
// (add_features inside scatter_moves) and the greedy scan are the one copy each, instantiated here on the staged network.  What this
// file holds is their siblings' few wrapper lines: one lane per game on q = r + gamma * V, 32 lanes per game or board on search_q, one
// lane per recorded move for the adds.  The stage of a key is about thirty integer operations on its two halves beside the few hundred of
// its feature indices; values4 forms the four stages once, before its loop over the tuples.  The backward walks touch neither weights
// nor features and are the launches they were, and so are the apply launches, called once per stage on that stage's slices.
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
static_assert(sizeof(PulseTfeNtStages) == 16 && sizeof(PulseTfeNtLearnBacked) == 208 && sizeof(PulseTfeNtRollout) == 232 && sizeof(PulseTfeNtEval) == 208 &&
              sizeof(PulseTfeNtSearch) == 176, "struct layouts are part of the ABI");
static_assert(sizeof(NtStagedDev) == sizeof(NtDev) + 16, "the staged network is the network and four words");

// pulse_tfe_nt_rollout_staged at layers = 0: one lane plays one game from start[g] or its reset, q = r + gamma * V
template <int IMG>
__global__ __launch_bounds__(kBlock) void tfe_nt_staged_games_kernel(const Games o, const NtStagedDev net) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    play_game<true, false, true>(o, wg, blockIdx.x * kBlock + threadIdx.x, true,
                                 [&](const uint64_t, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                     one_ply_q<IMG>(net, o.weights, o.gamma, ka, sc, v, q);
                                 });
}

// ... and at layers = 1: one game per group of 32 lanes (g < n_games is the same in the 32, and a group beyond the batch only meets the
// barrier of the counts), without and with the backed value
template <int IMG, bool Backed>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_staged_search_rollout_kernel(const Games o, const NtStagedDev net) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    play_game<true, Backed, true>(o, wg, g, s == 0,
                                  [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                      values4<IMG>(net, o.weights, ka, v);
                                      search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                                  });
}

// pulse_tfe_nt_evaluate_staged at layers = 0: one lane per game
template <int IMG>
__global__ __launch_bounds__(kBlock) void tfe_nt_staged_eval_kernel(const Games o, const NtStagedDev net) {
    __shared__ unsigned long long wg[kEvalBins];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    play_game<false>(o, wg, blockIdx.x * kBlock + threadIdx.x, true,
                     [&](const uint64_t, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                         one_ply_q<IMG>(net, o.weights, o.gamma, ka, sc, v, q);
                     });
}

// ... and at layers = 1: the 32 lanes of a group play the game alike, lane 0 writes and counts
template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_staged_search_eval_kernel(const Games o, const NtStagedDev net) {
    __shared__ unsigned long long wg[kEvalBins];
    if (threadIdx.x < kEvalBins) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
    play_game<false>(o, wg, g, s == 0,
                     [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&)[4], double (&q)[4]) {
                         search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                     });
}

// pulse_tfe_nt_search_staged: 32 lanes per board; what the kernel takes of pulse_tfe_nt_search's struct
struct Boards {
    const float* weights;
    int32_t n_boards;
    double gamma;
    uint64_t tie_seed, round;
    const uint64_t* boards;
    double* q; int8_t* action; uint8_t* candidates;
    const uint32_t* lut;
};

template <int IMG>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_staged_search_kernel(const Boards o, const NtStagedDev net) {
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

// pulse_tfe_nt_learn_staged's adds: the learners' one scatter text on the staged network
template <int IMG, bool Given, bool Abs>
__global__ __launch_bounds__(kScatterBlock) void tfe_nt_staged_scatter_kernel(const Moves o, const NtStagedDev net) {
    scatter_moves<IMG, Given, Abs>(o, net);
}

template <int IMG>
void launch_staged_scatter(const Moves& m, const NtStagedDev& dev, const dim3 grid, hipStream_t st) {
    const dim3 block(kScatterBlock);
    if (m.deltas) {
        if (m.acc_abs) hipLaunchKernelGGL((tfe_nt_staged_scatter_kernel<IMG, true, true>), grid, block, 0, st, m, dev);
        else hipLaunchKernelGGL((tfe_nt_staged_scatter_kernel<IMG, true, false>), grid, block, 0, st, m, dev);
    } else {
        if (m.acc_abs) hipLaunchKernelGGL((tfe_nt_staged_scatter_kernel<IMG, false, true>), grid, block, 0, st, m, dev);
        else hipLaunchKernelGGL((tfe_nt_staged_scatter_kernel<IMG, false, false>), grid, block, 0, st, m, dev);
    }
}

// The checks of the stages, after those of the network; fills the kernels' form of the staged network from that of the network.
int check_stages(const PulseTfeNtStages* s, const PulseTfeNtNet& n, const NtDev& dev, const char* name, NtStagedDev* out) {
    if (!s) return fail_named(name, "stages are null");
    if (s->n_stages < 1 || s->n_stages > PULSE_TFE_NT_MAX_STAGES) return fail_named(name, "n_stages must be in 1..4");
    if (s->reserved0 != 0) return fail_named(name, "stages.reserved0 must be 0 (zero-initialise the struct)");
    *out = NtStagedDev{};
    static_cast<NtDev&>(*out) = dev;
    int below = 0;
    for (int i = 0; i < 4; ++i) {
        const int th = s->threshold[i];
        if (i >= s->n_stages - 1) {
            if (th != 0) return fail_named(name, "a threshold at or beyond n_stages - 1 must be 0");
            continue;
        }
        if (th < 1 || th > 15) return fail_named(name, "a threshold must be a nibble in 1..15");
        if (th <= below) return fail_named(name, "the thresholds must be strictly increasing");
        below = th;
        out->reach[i] = (uint32_t)(16 - th) * 0x01010101u;
    }
    out->n_weights = (uint32_t)n.n_weights;                                             // (check_net: at most 8 * 16^6 = 2^27, so 4 stages end at 2^29)
    return 0;
}

int check_staged_layers(const int32_t layers, const char* name) {
    return layers == 0 || layers == 1 ? 0 : fail_named(name, "layers must be 0 or 1 (two layers are not built on stages)");
}

}  // namespace

extern "C" int pulse_tfe_nt_rollout_staged(const PulseTfeNtRollout* o, const PulseTfeNtStages* stages, int32_t layers, double* backed, uint64_t* start,
                                           void* stream) {
    const char* name = "pulse_tfe_nt_rollout_staged";
    NtDev dev;
    NtStagedDev net;
    Games g;
    if (int rc = check_rollout(o, name, &dev, &g)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = check_staged_layers(layers, name)) return rc;
    if (backed && layers == 0) return fail_named(name, "backed needs layers = 1: a one-ply roll-out has no search to back a value up");
    if ((uintptr_t)backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if (!start) return fail_named(name, "start is null");
    if ((uintptr_t)start & 7u) return fail_named(name, "start must be 8-byte aligned");
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    g.backed = backed;
    g.start = start;
    const bool sym = o->net.symmetric != 0;
    hipStream_t st = (hipStream_t)stream;
    if (layers == 0) {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kBlock - 1) / kBlock)), block(kBlock);
        if (sym) hipLaunchKernelGGL(tfe_nt_staged_games_kernel<8>, grid, block, 0, st, g, net);
        else hipLaunchKernelGGL(tfe_nt_staged_games_kernel<1>, grid, block, 0, st, g, net);
    } else {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kSearchBlock);
        if (backed) {
            if (sym) hipLaunchKernelGGL((tfe_nt_staged_search_rollout_kernel<8, true>), grid, block, 0, st, g, net);
            else hipLaunchKernelGGL((tfe_nt_staged_search_rollout_kernel<1, true>), grid, block, 0, st, g, net);
        } else {
            if (sym) hipLaunchKernelGGL((tfe_nt_staged_search_rollout_kernel<8, false>), grid, block, 0, st, g, net);
            else hipLaunchKernelGGL((tfe_nt_staged_search_rollout_kernel<1, false>), grid, block, 0, st, g, net);
        }
    }
    return finish_launch("pulse_tfe_nt_rollout_staged launch");
}

extern "C" int pulse_tfe_nt_learn_staged(const PulseTfeNtLearnBacked* o, const PulseTfeNtStages* stages, void* stream) {
    const char* name = "pulse_tfe_nt_learn_staged";
    NtDev dev;
    NtStagedDev net;
    Moves m;
    if (int rc = check_moves(o, name, &dev, &m)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (!(o->lambda >= 0.0 && o->lambda <= 1.0)) return fail_named(name, "lambda must be in [0, 1]");
    if (o->backed && !o->deltas) return fail_named(name, "deltas is null (backed needs them)");
    if (o->lambda > 0.0 && !o->deltas) return fail_named(name, "deltas is null (lambda > 0 needs them)");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->deltas & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / deltas / stats must be 8-byte aligned");
    if ((uintptr_t)o->backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if ((uintptr_t)o->acc_abs & 7u) return fail_named(name, "acc_abs must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    if (o->deltas) {                                                                    // the walk, then the adds of what it left
        WalkBacked w{};
        w.n_games = o->n_games; w.max_steps = o->max_steps; w.gamma = o->gamma; w.lambda = o->lambda;
        w.values = o->values; w.steps = o->steps; w.lengths = o->lengths; w.deltas = o->deltas; w.backed = o->backed;
        if (o->backed) launch_backed_walk(w, stream);
        else launch_lambda_walk(w, stream);
        m.deltas = o->deltas;
    }
    m.acc_abs = o->acc_abs;
    const dim3 grid((unsigned)((m.n_games + kScatterBlock - 1) / kScatterBlock), (unsigned)m.max_steps);
    if (o->net.symmetric) launch_staged_scatter<8>(m, net, grid, (hipStream_t)stream);
    else launch_staged_scatter<1>(m, net, grid, (hipStream_t)stream);
    return finish_launch("pulse_tfe_nt_learn_staged launch");
}

extern "C" int pulse_tfe_nt_evaluate_staged(const PulseTfeNtEval* o, const PulseTfeNtStages* stages, int32_t layers, void* stream) {
    const char* name = "pulse_tfe_nt_evaluate_staged";
    NtDev dev;
    NtStagedDev net;
    Games g;
    if (int rc = check_eval(o, name, &dev, &g)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = check_staged_layers(layers, name)) return rc;
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    const bool sym = o->net.symmetric != 0;
    hipStream_t st = (hipStream_t)stream;
    if (layers == 0) {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kBlock - 1) / kBlock)), block(kBlock);
        if (sym) hipLaunchKernelGGL(tfe_nt_staged_eval_kernel<8>, grid, block, 0, st, g, net);
        else hipLaunchKernelGGL(tfe_nt_staged_eval_kernel<1>, grid, block, 0, st, g, net);
    } else {
        const dim3 grid((unsigned)(((int64_t)g.n_games + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kSearchBlock);
        if (sym) hipLaunchKernelGGL(tfe_nt_staged_search_eval_kernel<8>, grid, block, 0, st, g, net);
        else hipLaunchKernelGGL(tfe_nt_staged_search_eval_kernel<1>, grid, block, 0, st, g, net);
    }
    return finish_launch("pulse_tfe_nt_evaluate_staged launch");
}

extern "C" int pulse_tfe_nt_search_staged(const PulseTfeNtSearch* o, const PulseTfeNtStages* stages, void* stream) {
    const char* name = "pulse_tfe_nt_search_staged";
    NtDev dev;
    NtStagedDev net;
    const uint32_t* lut = nullptr;
    if (int rc = check_search(o, name, &dev)) return rc;
    if (int rc = check_stages(stages, o->net, dev, name, &net)) return rc;
    if (int rc = pulse::tfe_row_lut(&lut)) return rc;
    const Boards b{o->net.weights, o->n_boards, o->gamma, o->tie_seed, o->round, o->boards, o->q, o->action, o->candidates, lut};
    const dim3 grid((unsigned)(((int64_t)o->n_boards + kGroupsPerBlock - 1) / kGroupsPerBlock)), block(kSearchBlock);
    if (o->net.symmetric) hipLaunchKernelGGL(tfe_nt_staged_search_kernel<8>, grid, block, 0, (hipStream_t)stream, b, net);
    else hipLaunchKernelGGL(tfe_nt_staged_search_kernel<1>, grid, block, 0, (hipStream_t)stream, b, net);
    return finish_launch("pulse_tfe_nt_search_staged launch");
}
