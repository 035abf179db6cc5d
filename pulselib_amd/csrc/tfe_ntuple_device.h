// tfe_ntuple_device.h -- what the units of the 2048 n-tuple network share (tfe_ntuple.hip: the learner's four launches; tfe_ntuple_search.hip:
// expectimax play; tfe_ntuple_lambda.hip: the TD(lambda) learner): the network as the kernels take it, a feature's index, V of four
// afterstates at once, the learners' target, fixed-point difference and adds, the 32,768-tile test, the game loops' parameters and
// the host's checks of the network, of the accumulators and of a batch of games.  One copy each.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pulse_internal.h"
#include "tfe_device.h"

namespace pulse_tfe {

using pulse::fail_named;

constexpr int kMaxTuples = PULSE_TFE_NT_MAX_TUPLES, kMaxLen = PULSE_TFE_NT_MAX_LEN;

// The network as the kernels take it (by value: every word is read at a wavefront-uniform position).  Feature f = t * images + j:
// byte i of shifts[f] = 4 * (the board cell that image j shows at cell i of tuple t), 0 at and beyond the tuple's length -- those
// nibbles are masked off again by mask[t] = 16^len - 1.
struct NtDev {
    uint64_t shifts[kMaxTuples * 8];
    uint32_t offset[kMaxTuples], mask[kMaxTuples];
    int32_t n_tuples;
};

__device__ __forceinline__ uint32_t feature_index(uint64_t key, uint64_t sh, uint32_t mask, uint32_t offset) {
    uint32_t idx = 0u;
#pragma unroll
    for (int i = 0; i < kMaxLen; ++i) idx |= ((uint32_t)(key >> ((sh >> (8 * i)) & 63ull)) & 15u) << (4 * i);
    return (idx & mask) + offset;
}

// V of the four afterstates of a move at once: per tuple the 4 * IMG indices are formed first and their loads issued with nothing
// dependent between them (32 lines in flight per lane), then added in the order of the definition: tuple-major, image j = 0..7.
template <int IMG>
__device__ __forceinline__ void values4(const NtDev& net, const float* __restrict__ w, const uint64_t (&ka)[4], double (&v)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) v[a] = 0.0;
#pragma unroll 1
    for (int t = 0; t < net.n_tuples; ++t) {
        const uint32_t mask = net.mask[t], offset = net.offset[t];
        uint32_t idx[4][IMG];
#pragma unroll
        for (int j = 0; j < IMG; ++j) {
            const uint64_t sh = net.shifts[t * IMG + j];
#pragma unroll
            for (int a = 0; a < 4; ++a) idx[a][j] = feature_index(ka[a], sh, mask, offset);
        }
        float x[4][IMG];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < IMG; ++j) x[a][j] = w[idx[a][j]];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < IMG; ++j) v[a] = __dadd_rn(v[a], (double)x[a][j]);
    }
}

// What the learners share (tfe_ntuple.hip: batch TD(0); tfe_ntuple_lambda.hip: TD(lambda)).  The one-step target of a move that is
// not its game's last, from the next move's byte and value ...
__device__ __forceinline__ double td_target(const uint32_t next_step, const double next_value, const double gamma) {
    return __dadd_rn((double)((next_step >> 2) & 31u), __dmul_rn(gamma, next_value));
}

// ... a difference clamped to +-PULSE_TFE_NT_DELTA_MAX (`clamp`: it was outside) as the fixed-point integer the accumulators hold ...
__device__ __forceinline__ unsigned long long td_fixed(double delta, bool& clamp) {
    clamp = delta > PULSE_TFE_NT_DELTA_MAX || delta < -PULSE_TFE_NT_DELTA_MAX;
    delta = delta > PULSE_TFE_NT_DELTA_MAX ? PULSE_TFE_NT_DELTA_MAX : (delta < -PULSE_TFE_NT_DELTA_MAX ? -PULSE_TFE_NT_DELTA_MAX : delta);
    return (unsigned long long)llrint(ldexp(delta, PULSE_TFE_NT_FRAC_BITS));
}

// ... and its adds: sum += d, cnt += 1 at every feature of `key`
template <int IMG>
__device__ __forceinline__ void add_features(const NtDev& net, unsigned long long* acc, const uint64_t key, const unsigned long long d) {
#pragma unroll 1
    for (int tu = 0; tu < net.n_tuples; ++tu) {
        const uint32_t mask = net.mask[tu], offset = net.offset[tu];
#pragma unroll
        for (int j = 0; j < IMG; ++j) {
            const size_t idx = (size_t)feature_index(key, net.shifts[tu * IMG + j], mask, offset);
            atomicAdd(acc + 2 * idx, d);
            atomicAdd(acc + 2 * idx + 1, 1ull);
        }
    }
}

__device__ __forceinline__ bool has_nibble15(const PackedBoard p) {
    const uint32_t l = p.lo & (p.lo >> 1) & (p.lo >> 2) & (p.lo >> 3), h = p.hi & (p.hi >> 1) & (p.hi >> 2) & (p.hi >> 3);
    return ((l | h) & 0x11111111u) != 0u;
}

// what the game loops get: pulse_tfe_nt_rollout's struct, or pulse_tfe_nt_evaluate's outputs in its shape (stats = summary)
struct Games {
    const float* weights;
    int32_t n_games, max_steps;
    double gamma;
    uint32_t eps_q24;
    uint64_t env_seed, agent_seed, tie_seed, board_id0, round;
    uint64_t* keys; double* values; uint8_t* steps;
    int32_t* lengths; int64_t* total_score; int32_t* episode_reward;
    int64_t* stats; int64_t* hist;
    const uint32_t* lut;
};

template <class O>
Games games_of(const O* o) {
    Games g{};
    g.weights = o->net.weights; g.n_games = o->n_games; g.max_steps = o->max_steps; g.gamma = o->gamma;
    g.eps_q24 = (uint32_t)std::floor(o->epsilon * 16777216.0);                         // once, here: the kernel compares integers
    g.env_seed = o->env_seed; g.agent_seed = o->agent_seed; g.tie_seed = o->tie_seed; g.board_id0 = o->board_id0; g.round = o->round;
    return g;
}

// The checks of the network, shared by the entry points; fills the kernels' form of it (defined in tfe_ntuple.hip).
int check_net(const PulseTfeNtNet& n, bool need_weights, const char* name, NtDev* dev);

// ... and those of a batch of games (the roll-out's, the learner's and the evaluation's structs name these fields alike)
template <class O>
int check_batch(const O* o, const char* name) {
    if (o->n_games < 1) return fail_named(name, "n_games must be positive");
    if (o->max_steps < 1 || o->max_steps > 65535) return fail_named(name, "max_steps must be in 1..65535");
    if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    return 0;
}

// ... and of the accumulators
inline int check_acc(const int64_t* acc, const char* name) {
    if (!acc) return fail_named(name, "acc is null");
    if ((uintptr_t)acc & 15u) return fail_named(name, "acc must be 16-byte aligned");
    return 0;
}

// what pulse_tfe_nt_evaluate and pulse_tfe_nt_evaluate_search refuse, and the game loop's parameters of an evaluation (defined in
// tfe_ntuple.hip)
int check_eval(const PulseTfeNtEval* o, const char* name, NtDev* dev, Games* g);

}  // namespace pulse_tfe
