// tfe_ntuple_device.h -- what the units of the 2048 n-tuple network share (tfe_ntuple.hip: the learner's four launches; tfe_ntuple_search.hip:
// expectimax play, one or two chance layers deep, and tfe_ntuple_search_rollout.hip, the roll-out under either; tfe_ntuple_lambda.hip: the TD(lambda) walk; tfe_ntuple_tc.hip: temporal-coherence step sizes;
// tfe_ntuple_backed.hip: search-backed targets; tfe_ntuple_restart.hip: roll-outs restarted from recorded boards;
// tfe_ntuple_staged.hip: weight sets by tile stage, with the staged network and the stage of a board): the network as the
// kernels take it, a feature's index, V of four afterstates at once, the learners' target, fixed-point difference and adds, their
// parameters (Moves), shared refusals (check_moves, check_learner), scatter kernel and launch ladder, the backward walk's kernel and hand-off (launch_walk), the four moves of a board, the greedy action, the game loop (play_game) with its parameters
// (Games) and the host's checks of the network, of the accumulators and of a batch of games.  One copy each.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "philox_device.h"
#include "pulse_internal.h"
#include "tfe_agent_device.h"
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

// The network with weight sets by tile stage (tfe_ntuple_staged.hip): stage s owns the weights
// [s * n_weights, (s + 1) * n_weights), and a board is in stage s = the number of thresholds its largest nibble has reached.
// reach[i] = 16 - (the nibble at which stage i + 1 begins) in each of its four bytes, 0 where the network has no such stage.
// Derived, so that NtDev -- a by-value argument of every kernel of the one-stage network -- keeps its size; the words are as
// wavefront-uniform as NtDev's.
struct NtStagedDev : NtDev {
    uint32_t reach[PULSE_TFE_NT_MAX_STAGES - 1];
    uint32_t n_weights;
};

template <class Net>
inline constexpr bool kStaged = std::is_same_v<Net, NtStagedDev>;

// The stage of board `key`: the even and the odd nibbles of its two halves as bytes (each 0..15); adding 16 - threshold to every byte
// sets bit 4 of a byte iff its nibble has reached the threshold (at most 15 + 15: no carry leaves a byte).  Four adds, an or of the
// four and one test per threshold, on the two 32-bit halves, with no array indexed by a lane.
__device__ __forceinline__ uint32_t stage_of(const NtStagedDev& net, const uint64_t key) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const uint32_t a = lo & 0x0F0F0F0Fu, b = (lo >> 4) & 0x0F0F0F0Fu, c = hi & 0x0F0F0F0Fu, d = (hi >> 4) & 0x0F0F0F0Fu;
    uint32_t s = 0u;
#pragma unroll
    for (int i = 0; i < PULSE_TFE_NT_MAX_STAGES - 1; ++i) {
        const uint32_t r = net.reach[i];
        s += (((a + r) | (b + r) | (c + r) | (d + r)) & 0x10101010u) != 0u ? 1u : 0u;
    }
    return s;
}

// what a feature's index gains in the stage of `key`: 0 for the one-stage network (nothing is computed), stage * n_weights otherwise;
// stages * n_weights <= 2^29, so the index stays inside 32 bits
template <class Net>
__device__ __forceinline__ uint32_t stage_base(const Net& net, const uint64_t key) {
    if constexpr (kStaged<Net>) return stage_of(net, key) * net.n_weights;
    else return 0u;
}

// V of the four afterstates of a move at once: per tuple the 4 * IMG indices are formed first and their loads issued with nothing
// dependent between them (32 lines in flight per lane), then added in the order of the definition: tuple-major, image j = 0..7.
// With weight sets by stage every afterstate is read in its own stage.
template <int IMG, class Net>
__device__ __forceinline__ void values4(const Net& net, const float* __restrict__ w, const uint64_t (&ka)[4], double (&v)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) v[a] = 0.0;
    uint32_t base[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) base[a] = stage_base(net, ka[a]);
#pragma unroll 1
    for (int t = 0; t < net.n_tuples; ++t) {
        const uint32_t mask = net.mask[t], offset = net.offset[t];
        uint32_t idx[4][IMG];
#pragma unroll
        for (int j = 0; j < IMG; ++j) {
            const uint64_t sh = net.shifts[t * IMG + j];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                idx[a][j] = feature_index(ka[a], sh, mask, offset);
                if constexpr (kStaged<Net>) idx[a][j] += base[a];
            }
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

// ... and its adds: sum += d, cnt += 1 at every feature of `key`; with Abs (temporal-coherence step sizes, tfe_ntuple_tc.hip) also
// acc_abs += |d|, d read as signed; with weight sets by stage, at the features of the stage of `key`
template <int IMG, bool Abs, class Net>
__device__ __forceinline__ void add_features(const Net& net, unsigned long long* acc, unsigned long long* acc_abs, const uint64_t key,
                                             const unsigned long long d) {
    const unsigned long long mag = (long long)d < 0 ? 0ull - d : d;
    const size_t base = (size_t)stage_base(net, key);
#pragma unroll 1
    for (int tu = 0; tu < net.n_tuples; ++tu) {
        const uint32_t mask = net.mask[tu], offset = net.offset[tu];
#pragma unroll
        for (int j = 0; j < IMG; ++j) {
            size_t idx = (size_t)feature_index(key, net.shifts[tu * IMG + j], mask, offset);
            if constexpr (kStaged<Net>) idx += base;                                    // (2 * idx below is formed in 64 bits)
            atomicAdd(acc + 2 * idx, d);
            atomicAdd(acc + 2 * idx + 1, 1ull);
            if constexpr (Abs) atomicAdd(acc_abs + idx, mag);
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
    double* backed;                                                                     // play_game<true, true> alone (tfe_ntuple_backed.hip): the search's best q per move
    uint64_t* start;                                                                    // play_game<true, *, true> alone (tfe_ntuple_restart.hip): the board game g starts from, or 0
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

// The learners' counterpart of Games: what pulse_tfe_nt_learn, pulse_tfe_nt_learn_lambda and pulse_tfe_nt_learn_tc hand the scatter
// (deltas: null for TD(0); acc_abs: pulse_tfe_nt_learn_tc's third accumulator, null for the other two)
struct Moves {
    int32_t n_games, max_steps;
    double gamma;
    const uint64_t* keys; const double* values; const uint8_t* steps;
    const int32_t* lengths;
    const double* deltas;
    int64_t* acc; int64_t* stats;
    int64_t* acc_abs;
};

// ... what both learners refuse, and the scatter's parameters of their struct (deltas left null)
template <class O>
int check_moves(const O* o, const char* name, NtDev* dev, Moves* m) {
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_net(o->net, false, name, dev)) return rc;
    if (int rc = check_batch(o, name)) return rc;
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->values) return fail_named(name, "values is null");
    if (!o->steps) return fail_named(name, "steps is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (int rc = check_acc(o->acc, name)) return rc;
    if (!o->stats) return fail_named(name, "stats is null");
    *m = Moves{o->n_games, o->max_steps, o->gamma, o->keys, o->values, o->steps, o->lengths, nullptr, o->acc, o->stats, nullptr};
    return 0;
}

// The learners' adds, one lane per recorded move: blockIdx.y = t, blockIdx.x * kScatterBlock + threadIdx.x = g.  Given: the move's
// difference is o.deltas' (after the walk of tfe_ntuple_lambda.hip); otherwise it is the one-step difference, formed here.  Abs: the
// adds go to o.acc_abs too (add_features).  One text (scatter_moves, which the kernel only calls): tfe_ntuple.hip instantiates the four forms without Abs (launch_scatter),
// tfe_ntuple_tc.hip the four with it (launch_scatter_tc), tfe_ntuple_staged.hip the eight on the staged network.
constexpr int kScatterBlock = 256;

template <int IMG, bool Given, bool Abs, class Net>
__device__ __forceinline__ void scatter_moves(const Moves& o, const Net& net) {
    __shared__ unsigned long long wg[3];
    if (threadIdx.x < 3) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = blockIdx.x * kScatterBlock + threadIdx.x, t = (int)blockIdx.y;
    const size_t B = (size_t)o.n_games;
    if (g < o.n_games) {
        int length = o.lengths[g];
        length = length > o.max_steps ? o.max_steps : length;                          // (the buffers hold max_steps rows)
        if (t < length) {
            const size_t at = (size_t)t * B + (size_t)g;
            const bool last = t == length - 1;
            const bool skip = last && (o.steps[at] & 0x80u) == 0u;
            if (skip) {
                atomicAdd(&wg[1], 1ull);                                                // LDS
            } else {
                double delta;
                if constexpr (Given) {
                    delta = o.deltas[at];
                } else {
                    double target = 0.0;
                    if (!last) target = td_target(o.steps[at + B], o.values[at + B], o.gamma);
                    delta = __dsub_rn(target, o.values[at]);
                }
                bool clamp;
                const unsigned long long d = td_fixed(delta, clamp);
                add_features<IMG, Abs>(net, reinterpret_cast<unsigned long long*>(o.acc), reinterpret_cast<unsigned long long*>(o.acc_abs), o.keys[at], d);
                atomicAdd(&wg[0], 1ull);
                if (clamp) atomicAdd(&wg[2], 1ull);
            }
        }
    }
    __syncthreads();
    const int i = (int)threadIdx.x;
    if (i < 3 && wg[i]) atomicAdd(reinterpret_cast<unsigned long long*>(o.stats) + (i == 0 ? 1 : i == 1 ? 2 : 4), wg[i]);
}

template <int IMG, bool Given, bool Abs, class Net>
__global__ __launch_bounds__(kScatterBlock) void tfe_nt_scatter_kernel(const Moves o, const Net net) {
    scatter_moves<IMG, Given, Abs>(o, net);
}

// ... and its one launch ladder: the difference is m.deltas' where it is set and the one-step difference otherwise
template <bool Abs, class Net>
void launch_scatter_as(const Moves& m, const Net& net, const bool symmetric, void* stream) {
    const dim3 grid((unsigned)((m.n_games + kScatterBlock - 1) / kScatterBlock), (unsigned)m.max_steps), block(kScatterBlock);
    hipStream_t st = (hipStream_t)stream;
    if (m.deltas) {
        if (symmetric) hipLaunchKernelGGL((tfe_nt_scatter_kernel<8, true, Abs, Net>), grid, block, 0, st, m, net);
        else hipLaunchKernelGGL((tfe_nt_scatter_kernel<1, true, Abs, Net>), grid, block, 0, st, m, net);
    } else {
        if (symmetric) hipLaunchKernelGGL((tfe_nt_scatter_kernel<8, false, Abs, Net>), grid, block, 0, st, m, net);
        else hipLaunchKernelGGL((tfe_nt_scatter_kernel<1, false, Abs, Net>), grid, block, 0, st, m, net);
    }
}

// ... instantiated on the one-stage network without Abs (defined in tfe_ntuple.hip)
void launch_scatter(const Moves& m, const NtDev& dev, bool symmetric, void* stream);

// ... and with the third accumulator, m.acc_abs (defined in tfe_ntuple_tc.hip)
void launch_scatter_tc(const Moves& m, const NtDev& dev, bool symmetric, void* stream);

// The backward walk of the learners that carry credit along a game: D_t = delta_t + (gamma * lambda) * D_{t+1} into o.deltas.  Backed
// says where delta_t of a move that is not its game's last comes from: without it (tfe_ntuple_lambda.hip) it
// is the one-step difference (r_{t+1} + gamma * V_{t+1}) - V_t of the records; with it (tfe_ntuple_backed.hip, section 13.6) it is
// backed[t + 1] - V_t, the search's value of the board the next move was made on.  What the kernel takes: the TD(lambda) learner's
// struct, of which it reads n_games, max_steps, gamma, lambda, values, steps, lengths and deltas, with `backed` behind it for the
// second form.
constexpr int kWalkBlock = 64, kRows = 8;

struct WalkBacked : PulseTfeNtLearnLambda {
    const double* backed;
};

// One lane per game, one wavefront per workgroup, t downwards from the wavefront's longest game: every lane of the wavefront is at
// the same row t, so a row's loads and stores are one 512-byte and one 64-byte segment, and a lane whose game is shorter waits with
// `t < length` as its predicate.  A lane reads its column of every row from the wavefront's first (what a row at or beyond its own
// length holds is loaded and not used); rows of kRows are loaded together, the next kRows before the chain of these is run, so the
// chain is one multiply and one add per move and no memory latency.  V and the byte of row t + 1 (Backed: `backed` of row t + 1) stay
// in registers for row t.
template <bool Backed>
__global__ __launch_bounds__(kWalkBlock) void tfe_nt_lambda_walk_kernel(const std::conditional_t<Backed, WalkBacked, PulseTfeNtLearnLambda> o) {
    const int g = (int)blockIdx.x * kWalkBlock + (int)threadIdx.x;
    const size_t B = (size_t)o.n_games;
    int length = 0;
    if (g < o.n_games) {
        length = o.lengths[g];
        length = length > o.max_steps ? o.max_steps : length;                          // (the buffers hold max_steps rows)
    }
    int longest = length;
#pragma unroll
    for (int d = 1; d < kWalkBlock; d <<= 1) longest = max(longest, __shfl_xor(longest, d, kWalkBlock));
    if (longest < 1) return;
    const size_t col = (size_t)(g < o.n_games ? g : o.n_games - 1);                    // a lane beyond the batch reads the last column, and writes nothing
    const double gl = __dmul_rn(o.gamma, o.lambda);
    double v[kRows], nv[kRows], b[Backed ? kRows : 1], nb[Backed ? kRows : 1];
    uint32_t s[kRows], ns[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const size_t at = (size_t)max(longest - 1 - j, 0) * B + col;
        v[j] = o.values[at]; s[j] = o.steps[at];
        if constexpr (Backed) b[j] = o.backed[at];
    }
    double above_v = 0.0, above_b = 0.0, big = 0.0;                                    // row t + 1's V and byte (its `backed`); D_{t+1}
    uint32_t above_s = 0u;
    for (int top = longest - 1; top >= 0; top -= kRows) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const size_t at = (size_t)max(top - kRows - j, 0) * B + col;
            nv[j] = o.values[at]; ns[j] = o.steps[at];
            if constexpr (Backed) nb[j] = o.backed[at];
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int t = top - j;
            const bool last = t == length - 1;
            double target;
            if constexpr (Backed) target = last ? 0.0 : above_b;
            else target = last ? 0.0 : td_target(above_s, above_v, o.gamma);
            const double delta = __dsub_rn(target, v[j]);
            const double carried = __dadd_rn(delta, __dmul_rn(gl, big));
            big = last ? ((s[j] & 0x80u) != 0u ? delta : 0.0) : carried;              // (a cut game's last move is skipped: +0.0)
            if (t >= 0 && t < length) o.deltas[(size_t)t * B + col] = big;
            above_v = v[j]; above_s = s[j];
            if constexpr (Backed) above_b = b[j];
        }
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            v[j] = nv[j]; s[j] = ns[j];
            if constexpr (Backed) b[j] = nb[j];
        }
    }
}

// ... and the launch of its first form, the TD(lambda) walk (defined in tfe_ntuple_lambda.hip, which instantiates it)
void launch_lambda_walk(const PulseTfeNtLearnLambda& o, void* stream);

// ... and of its second, the walk of backed[t + 1] - V_t (defined in tfe_ntuple_backed.hip, which instantiates it)
void launch_backed_walk(const WalkBacked& o, void* stream);

// `backed` and acc_abs of a learner's struct, null where the struct has no such field
inline const double* backed_of(const PulseTfeNtLearnBacked& o) { return o.backed; }
template <class O> const double* backed_of(const O&) { return nullptr; }
inline int64_t* acc_abs_of(const PulseTfeNtLearnLambda&) { return nullptr; }
template <class O> int64_t* acc_abs_of(const O& o) { return o.acc_abs; }

// What the learners with a lambda refuse after check_moves (pulse_tfe_nt_learn_lambda, _learn_tc, _learn_backed, _learn_staged).
// `need`: which of deltas, backed and acc_abs the entry point requires; one it does not require may be null, and deltas then only
// where neither `backed` nor a lambda above 0 asks for them.
enum : unsigned { kNeedDeltas = 1u, kNeedBacked = 2u, kNeedAccAbs = 4u };

template <class O>
int check_learner(const O* o, const char* name, const unsigned need) {
    const double* backed = backed_of(*o);
    const int64_t* acc_abs = acc_abs_of(*o);
    if (!(o->lambda >= 0.0 && o->lambda <= 1.0)) return fail_named(name, "lambda must be in [0, 1]");
    if (need & kNeedAccAbs) {                                                           // (who requires acc_abs refuses all of it first)
        if (!acc_abs) return fail_named(name, "acc_abs is null");
        if ((uintptr_t)acc_abs & 7u) return fail_named(name, "acc_abs must be 8-byte aligned");
    }
    if ((need & kNeedDeltas) && !o->deltas) return fail_named(name, "deltas is null");
    if ((need & kNeedBacked) && !backed) return fail_named(name, "backed is null");
    if (backed && !o->deltas) return fail_named(name, "deltas is null (backed needs them)");
    if (o->lambda > 0.0 && !o->deltas) return fail_named(name, "deltas is null (lambda > 0 needs them)");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->values & 7u) || ((uintptr_t)o->deltas & 7u) || ((uintptr_t)o->stats & 7u))
        return fail_named(name, "keys / values / deltas / stats must be 8-byte aligned");
    if ((uintptr_t)backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if ((uintptr_t)acc_abs & 7u) return fail_named(name, "acc_abs must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    return 0;
}

// ... and their hand-off after the checks: where the struct has deltas, the walk (Backed where it has `backed`), then the adds of
// what it left; m->acc_abs is the struct's
template <class O>
void launch_walk(const O* o, Moves* m, void* stream) {
    m->acc_abs = acc_abs_of(*o);
    if (!o->deltas) return;
    WalkBacked w{};
    w.n_games = o->n_games; w.max_steps = o->max_steps; w.gamma = o->gamma; w.lambda = o->lambda;
    w.values = o->values; w.steps = o->steps; w.lengths = o->lengths; w.deltas = o->deltas; w.backed = backed_of(*o);
    if (w.backed) launch_backed_walk(w, stream);
    else launch_lambda_walk(w, stream);
    m->deltas = o->deltas;
}

// what pulse_tfe_nt_rollout and pulse_tfe_nt_rollout_search refuse, and the game loop's parameters of a recording launch (defined in
// tfe_ntuple.hip)
int check_rollout(const PulseTfeNtRollout* o, const char* name, NtDev* dev, Games* g);

// what pulse_tfe_nt_evaluate and pulse_tfe_nt_evaluate_search refuse, and the game loop's parameters of an evaluation (defined in
// tfe_ntuple.hip)
int check_eval(const PulseTfeNtEval* o, const char* name, NtDev* dev, Games* g);

// The four moves of board `key`: the afterstates' keys and the merge scores
__device__ __forceinline__ void moves4(const uint64_t key, const uint32_t* __restrict__ lut, uint64_t (&ka)[4], int (&sc)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        PackedBoard m{(uint32_t)key, (uint32_t)(key >> 32)};
        sc[a] = tfe_move_packed(m, a, lut);
        ka[a] = (uint64_t)m.hi << 32 | m.lo;
    }
}

// the greedy action of pulse_tfe_nt_rollout on these q (-1: no candidate), and the candidates (the moves that change the board) as bit a
__device__ __forceinline__ int greedy_of(const double (&q)[4], const uint64_t key_b, const uint64_t (&ka)[4], uint64_t tie_seed, uint64_t round,
                                         uint32_t* bits = nullptr) {
    pulse_philox::U4 coins{0u, 0u, 0u, 0u};
    if (any_two_equal(q)) coins = pulse_philox::philox4x32(tie_seed, key_b, round);
    const bool cand[4] = {ka[0] != key_b, ka[1] != key_b, ka[2] != key_b, ka[3] != key_b};
    if (bits) *bits = (cand[0] ? 1u : 0u) | (cand[1] ? 2u : 0u) | (cand[2] ? 4u : 0u) | (cand[3] ? 8u : 0u);
    return greedy_scan<false>(q, coins, cand);
}

// the one-ply q of a board's four moves, q = r + gamma * V(afterstate), with V of the four afterstates left in v (what
// pulse_tfe_nt_rollout and pulse_tfe_nt_evaluate play on; tfe_ntuple_restart.hip's one-ply games too)
template <int IMG, class Net>
__device__ __forceinline__ void one_ply_q(const Net& net, const float* __restrict__ w, const double gamma, const uint64_t (&ka)[4], const int (&sc)[4],
                                          double (&v)[4], double (&q)[4]) {
    values4<IMG>(net, w, ka, v);
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = __dadd_rn((double)tfe_reward(sc[a]), __dmul_rn(gamma, v[a]));
}

// The game loop of the roll-out (Record) and of the two evaluations: game g of the launch, from its reset to its end, its cap or
// max_steps.  q_of(key_b, ka, sc, v, q) fills the four q of board key_b from its moves, and where the launch records also V of the
// four afterstates.  Backed (with Record): a move also records in o.backed the largest q over the moves that
// change the board -- scanned a = 0..3, the first candidate starts, a strictly larger q replaces it -- whatever the action taken.
// From (with Record): the game starts on the board packed in o.start[g] instead of its reset board where that
// board is usable -- not zero, changed by at least one of its four moves, no nibble 15 -- and otherwise at its reset, with 0 stored
// into o.start[g]; the draws, the counts and the records are those of a game that met this board at its move 0.  `writer`: this lane writes the game's outputs and counts it (a game that several lanes play alike has one).
// wg: the workgroup's zeroed LDS words, 2 with Record and kEvalBins without.  Called by every thread of the workgroup, whatever its g.
template <bool Record, bool Backed = false, bool From = false, class Q>
__device__ __forceinline__ void play_game(const Games& o, unsigned long long* wg, const int g, const bool writer, Q&& q_of) {
    using pulse_philox::philox4x32;
    using pulse_philox::U4;
    const size_t B = (size_t)o.n_games;
    unsigned long long n_moves = 0ull, n_cut = 0ull;
    if (g < o.n_games) {
        const uint64_t id = o.board_id0 + (uint64_t)g;
        PackedBoard p = tfe_reset_packed(o.env_seed, id);
        if constexpr (From) {
            const uint64_t key0 = o.start[g];                                           // (the same word in every lane that plays game g)
            const PackedBoard p0{(uint32_t)key0, (uint32_t)(key0 >> 32)};
            // A move changes a board without nibble 15 iff it is not zero and has an empty cell or two equal neighbours: the
            // environment's own test (a second moves4 here cost the one-lane kernel at IMG = 1 30 VGPRs and two waves, section 13.7)
            const bool full = (tfe_nz_nibbles(p0.lo) & tfe_nz_nibbles(p0.hi)) == 0x88888888u;
            const bool live = !tfe_over_packed(p0, full ? 0 : 2);
            if (key0 != 0ull && live && !has_nibble15(p0)) p = p0;
            else if (writer) o.start[g] = 0ull;
        }
        int64_t total = 0;
        int ep_reward = 0, length = 0;
        bool over = false, capped = false;
        unsigned long long n_greedy = 0ull;
        for (int t = 0; t < o.max_steps && !over && !capped; ++t) {
            const U4 r = philox4x32(o.agent_seed, id, (uint64_t)t);
            const uint64_t key_b = (uint64_t)p.hi << 32 | p.lo;
            uint64_t ka[4];
            int sc[4];
            moves4(key_b, o.lut, ka, sc);
            double v[4] = {0.0, 0.0, 0.0, 0.0}, q[4];
            q_of(key_b, ka, sc, v, q);
            const bool greedy = (r.x >> 8) >= o.eps_q24;
            int act = (int)(r.y >> 30);
            if (greedy) {
                const int best = greedy_of(q, key_b, ka, o.tie_seed, o.round);
                act = best < 0 ? act : best;                                            // (a live board has a candidate)
                n_greedy += 1ull;
            }
            double best_q = 0.0;
            if constexpr (Backed) {
                bool any = false;
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const bool cand = ka[a] != key_b;
                    best_q = cand && (!any || q[a] > best_q) ? q[a] : best_q;
                    any = any || cand;
                }
            }
            uint64_t key = ka[0];
            double val = v[0];
            int score = sc[0];
#pragma unroll
            for (int a = 1; a < 4; ++a) { key = act == a ? ka[a] : key; val = act == a ? v[a] : val; score = act == a ? sc[a] : score; }
            p.lo = (uint32_t)key; p.hi = (uint32_t)(key >> 32);                         // the afterstate's key IS the moved board
            const U4 rnd = philox4x32(o.env_seed, id, (uint64_t)t + 1ull);
            const int empty_before = tfe_spawn_packed(p, rnd.x, rnd.y);                // TFE.py:182 (always)
            over = tfe_over_packed(p, empty_before);                                   // TFE.py:48-67
            capped = has_nibble15(p);
            const int reward = tfe_reward(score);
            if constexpr (Record) {
                if (writer) {
                    const size_t at = (size_t)t * B + (size_t)g;
                    o.keys[at] = key;
                    o.values[at] = val;
                    o.steps[at] = tfe_step_byte(act, reward, over ? 1u : 0u);
                    if constexpr (Backed) o.backed[at] = best_q;
                }
            }
            total += score; ep_reward += reward;
            length = t + 1;
        }
        if (writer) {
            n_moves = (unsigned long long)length;
            n_cut = over ? 0ull : 1ull;
            if constexpr (Record) {
                o.lengths[g] = length;
                o.total_score[g] = total;
                o.episode_reward[g] = ep_reward;
            } else {
                if (o.lengths) o.lengths[g] = length;
                if (o.total_score) o.total_score[g] = total;
                uint32_t top = 0u;
#pragma unroll
                for (int i = 0; i < 8; ++i) top = max(top, max((p.lo >> (4 * i)) & 15u, (p.hi >> (4 * i)) & 15u));
                const unsigned long long s = (unsigned long long)total;
                add_game(wg, {1ull, n_moves, s, s * s, s, n_cut, n_greedy, capped ? 1ull : 0ull}, (int)top);
            }
        }
    }
    if constexpr (Record) add_stats(wg, o.stats, 0, n_moves, 3, n_cut);
    else flush_bins(wg, o.stats, o.hist);
}

}  // namespace pulse_tfe
