// tfe_ntuple_search_device.h -- what the units of the n-tuple network's play share (tfe_ntuple.hip: one ply; tfe_ntuple_search.hip: one
// chance layer, DESIGN.md section 13.1, two, section 13.4, and one or two by the board's empty cells, section 13.11;
// tfe_ntuple_search_rollout.hip, _backed.hip, _restart.hip and _staged.hip: the recording games, sections 13.5 to 13.13): the group of
// 32 lanes, the tile odds, the board launch's refusals (check_search), the chance layer itself (search_q_move, one move; search_q, the
// four in turn), the two-layer deal over a workgroup (search_q2 with live_slots and nth_set_bit), the choice between the two per board
// (search_q_adaptive, on the network as NtAdaptiveDev), the one board kernel (tfe_nt_search_kernel) with its launch ladder
// (launch_boards), and the one game kernel (tfe_nt_play_kernel) with its launch ladder (launch_play) and the step to it from an entry
// point's `backed` / `start` (launch_play_from).  One copy each.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "pulse_internal.h"
#include "tfe_device.h"
#include "tfe_ntuple_device.h"

namespace pulse_tfe {

constexpr int kSearchBlock = 256, kGroup = 32, kGroupsPerBlock = kSearchBlock / kGroup;

// the environment's tile odds (tfe_spawn_packed: the nibble is 2 iff r >> 8 > 15099494), exact doubles
constexpr double kP1 = 15099495.0 / 16777216.0, kP2 = 1677721.0 / 16777216.0;

// what pulse_tfe_nt_search and pulse_tfe_nt_search_deep refuse; fills the kernels' form of the network
inline int check_search(const PulseTfeNtSearch* o, const char* name, NtDev* dev) {
    if (!o) return fail_named(name, "options are null");
    if (int rc = check_net(o->net, true, name, dev)) return rc;
    if (o->n_boards < 1) return fail_named(name, "n_boards must be positive");
    if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (o->reserved0 != 0 || o->reserved1 != 0) return fail_named(name, "reserved0 / reserved1 must be 0 (zero-initialise the struct)");
    if (!o->boards) return fail_named(name, "boards is null");
    if (!o->q) return fail_named(name, "q is null");
    if (!o->action) return fail_named(name, "action is null");
    if (!o->candidates) return fail_named(name, "candidates is null");
    if (((uintptr_t)o->boards & 7u) || ((uintptr_t)o->q & 7u)) return fail_named(name, "boards / q must be 8-byte aligned");
    return 0;
}

// the depth beside the struct, as pulse_tfe_nt_search_deep, pulse_tfe_nt_evaluate_search_deep and pulse_tfe_nt_rollout_search take it
inline int check_layers(const int32_t layers, const char* name) {
    return layers == 1 || layers == 2 ? 0 : fail_named(name, "layers must be 1 or 2");
}

// ... and the threshold beside it, as the adaptive launches take it (tfe_ntuple_search.hip, tfe_ntuple_search_rollout.hip)
inline int check_deep_empty_max(const int32_t deep_empty_max, const char* name) {
    return deep_empty_max >= 0 && deep_empty_max <= 16 ? 0 : fail_named(name, "deep_empty_max must be in 0..16");
}

// ... and what pulse_tfe_nt_rollout_from and pulse_tfe_nt_rollout_staged refuse of theirs, of `backed` and of `start`
inline int check_start(const int32_t layers, const double* backed, const uint64_t* start, const char* name, const char* layers_message) {
    if (layers != 0 && layers != 1) return fail_named(name, layers_message);
    if (backed && layers == 0) return fail_named(name, "backed needs layers = 1: a one-ply roll-out has no search to back a value up");
    if ((uintptr_t)backed & 7u) return fail_named(name, "backed must be 8-byte aligned");
    if (!start) return fail_named(name, "start is null");
    if ((uintptr_t)start & 7u) return fail_named(name, "start must be 8-byte aligned");
    return 0;
}

__device__ __forceinline__ int count_empty(const uint64_t key) {
    return __popc(tfe_nz_nibbles((uint32_t)key) ^ 0x88888888u) + __popc(tfe_nz_nibbles((uint32_t)(key >> 32)) ^ 0x88888888u);
}

// q of ONE move of board `key_b` -- kb its afterstate, score its merge score -- by the 32 lanes of a group together; s = this lane's
// slot of kb: cell s / 2 with the tile 2 (s even) or 4 (s odd).  The chance layer, one copy: the lane's chance board, its four moves,
// values4, the term, the xor butterfly among the 32, the division.  Every lane of the group must call it with the same move, and
// every lane returns the same q; +0.0 for a move that does not change the board.
template <int IMG, class Net>
__device__ __forceinline__ double search_q_move(const Net& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                                const uint64_t key_b, const uint64_t kb, const int score, const int s) {
    const int cell4 = 4 * (s >> 1);
    const uint64_t tile = (uint64_t)((s & 1) + 1) << cell4;
    const double odds = (s & 1) ? kP2 : kP1;
    const bool candidate = kb != key_b;                                                 // (the same in the 32 lanes)
    double term = 0.0;
    if (candidate && ((kb >> cell4) & 15ull) == 0ull) {
        const uint64_t chance = kb | tile;
        uint64_t kc[4];
        int scc[4];
        moves4(chance, lut, kc, scc);
        double v[4];
        values4<IMG>(net, w, kc, v);
        double m = 0.0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double x = __dadd_rn((double)tfe_reward(scc[i]), __dmul_rn(gamma, v[i]));
            const bool cand = kc[i] != chance;
            m = cand && (!any || x > m) ? x : m;
            any = any || cand;
        }
        term = __dmul_rn(odds, m);
    }
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) term = __dadd_rn(term, __shfl_xor(term, d, kGroup));
    double qa = 0.0;
    if (candidate) qa = __dadd_rn((double)tfe_reward(score), __dmul_rn(gamma, __ddiv_rn(term, (double)count_empty(kb))));
    return qa;
}

// The four q of board `key_b` (its moves ka / sc given), by the 32 lanes of its group together; s = this lane's slot.  Every lane of
// the group must call it with the same board (the butterfly is among them), and every lane returns the same q.  A move that does
// not change the board has q = +0.0.  The loop over the moves is kept rolled: one copy of the chance layer in the code.
template <int IMG, class Net>
__device__ __forceinline__ void search_q(const Net& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                         const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], const int s, double (&q)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = 0.0;
#pragma unroll 1
    for (int a = 0; a < 4; ++a) {
        uint64_t kb = ka[0];
        int score = sc[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) { kb = a == i ? ka[i] : kb; score = a == i ? sc[i] : score; }
        const double qa = search_q_move<IMG>(net, w, lut, gamma, key_b, kb, score, s);
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = a == i ? qa : q[i];
    }
}

// bit s of the result: slot s of B_a = kb holds a child (the cell 2 s and 2 s + 1 share is empty); 0 for a move that is no candidate
__device__ __forceinline__ uint32_t live_slots(const uint64_t kb, const uint64_t key_b) {
    const uint32_t lo = tfe_nz_nibbles((uint32_t)kb) ^ 0x88888888u, hi = tfe_nz_nibbles((uint32_t)(kb >> 32)) ^ 0x88888888u;   // bit 4 c + 3: cell c is empty
    uint32_t m = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        m |= ((lo >> (4 * c + 3)) & 1u) * (3u << (2 * c));
        m |= ((hi >> (4 * c + 3)) & 1u) * (3u << (2 * c + 16));
    }
    return kb != key_b ? m : 0u;
}

// the position of set bit number k (from 0, upwards) of m; k < popc(m)
__device__ __forceinline__ int nth_set_bit(uint32_t m, int k) {
    int pos = 0;
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        const int c = __popc(m & ((1u << w) - 1u));
        const bool up = k >= c;
        k = up ? k - c : k;
        m = up ? m >> w : m;
        pos = up ? pos + w : pos;
    }
    return pos;
}

// The four q of board `key_b` (its moves ka / sc given) under two chance layers, by the 256 lanes of the workgroup together.  Every
// lane of the workgroup must call it, with the same board, the same number of times (two workgroup barriers a call); every lane
// returns the same q.  terms: 4 * 32 doubles of LDS, which need no initial value.
template <int IMG>
__device__ __forceinline__ void search_q2(const NtDev& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                          const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double* terms, double (&q)[4]) {
    const int group = (int)threadIdx.x >> 5, s = (int)threadIdx.x & (kGroup - 1);
    uint32_t live[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) live[a] = live_slots(ka[a], key_b);
    const int n0 = __popc(live[0]), n1 = n0 + __popc(live[1]), n2 = n1 + __popc(live[2]), total = n2 + __popc(live[3]);
    __syncthreads();                                                                    // the rows of the call before have been read
#pragma unroll 1
    for (int n = group; n < total; n += kGroupsPerBlock) {                              // (the same in the 32 lanes of a group)
        const int a = (n >= n0) + (n >= n1) + (n >= n2);
        const int k = n - (a == 0 ? 0 : a == 1 ? n0 : a == 2 ? n1 : n2);
        uint64_t kb = ka[0];
        uint32_t m = live[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) { kb = a == i ? ka[i] : kb; m = a == i ? live[i] : m; }
        const int slot = nth_set_bit(m, k);
        const uint64_t chance = kb | (uint64_t)((slot & 1) + 1) << (4 * (slot >> 1));
        uint64_t kc[4];
        int scc[4];
        moves4(chance, lut, kc, scc);
        double qc[4];
        search_q<IMG>(net, w, lut, gamma, chance, kc, scc, s, qc);
        double best = 0.0;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool cand = kc[i] != chance;
            best = cand && (!any || qc[i] > best) ? qc[i] : best;
            any = any || cand;
        }
        if (s == 0) terms[a * kGroup + slot] = __dmul_rn((slot & 1) ? kP2 : kP1, best);  // (a, slot) < 4 * 32: inside the rows
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double term = (live[a] >> s) & 1u ? terms[a * kGroup + s] : 0.0;
#pragma unroll
        for (int d = 1; d < kGroup; d <<= 1) term = __dadd_rn(term, __shfl_xor(term, d, kGroup));
        q[a] = 0.0;
        if (ka[a] != key_b) q[a] = __dadd_rn((double)tfe_reward(sc[a]), __dmul_rn(gamma, __ddiv_rn(term, (double)count_empty(ka[a]))));
    }
}

// The four q of board `key_b` at the depth its empty cells choose, by the 256 lanes of the workgroup
// together: with count_empty(key_b) <= deep_empty_max search_q2, two chance layers; otherwise the one-layer q of search_q, the four
// moves side by side: group a < 4 runs search_q_move on move a and its lane 0 stores q_a into qs[a], groups 4..7 only meet the
// barriers.  Every lane of the workgroup must call it, with the same board, the same number of times; every lane returns the same q
// and the same `deep`.  The branch depends on the board alone, so the 256 lanes take it alike and meet the same two barriers a
// call on either side.  terms: search_q2's rows; qs: 4 doubles of LDS of their own, which need no initial value.
template <int IMG>
__device__ __forceinline__ bool search_q_adaptive(const NtDev& net, const float* __restrict__ w, const uint32_t* __restrict__ lut, const double gamma,
                                                  const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], const int deep_empty_max,
                                                  double* terms, double* qs, double (&q)[4]) {
    // (the same in the 256 lanes; read from the first, so that the compiler knows it too and the branch is a scalar one)
    const bool deep = __builtin_amdgcn_readfirstlane(count_empty(key_b)) <= deep_empty_max;
    if (deep) {
        search_q2<IMG>(net, w, lut, gamma, key_b, ka, sc, terms, q);
    } else {
        const int group = (int)threadIdx.x >> 5, s = (int)threadIdx.x & (kGroup - 1);
        __syncthreads();                                                                // the four q of the shallow call before have been read
        if (group < 4) {                                                                // (the same in the 32 lanes of a group; no barrier inside)
            uint64_t kb = ka[0];
            int score = sc[0];
#pragma unroll
            for (int i = 1; i < 4; ++i) { kb = group == i ? ka[i] : kb; score = group == i ? sc[i] : score; }
            const double qa = search_q_move<IMG>(net, w, lut, gamma, key_b, kb, score, s);
            if (s == 0) qs[group] = qa;                                                 // group < 4: inside the four words
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) q[a] = qs[a];
    }
    return deep;
}

// The one-stage network under that choice, as the adaptive launches hand it to the board and the game kernel: the threshold, and
// where a game adds its moves at each depth -- [0] += those whose q came from two layers, [1] += those from one; null for boards, and
// for games nobody counts.  Derived, as NtStagedDev is, so that the kernels of the fixed depths keep their arguments and their names.
struct NtAdaptiveDev : NtDev {
    int32_t deep_empty_max;
    unsigned long long* depth_stats;
};

template <class Net>
inline constexpr bool kAdaptive = std::is_same_v<Net, NtAdaptiveDev>;

inline NtAdaptiveDev adaptive_of(const NtDev& dev, const int32_t deep_empty_max, int64_t* depth_stats) {
    return NtAdaptiveDev{dev, deep_empty_max, reinterpret_cast<unsigned long long*>(depth_stats)};
}

// pulse_tfe_nt_search's struct as the board kernel takes it
struct Boards {
    const float* weights;
    int32_t n_boards;
    double gamma;
    uint64_t tie_seed, round;
    const uint64_t* boards;
    double* q; int8_t* action; uint8_t* candidates;
    const uint32_t* lut;
};

// The one board kernel: the four q of board g, its greedy action and its candidates, on one of two mappings of a board to lanes, each
// with its q.  32 lanes per board: search_q, and a group beyond the batch leaves at once (nothing below meets the workgroup).  A
// workgroup per board: g is blockIdx.x (grid = n_boards), so the 256 lanes carry the board alike and meet the two barriers of
// search_q2 -- of search_q_adaptive on NtAdaptiveDev, on either side of the branch the board alone decides -- together.  The first lane
// of the board's lanes writes.
template <int LANES /* 32 (kGroup) or 256 (kSearchBlock) per board */, int IMG, class Net>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_search_kernel(const Boards o, const Net net) {
    static_assert(LANES == kGroup || (LANES == kSearchBlock && !kStaged<Net>), "search_q2 takes the one-stage network only");
    static_assert(!kAdaptive<Net> || LANES == kSearchBlock, "search_q_adaptive is a workgroup's");
    const int g = LANES == kGroup ? (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5) : (int)blockIdx.x;
    if constexpr (LANES == kGroup) {
        if (g >= o.n_boards) return;
    }
    const uint64_t key_b = o.boards[g];
    uint64_t ka[4];
    int sc[4];
    moves4(key_b, o.lut, ka, sc);
    double q[4];
    if constexpr (LANES == kGroup) {
        search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, (int)threadIdx.x & (kGroup - 1), q);
    } else {
        __shared__ double terms[4 * kGroup];
        if constexpr (kAdaptive<Net>) {
            __shared__ double qs[4];
            search_q_adaptive<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, net.deep_empty_max, terms, qs, q);
        } else {
            search_q2<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, terms, q);
        }
    }
    uint32_t bits;
    const int best = greedy_of(q, key_b, ka, o.tie_seed, o.round, &bits);
    if (((int)threadIdx.x & (LANES - 1)) == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) o.q[(size_t)g * 4 + a] = q[a];
        o.action[g] = (int8_t)best;
        o.candidates[g] = (uint8_t)bits;
    }
}

// The one launch ladder of the boards, after the checks: the mapping of `layers` (1: 32 lanes per board, 2: 256), which the caller has
// checked to be one its network has -- the staged network one layer, the adaptive network (the threshold in it) the workgroup alone.
template <class Net>
void launch_boards(const int layers, const PulseTfeNtSearch& o, const Net& net, const uint32_t* lut, void* stream) {
    const Boards b{o.net.weights, o.n_boards, o.gamma, o.tie_seed, o.round, o.boards, o.q, o.action, o.candidates, lut};
    const auto launch = [&](auto lanes) {
        constexpr int LANES = decltype(lanes)::value;
        const dim3 grid((unsigned)(((int64_t)o.n_boards * LANES + kSearchBlock - 1) / kSearchBlock)), block(kSearchBlock);
        if (o.net.symmetric) hipLaunchKernelGGL((tfe_nt_search_kernel<LANES, 8, Net>), grid, block, 0, (hipStream_t)stream, b, net);
        else hipLaunchKernelGGL((tfe_nt_search_kernel<LANES, 1, Net>), grid, block, 0, (hipStream_t)stream, b, net);
    };
    if constexpr (!kAdaptive<Net>) {
        if (layers == 1) launch(std::integral_constant<int, kGroup>{});
    }
    if constexpr (!kStaged<Net>) {
        if (layers == 2) launch(std::integral_constant<int, kSearchBlock>{});
    }
}

// The one game kernel: play_game<Record, Backed, From> on one of three mappings of a game to lanes, each with the q its policy plays on.
template <int LANES /* 1, 32 (kGroup) or 256 (kSearchBlock) per game */, int IMG, bool Record, bool Backed, bool From, class Net>
__global__ __launch_bounds__(kSearchBlock) void tfe_nt_play_kernel(const Games o, const Net net) {
    static_assert(!kAdaptive<Net> || (LANES == kSearchBlock && !kStaged<Net>), "search_q_adaptive is a workgroup's, on the one-stage network");
    constexpr int kCounters = Record ? 2 : kEvalBins;
    __shared__ unsigned long long wg[kCounters];
    if (threadIdx.x < kCounters) wg[threadIdx.x] = 0ull;
    if constexpr (LANES == 1) {
        // one lane plays one game: q = r + gamma * V
        static_assert(kSearchBlock == 256, "the one-lane mapping's workgroup is the 256 lanes (kBlock) of its units' other kernels");
        __syncthreads();
        play_game<Record, Backed, From>(o, wg, blockIdx.x * kSearchBlock + threadIdx.x, true,
                                        [&](const uint64_t, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                            one_ply_q<IMG>(net, o.weights, o.gamma, ka, sc, v, q);
                                        });
    } else if constexpr (LANES == kGroup) {
        // One game per group of 32 lanes, which play it alike -- the same start[g], boards, draws and four afterstates, so the gathers
        // are uniform -- and lane 0 of the group writes and counts.  g < n_games is the same in the 32, and a group beyond the batch
        // only meets the barrier of the counts.  A recording launch records the NETWORK's V of the chosen afterstate, not the search's
        // backed-up value: values4 runs before the search starts, so that its indices and loaded words are dead by then and eight
        // registers (the four doubles) live across the search.
        __syncthreads();
        const int g = (int)blockIdx.x * kGroupsPerBlock + ((int)threadIdx.x >> 5), s = (int)threadIdx.x & (kGroup - 1);
        play_game<Record, Backed, From>(o, wg, g, s == 0,
                                        [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                            if constexpr (Record) values4<IMG>(net, o.weights, ka, v);
                                            search_q<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, s, q);
                                        });
    } else {
        // One game per workgroup: g is blockIdx.x (grid = n_games), so the 256 lanes play the game alike -- the same boards, draws and
        // length -- and thread 0 writes and counts.  Nothing lane-dependent encloses q_of: search_q2's two barriers per move --
        // search_q_adaptive's, on either side of a branch the board alone decides -- are reached by the 256 lanes together, which
        // leave the loop at the same move, and `writer` guards stores only, with Record, Backed and From alike.
        // From: thread 0 stores 0 into an unusable start[g] while a slower wavefront may not have read the word yet.  The word is
        // 8-byte aligned (the entry points check it) and read and written as one 64-bit access, so such a lane reads either the
        // unusable word as it was or 0; 0 is itself unusable (play_game tests key0 != 0 first), so every lane falls back to the reset
        // board: the four wavefronts decide alike whichever they read.  A usable word is never written.
        // On NtAdaptiveDev (DESIGN.md sections 13.11 and 13.13) the q is search_q_adaptive's, with four LDS words of its own, and the
        // closure counts the moves at each depth; thread 0 adds the two counts once, after the game.
        static_assert(LANES == kSearchBlock, "a game is played by 1, 32 or 256 lanes");
        __shared__ double terms[4 * kGroup];
        __syncthreads();
        [[maybe_unused]] uint32_t depths = 0u;                                         // deep moves + 65,536 * shallow moves: a game has at most 65,535
        play_game<Record, Backed, From>(o, wg, (int)blockIdx.x, threadIdx.x == 0,
                                        [&](const uint64_t key_b, const uint64_t (&ka)[4], const int (&sc)[4], double (&v)[4], double (&q)[4]) {
                                            if constexpr (Record) values4<IMG>(net, o.weights, ka, v);
                                            if constexpr (kAdaptive<Net>) {
                                                __shared__ double qs[4];
                                                const bool deep = search_q_adaptive<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, net.deep_empty_max, terms, qs, q);
                                                depths += deep ? 1u : 65536u;
                                            } else {
                                                search_q2<IMG>(net, o.weights, o.lut, o.gamma, key_b, ka, sc, terms, q);
                                            }
                                        });
        if constexpr (kAdaptive<Net>) {
            if (threadIdx.x == 0 && net.depth_stats) {
                atomicAdd(net.depth_stats, (unsigned long long)(depths & 65535u));
                atomicAdd(net.depth_stats + 1, (unsigned long long)(depths >> 16));
            }
        }
    }
}

// The one launch ladder of the games, after the checks: fetches the row table, and launches the mapping of `layers` (0: one lane
// per game, 1: 32, 2: 256), which the caller has checked to be in MinLayers..MaxLayers -- the depths its unit builds, so a unit
// instantiates the kernels it can launch and no others.  A backed value needs a search: Backed builds no one-ply form.  The adaptive
// network (the threshold and the counts' address in it) has the 256-lane mapping alone: its launches say 2 .. 2.
template <bool Record, int MinLayers, int MaxLayers, bool Backed = false, bool From = false, class Net>
int launch_play(const int layers, Games& g, const Net& net, const bool symmetric, void* stream) {
    static_assert(0 <= MinLayers && MinLayers <= MaxLayers && MaxLayers <= (kStaged<Net> ? 1 : 2), "search_q2 takes the one-stage network only");
    static_assert(!kAdaptive<Net> || MinLayers == 2, "search_q_adaptive is a workgroup's");
    if (int rc = pulse::tfe_row_lut(&g.lut)) return rc;
    const auto launch = [&](auto lanes) {
        constexpr int LANES = decltype(lanes)::value;
        const dim3 grid((unsigned)(((int64_t)g.n_games * LANES + kSearchBlock - 1) / kSearchBlock)), block(kSearchBlock);
        if (symmetric) hipLaunchKernelGGL((tfe_nt_play_kernel<LANES, 8, Record, Backed, From, Net>), grid, block, 0, (hipStream_t)stream, g, net);
        else hipLaunchKernelGGL((tfe_nt_play_kernel<LANES, 1, Record, Backed, From, Net>), grid, block, 0, (hipStream_t)stream, g, net);
    };
    if constexpr (MinLayers == 0 && !Backed) {
        if (layers == 0) launch(std::integral_constant<int, 1>{});
    }
    if constexpr (MinLayers <= 1 && MaxLayers >= 1) {
        if (layers == 1) launch(std::integral_constant<int, kGroup>{});
    }
    if constexpr (MaxLayers == 2) {
        if (layers == 2) launch(std::integral_constant<int, kSearchBlock>{});
    }
    return 0;
}

// The one step from `backed` / `start` as a recording entry point got them (either may be null) to launch_play's Backed / From, with
// g.backed / g.start set.  NeedStart: the entry point has refused a null `start`, so its unit builds no form without From.
template <int MinLayers, int MaxLayers, bool NeedStart, class Net>
int launch_play_from(const int layers, Games& g, double* backed, uint64_t* start, const Net& net, const bool symmetric, void* stream) {
    g.backed = backed;
    g.start = start;
    const auto launch = [&](auto with_backed, auto from) {
        return launch_play<true, MinLayers, MaxLayers, decltype(with_backed)::value, decltype(from)::value>(layers, g, net, symmetric, stream);
    };
    if constexpr (!NeedStart) {
        if (!start) return backed ? launch(std::true_type{}, std::false_type{}) : launch(std::false_type{}, std::false_type{});
    }
    return backed ? launch(std::true_type{}, std::true_type{}) : launch(std::false_type{}, std::true_type{});
}

}  // namespace pulse_tfe
