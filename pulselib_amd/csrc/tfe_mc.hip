// tfe_mc.hip -- on-policy first-visit Monte-Carlo control for 2048 (agents/MonteCarlo/OnPolicyFirstVisit.py:6-71 on the games of
// scripts/TFE/mctrain.py) as two launches per batch of games: pulse_tfe_mc_rollout and pulse_tfe_mc_learn.
//
// The reference steps one board through the interpreter, keeps the episode in a list and the pairs it has seen in a set.  Here one
// lane plays one game from reset to the terminal step with the board in registers (tfe_device.h: the env kernels' own move, spawn
// and game-over test, drawing from the env's own Philox stream, so game (env_seed, board id) IS the game pulse_tfe_reset +
// pulse_tfe_step play under the same actions) against a policy read from a hash table of states in HBM, and writes one key and one
// byte per move, step-major (a wavefront's stores of a step are one run of 512 + 64 bytes).  The table is read-only in that launch.
// A second launch walks every game backwards and adds the first-visit returns into the table as fixed-point integers: the adds
// commute, so the table as a map does not depend on the order of the atomics.
//
// First visits without a per-game set: a merge keeps the tile sum and a spawn adds to it, so the sum rises at every step unless the
// board is full and the move changes nothing -- equal states of a game are consecutive, and "first visit of (s, a)" is "a was not
// yet taken in the current run of identical boards": four bits per lane.
//
// The same game loop has two more instantiations.  Canon: the state is the smallest key among the board's
// eight images under the symmetries of the square, the greedy action is taken in that image's frame and mapped back
// (pulse_tfe_mc_rollout_canon).  Not Record: no trajectory is written and the scores are reduced in the launch
// (pulse_tfe_mc_evaluate).  The table is only read by all of them.
//
// pulse_tfe_mc_table_merge adds one array of entries into a table by key: growing, folding a plain table
// into a symmetric one, adding two agents' tables and loading a checkpoint are that one launch.
//
// After: the table holds V(afterstate) -- the board after the move and before the spawn -- in cnt[0] / sum[0]
// of the afterstate's key.  The game loop looks up the four afterstates of a board and takes the largest reward + gamma * v
// (pulse_tfe_mc_rollout_after, _after_canon, pulse_tfe_mc_evaluate_after), the learner adds the return that FOLLOWS a step
// (pulse_tfe_mc_learn_after), and the fold keeps the slots where they are (pulse_tfe_mc_table_fold_after).
#include <hip/hip_runtime.h>

#include <cmath>

#include "philox_device.h"
#include "pulse_internal.h"
#include "tfe_agent_device.h"
#include "tfe_device.h"
#include "tfe_table_device.h"

namespace {

using namespace pulse_tfe;
using pulse_philox::philox4x32;
using pulse_philox::U4;
using pulse::fail_named;
using pulse::finish_launch;

constexpr int kBlock = 256;
constexpr uint64_t kMaxProbe = PULSE_TFE_MC_MAX_PROBE;

// one table entry = one 128-byte line
struct alignas(128) Entry { unsigned long long key; long long cnt[4]; long long sum[4]; unsigned long long spare[7]; };
static_assert(sizeof(Entry) == PULSE_TFE_MC_ENTRY_BYTES, "entry layout is part of the ABI");

// The greedy action of an entry (greedy_scan over its four q; the coins' key is the key of the entry).
__device__ __forceinline__ int greedy_action(const Entry& e, uint64_t key, uint64_t tie_seed, uint64_t round, double inv_scale) {
    double q[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long long n = e.cnt[a];
        q[a] = n > 0 ? __dmul_rn(__ddiv_rn((double)e.sum[a], (double)n), inv_scale) : 0.0;   // an unseen pair reads 0.0 (defaultdict(float))
    }
    U4 coins{0u, 0u, 0u, 0u};
    if (any_two_equal(q)) coins = philox4x32(tie_seed, key, round);
    return greedy_scan(q, coins);
}

// The eight symmetries of the square, T_0 .. T_7: T_j rotates the board j & 3 times by the move's own rotation (rot_src), for
// j >= 4 after a transpose.  sym_src = the cell of the board that cell (r, c) of T_j(board) shows.
template <int NB>
__device__ __forceinline__ int sym_src(int j, int r, int c) {
    const int i = rot_src<NB>(j & 3, r, c);
    return j >= 4 ? (i % NB) * NB + i / NB : i;
}
// kActionMap >> (8 j + 2 a) & 3 = the action with T_j(move(B, a)) == move(T_j(B), that action); kActionUnmap is its inverse per j.
// (ACTION_MAP / ACTION_UNMAP of agents/tfe_on_policy_mc_gpu.py, which a test holds to the environment's move.)
constexpr uint64_t kActionMap = 0xc61b6cb1394e93e4ull, kActionUnmap = 0xc61b6cb1934e39e4ull;
__device__ __forceinline__ int map_action(uint64_t map, int j, int a) { return (int)((map >> (8 * j + 2 * a)) & 3ull); }

// (key_c, j*) of a board: the smallest of the keys of its eight images and the smallest j whose image has it.  The cells' nibbles
// (e) are taken once; every image is NB * NB shift-ors of them at constant positions -- registers only.
template <int NB>
__device__ __forceinline__ uint64_t canon_nibbles(const uint32_t (&e)[NB * NB], int& j_min) {
    uint64_t best = 0ull;
    j_min = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int i = r * NB + c;
                const uint32_t v = e[sym_src<NB>(j, r, c)] << (4 * (i & 7));
                if (i < 8) lo |= v; else hi |= v;
            }
        const uint64_t key = (uint64_t)hi << 32 | lo;
        const bool less = j > 0 && key < best;
        j_min = less ? j : j_min;
        best = j == 0 || less ? key : best;
    }
    return best;
}
// ... of a board of tiles (the roll-outs), and of a state key (the merge launch): one text of the images above for both
template <int NB>
__device__ __forceinline__ uint64_t canon_key(const int (&b)[NB * NB], int& j_min) {
    uint32_t e[NB * NB];
#pragma unroll
    for (int i = 0; i < NB * NB; ++i) e[i] = b[i] > 0 ? (uint32_t)min(31 - __clz(b[i]), 15) : 0u;         // pack_cells' nibble
    return canon_nibbles<NB>(e, j_min);
}
template <int NB>
__device__ __forceinline__ uint64_t canon_of_key(uint64_t key, int& j_min) {
    uint32_t e[NB * NB];
#pragma unroll
    for (int i = 0; i < NB * NB; ++i) e[i] = (uint32_t)(key >> (4 * i)) & 15u;
    return canon_nibbles<NB>(e, j_min);
}

// A value table's entry of `key`: find() with the first slot's key, cnt[0] and sum[0] already loaded by the
// caller -- the four afterstates of a move load theirs before any of them is compared, so the four lines are in flight together.
// The same slots in the same order as find(): the first was examined by the caller, probes 1 .. limit - 1 follow here.
struct Value { long long cnt, sum; bool hit; };
__device__ __forceinline__ Value value_after_first(const Entry* table, uint64_t slots, uint64_t key, uint64_t h, unsigned long long key0, long long cnt0, long long sum0) {
    if (key0 == key) return Value{cnt0, sum0, true};
    if (key0 == 0ull) return Value{0, 0, false};
    const uint64_t limit = slots < kMaxProbe ? slots : kMaxProbe;
    for (uint64_t probe = 1; probe < limit; ++probe) {
        const Entry& e = table[(h + probe) & (slots - 1)];
        const unsigned long long cur = e.key;
        if (cur == key) return Value{e.cnt[0], e.sum[0], true};
        if (cur == 0ull) break;
    }
    return Value{0, 0, false};
}

// The action of the afterstate policy on board b, a = 0..3 as the board lies (a value has no frame), and the key of the afterstate it
// leads to.  any: one of the four keys had an entry; greedy: and it was not the epsilon branch.  r = this move's agent draw.
template <int NB, bool Canon>
__device__ __forceinline__ int afterstate_action(const int (&b)[NB * NB], const Entry* table, const PulseTfeMCRollout& o, uint32_t eps_q24,
                                                 double inv_scale, const U4& r, uint64_t& key, bool& any, bool& greedy) {
    // The four afterstates: keys and rewards only -- the caller moves the board itself again by the action returned.  One move at
    // a time (not unrolled): the moved board is dead once its key is formed, and the kernel holds one text of the move for the four.
    uint64_t ka[4] = {0ull, 0ull, 0ull, 0ull};
    int ra[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        int c[NB * NB];
#pragma unroll
        for (int x = 0; x < NB * NB; ++x) c[x] = b[x];
        const int sc = tfe_move<NB>(c, i);
        const int rw = tfe_reward(sc);
        int jc = 0;
        uint64_t k;
        if constexpr (Canon) k = canon_key<NB>(c, jc); else k = pack_cells<NB * NB>(c);
#pragma unroll
        for (int x = 0; x < 4; ++x) { ka[x] = x == i ? k : ka[x]; ra[x] = x == i ? rw : ra[x]; }      // (selects, not addresses)
    }
    uint64_t h[4];
    unsigned long long k0[4];
    long long c0[4], s0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = mix64(ka[i]) & (o.capacity - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) { k0[i] = table[h[i]].key; c0[i] = table[h[i]].cnt[0]; s0[i] = table[h[i]].sum[0]; }
    double q[4];
    any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const Value v = value_after_first(table, o.capacity, ka[i], h[i], k0[i], c0[i], s0[i]);
        any = any || v.hit;
        const double val = v.cnt > 0 ? __dmul_rn(__ddiv_rn((double)v.sum, (double)v.cnt), inv_scale) : 0.0;
        q[i] = __dadd_rn((double)ra[i], __dmul_rn(o.gamma, val));
    }
    greedy = any && (r.x >> 8) >= eps_q24;
    int a = (int)(r.y >> 30);                             // no entry among the four, or the epsilon branch
    if (greedy) {
        U4 coins{0u, 0u, 0u, 0u};
        if (any_two_equal(q)) coins = philox4x32(o.tie_seed, pack_cells<NB * NB>(b), o.round);     // the plain key of the state, in both forms
        a = greedy_scan(q, coins);
    }
    key = ka[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) key = a == i ? ka[i] : key;
    return a;
}

// The game loop.  <NB, false, true, false> is pulse_tfe_mc_rollout; Canon plays in the canonical frame; without Record nothing is
// written per move, lengths / total_score are optional, o.stats is the evaluation's summary[8] and `hist` its max_tile_hist[16].
// After: the policy reads the values of the board's four afterstates and the afterstate of the move taken is what is recorded.
template <int NB, bool Canon, bool Record, bool After>
__global__ __launch_bounds__(kBlock) void tfe_mc_rollout_kernel(const PulseTfeMCRollout o, uint32_t eps_q24, double inv_scale, int64_t* hist) {
    __shared__ unsigned long long wg[Record ? 2 : kEvalBins];
    if (threadIdx.x < (Record ? 2 : kEvalBins)) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const size_t B = (size_t)o.n_games;
    unsigned long long n_moves = 0ull, n_cut = 0ull;
    if (g < o.n_games) {
        const Entry* table = static_cast<const Entry*>(o.entries);
        const uint64_t id = o.board_id0 + (uint64_t)g;
        int b[NB * NB];
        tfe_reset<NB>(b, o.env_seed, id);
        int64_t total = 0;
        int ep_reward = 0, length = 0;
        uint32_t taken = 0u;                              // bit a: action a was taken in the current run of identical boards
        uint64_t prev_key = 0ull;                         // (no live board packs to 0)
        bool over = false;
        unsigned long long n_present = 0ull, n_greedy = 0ull;
        for (int t = 0; t < o.max_steps && !over; ++t) {
            int a, score;                                 // a: the action in the frame of `key`
            uint64_t key;
            uint32_t first;
            const U4 r = philox4x32(o.agent_seed, id, (uint64_t)t);
            if constexpr (After) {
                bool any, greedy;
                a = afterstate_action<NB, Canon>(b, table, o, eps_q24, inv_scale, r, key, any, greedy);
                if constexpr (!Record) { n_present += any; n_greedy += greedy; }
                first = key != prev_key ? 1u : 0u;        // equal afterstates of a game are consecutive
                prev_key = key;
                score = tfe_move<NB>(b, a);               // the board moves again, so the four moved boards were never kept
            } else {
                int j = 0;                                // the board shows its canonical state under T_j
                if constexpr (Canon) key = canon_key<NB>(b, j); else key = pack_cells<NB * NB>(b);
                taken = key == prev_key ? taken : 0u;
                prev_key = key;
                const long long s = find<kMaxProbe>(table, 0, o.capacity, key);
                a = (int)(r.y >> 30);                     // no entry: the reference's uniform default policy; or the epsilon branch
                if constexpr (Canon) a = map_action(kActionMap, j, a);                     // a: the action in the frame of `key`
                if (s >= 0 && (r.x >> 8) >= eps_q24) a = greedy_action(table[s], key, o.tie_seed, o.round, inv_scale);
                if constexpr (!Record) { n_present += s >= 0; n_greedy += s >= 0 && (r.x >> 8) >= eps_q24; }
                int a_board = a;                                                           // ... and as the board lies
                if constexpr (Canon) a_board = map_action(kActionUnmap, j, a);
                score = tfe_move<NB>(b, a_board);                                          // TFE.py:154-178
                first = ((taken >> a) & 1u) ^ 1u;
                taken |= 1u << a;
            }
            const U4 rnd = philox4x32(o.env_seed, id, (uint64_t)t + 1ull);
            tfe_spawn<NB>(b, rnd.x, rnd.y);                                            // TFE.py:182 (always)
            over = tfe_over<NB>(b);                                                    // TFE.py:48-67
            const int reward = tfe_reward(score);
            if constexpr (Record) {
                o.keys[(size_t)t * B + (size_t)g] = key;
                o.steps[(size_t)t * B + (size_t)g] = tfe_step_byte(a, reward, first);
            }
            total += score; ep_reward += reward;
            length = t + 1;
        }
        n_moves = (unsigned long long)length;
        n_cut = over ? 0ull : 1ull;
        if constexpr (Record) {
            o.lengths[g] = length;
            o.total_score[g] = total;
            o.episode_reward[g] = ep_reward;
        } else {
            if (o.lengths) o.lengths[g] = length;
            if (o.total_score) o.total_score[g] = total;
            int top = 0;
#pragma unroll
            for (int i = 0; i < NB * NB; ++i) top = max(top, b[i]);
            const unsigned long long sc = (unsigned long long)total;
            add_game(wg, {1ull, n_moves, sc, sc * sc, sc, n_cut, n_present, n_greedy}, min(31 - __clz(top | 1), 15));
        }
    }
    if constexpr (Record) add_stats(wg, o.stats, 0, n_moves, 3, n_cut);
    else flush_bins(wg, o.stats, hist);
}

// After: a flagged step adds the return that FOLLOWS it (G before this step's reward enters) to cnt[0] / sum[0] of its key.
template <bool After>
__global__ __launch_bounds__(kBlock) void tfe_mc_learn_kernel(const PulseTfeMCLearn o) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const size_t B = (size_t)o.n_games;
    unsigned long long n_added = 0ull, n_dropped = 0ull;
    if (g < o.n_games) {
        Entry* table = static_cast<Entry*>(o.entries);
        int length = o.lengths[g];
        length = length < 0 ? 0 : (length > o.max_steps ? o.max_steps : length);       // (the buffers hold max_steps rows)
        double G = 0.0;
        for (int t = length - 1; t >= 0; --t) {
            const uint32_t st = o.steps[(size_t)t * B + (size_t)g];
            if constexpr (!After) G = __dadd_rn(__dmul_rn(o.gamma, G), (double)((st >> 2) & 31u));    // OnPolicyFirstVisit.py:28: G = gamma * G + reward
            if (st & 0x80u) {
                const uint64_t key = o.keys[(size_t)t * B + (size_t)g];
                const long long s = key ? find_or_insert<kMaxProbe>(table, 0, o.capacity, key) : -1;
                if (s >= 0) {
                    const int a = After ? 0 : (int)(st & 3u);
                    atomicAdd(reinterpret_cast<unsigned long long*>(&table[s].sum[a]), (unsigned long long)llrint(ldexp(G, o.frac_bits)));
                    atomicAdd(reinterpret_cast<unsigned long long*>(&table[s].cnt[a]), 1ull);
                    n_added += 1ull;
                } else {
                    n_dropped += 1ull;
                }
            }
            if constexpr (After) G = __dadd_rn(__dmul_rn(o.gamma, G), (double)((st >> 2) & 31u));
        }
    }
    add_stats(wg, o.stats, 1, n_added, 2, n_dropped);
}

// dst += src over entries (pulse_tfe_mc_table_merge).  One lane per SOURCE slot: the source is scanned, not
// probed, and an empty slot costs its one line whatever the mapping, so lanes per entry would save no traffic.  NB = 0: keys as they
// are; NB = 2..4: every key goes to its canonical key with the eight values permuted by amap[j*] (the fold).  The adds are the
// learner's integer atomics, so dst as a map does not depend on the order; an entry with no room adds nothing of itself.
// Values: the fold of a value table (pulse_tfe_mc_table_fold_after) -- the key goes to its canonical key, the slots stay where they are.
template <int NB, bool Values>
__global__ __launch_bounds__(kBlock) void tfe_mc_merge_kernel(const PulseTfeMCMerge o) {
    __shared__ unsigned long long wg[2];
    if (threadIdx.x < 2) wg[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long n_live = 0ull, n_dropped = 0ull;
    if (i < o.src_entries) {
        const Entry& e = static_cast<const Entry*>(o.src)[i];
        uint64_t key = e.key;
        if (key) {
            n_live = 1ull;
            long long cnt[4], sum[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { cnt[a] = e.cnt[a]; sum[a] = e.sum[a]; }
            int j = 0;
            if constexpr (NB > 0) key = canon_of_key<NB>(key, j);
            Entry* table = static_cast<Entry*>(o.dst);
            const long long s = find_or_insert<kMaxProbe>(table, 0, o.dst_capacity, key);
            if (s >= 0) {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (cnt[a] | sum[a]) {
                        const int at = NB > 0 && !Values ? map_action(kActionMap, j, a) : a;      // (an address, not a register index)
                        atomicAdd(reinterpret_cast<unsigned long long*>(&table[s].sum[at]), (unsigned long long)sum[a]);
                        atomicAdd(reinterpret_cast<unsigned long long*>(&table[s].cnt[at]), (unsigned long long)cnt[a]);
                    }
            } else {
                n_dropped = 1ull;
            }
        }
    }
    add_stats(wg, o.stats, 0, n_live, 2, n_dropped);                                   // (ends behind a barrier: wg is final)
    if (threadIdx.x == 2 && wg[0] != wg[1]) atomicAdd(reinterpret_cast<unsigned long long*>(o.stats) + 1, wg[0] - wg[1]);   // placed
}

// The largest frac_bits <= 30 with G_max * 2^frac_bits * 2^32 < 2^62, G_max = r_max * min(max_steps, 1 / (1 - gamma)); -1 = none.
int max_frac_bits(double gamma, int max_steps) {
    const double horizon = 1.0 / (1.0 - gamma);                                        // (gamma = 1: inf)
    const double g_max = (double)PULSE_TFE_MC_R_MAX * (horizon < (double)max_steps ? horizon : (double)max_steps);
    for (int f = 30; f >= 0; --f)
        if (std::ldexp(g_max, f) < 1073741824.0) return f;                             // 2^30
    return -1;
}

// The checks every entry point shares: the table and the shape of the batch ...
template <class O>
int check_table(const O* o, const char* name) {
    if (!o) return fail_named(name, "options are null");
    if (!o->entries) return fail_named(name, "entries is null");
    if ((uintptr_t)o->entries & (PULSE_TFE_MC_ENTRY_BYTES - 1)) return fail_named(name, "entries must be 128-byte aligned");
    if (o->capacity == 0 || (o->capacity & (o->capacity - 1))) return fail_named(name, "capacity must be a power of two");
    if (o->n < 2 || o->n > 4) return fail_named(name, "board side must be 2..4 (64-bit state key)");
    if (o->n_games < 1) return fail_named(name, "n_games must be positive");
    if (o->max_steps < 1 || o->max_steps > 65535) return fail_named(name, "max_steps must be in 1..65535");
    return 0;
}
// ... and those of the roll-outs and the learner: their structs begin with the same fields.
template <class O>
int check_common(const O* o, const char* name) {
    if (int rc = check_table(o, name)) return rc;
    if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (!(o->epsilon >= 0.0 && o->epsilon <= 1.0)) return fail_named(name, "epsilon must be in [0, 1]");
    if (o->frac_bits < 0 || o->frac_bits > max_frac_bits(o->gamma, o->max_steps))
        return fail_named(name, "frac_bits outside 0 .. the largest value with 17 * min(max_steps, 1 / (1 - gamma)) * 2^frac_bits < 2^30");
    if (!o->keys) return fail_named(name, "keys is null");
    if (!o->steps) return fail_named(name, "steps is null");
    if (!o->lengths) return fail_named(name, "lengths is null");
    if (!o->stats) return fail_named(name, "stats is null");
    if (((uintptr_t)o->keys & 7u) || ((uintptr_t)o->stats & 7u)) return fail_named(name, "keys / stats must be 8-byte aligned");
    if ((uintptr_t)o->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    return 0;
}

// The launches of the game loop.  `o` is the caller's struct, or pulse_tfe_mc_evaluate's outputs in its shape.
template <bool Canon, bool Record, bool After>
void launch_games(const PulseTfeMCRollout& o, int64_t* hist, void* stream) {
    const uint32_t eps_q24 = (uint32_t)std::floor(o.epsilon * 16777216.0);             // once, here: the kernel compares integers
    const double inv_scale = std::ldexp(1.0, -o.frac_bits);
    const dim3 grid((unsigned)((o.n_games + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    switch (o.n) {
    case 2: hipLaunchKernelGGL((tfe_mc_rollout_kernel<2, Canon, Record, After>), grid, block, 0, st, o, eps_q24, inv_scale, hist); break;
    case 3: hipLaunchKernelGGL((tfe_mc_rollout_kernel<3, Canon, Record, After>), grid, block, 0, st, o, eps_q24, inv_scale, hist); break;
    default: hipLaunchKernelGGL((tfe_mc_rollout_kernel<4, Canon, Record, After>), grid, block, 0, st, o, eps_q24, inv_scale, hist);
    }
}

template <bool Record, bool After>
void launch_games(const PulseTfeMCRollout& o, int64_t* hist, void* stream, bool canon) {
    if (canon) launch_games<true, Record, After>(o, hist, stream); else launch_games<false, Record, After>(o, hist, stream);
}

int rollout(const PulseTfeMCRollout* o, void* stream, bool canon, bool after, const char* name) {
    if (int rc = check_common(o, name)) return rc;
    if (!o->total_score) return fail_named(name, "total_score is null");
    if (!o->episode_reward) return fail_named(name, "episode_reward is null");
    if ((uintptr_t)o->total_score & 7u) return fail_named(name, "total_score must be 8-byte aligned");
    if ((uintptr_t)o->episode_reward & 3u) return fail_named(name, "episode_reward must be 4-byte aligned");
    if (after) launch_games<true, true>(*o, nullptr, stream, canon); else launch_games<true, false>(*o, nullptr, stream, canon);
    return 0;
}

// pulse_tfe_mc_evaluate and pulse_tfe_mc_evaluate_after (gamma: the latter's, which its policy needs and the struct does not hold)
int evaluate(const PulseTfeMCEval* e, double gamma, void* stream, bool after, const char* name) {
    if (int rc = check_table(e, name)) return rc;
    if (!(e->epsilon >= 0.0 && e->epsilon <= 1.0)) return fail_named(name, "epsilon must be in [0, 1]");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail_named(name, "gamma must be in [0, 1]");
    if (e->frac_bits < 0 || e->frac_bits > 30) return fail_named(name, "frac_bits must be in 0..30");
    if (e->canonical != 0 && e->canonical != 1) return fail_named(name, "canonical must be 0 or 1");
    if (!e->summary) return fail_named(name, "summary is null");
    if (!e->max_tile_hist) return fail_named(name, "max_tile_hist is null");
    if (((uintptr_t)e->summary & 7u) || ((uintptr_t)e->max_tile_hist & 7u)) return fail_named(name, "summary / max_tile_hist must be 8-byte aligned");
    if ((uintptr_t)e->total_score & 7u) return fail_named(name, "total_score must be 8-byte aligned");
    if ((uintptr_t)e->lengths & 3u) return fail_named(name, "lengths must be 4-byte aligned");
    if (e->reserved0 != 0 || e->reserved1 != 0) return fail_named(name, "reserved0 / reserved1 must be 0 (zero-initialise the struct)");
    PulseTfeMCRollout o{};                                                             // keys / steps / episode_reward stay null: not Record
    o.entries = const_cast<void*>(e->entries); o.capacity = e->capacity;
    o.n_games = e->n_games; o.n = e->n; o.max_steps = e->max_steps; o.frac_bits = e->frac_bits;
    o.gamma = gamma; o.epsilon = e->epsilon;
    o.env_seed = e->env_seed; o.agent_seed = e->agent_seed; o.tie_seed = e->tie_seed; o.board_id0 = e->board_id0; o.round = e->round;
    o.lengths = e->lengths; o.total_score = e->total_score; o.stats = e->summary;
    if (after) launch_games<false, true>(o, e->max_tile_hist, stream, e->canonical != 0);
    else launch_games<false, false>(o, e->max_tile_hist, stream, e->canonical != 0);
    return 0;
}

// pulse_tfe_mc_table_merge, and pulse_tfe_mc_table_fold_after (values): the fold of a value table
int merge(const PulseTfeMCMerge* o, void* stream, bool values, const char* name) {
    constexpr uint64_t kLine = PULSE_TFE_MC_ENTRY_BYTES;
    if (!o) return fail_named(name, "options are null");
    if (!o->src) return fail_named(name, "src is null");
    if (!o->dst) return fail_named(name, "dst is null");
    if ((uintptr_t)o->src & (kLine - 1)) return fail_named(name, "src must be 128-byte aligned");
    if ((uintptr_t)o->dst & (kLine - 1)) return fail_named(name, "dst must be 128-byte aligned");
    if (o->src_entries < 1) return fail_named(name, "src_entries must be positive");
    if (o->src_entries > 0xFFFFFFFFull) return fail_named(name, "src_entries must be below 2^32 (one lane per slot, one launch)");
    if (o->dst_capacity == 0 || (o->dst_capacity & (o->dst_capacity - 1)) || o->dst_capacity > (UINT64_MAX >> 8))
        return fail_named(name, "dst_capacity must be a power of two");
    {
        const uint64_t s0 = (uint64_t)(uintptr_t)o->src, s1 = s0 + o->src_entries * kLine;
        const uint64_t d0 = (uint64_t)(uintptr_t)o->dst, d1 = d0 + o->dst_capacity * kLine;
        if (s0 < d1 && d0 < s1) return fail_named(name, "src and dst overlap");
    }
    if (o->canonical != 0 && o->canonical != 1) return fail_named(name, "canonical must be 0 or 1");
    if (values && o->canonical != 1) return fail_named(name, "canonical must be 1 (the plain merge of a value table is pulse_tfe_mc_table_merge)");
    if (o->n < 2 || o->n > 4) return fail_named(name, "board side n must be 2..4 (64-bit state key)");
    if (!o->stats) return fail_named(name, "stats is null");
    if ((uintptr_t)o->stats & 7u) return fail_named(name, "stats must be 8-byte aligned");
    if (o->reserved0 != 0) return fail_named(name, "reserved0 must be 0 (zero-initialise the struct)");
    const dim3 grid((unsigned)((o->src_entries + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    switch ((o->canonical ? o->n : 0) + (values ? 8 : 0)) {
    case 0: hipLaunchKernelGGL((tfe_mc_merge_kernel<0, false>), grid, block, 0, st, *o); break;
    case 2: hipLaunchKernelGGL((tfe_mc_merge_kernel<2, false>), grid, block, 0, st, *o); break;
    case 3: hipLaunchKernelGGL((tfe_mc_merge_kernel<3, false>), grid, block, 0, st, *o); break;
    case 4: hipLaunchKernelGGL((tfe_mc_merge_kernel<4, false>), grid, block, 0, st, *o); break;
    case 10: hipLaunchKernelGGL((tfe_mc_merge_kernel<2, true>), grid, block, 0, st, *o); break;
    case 11: hipLaunchKernelGGL((tfe_mc_merge_kernel<3, true>), grid, block, 0, st, *o); break;
    default: hipLaunchKernelGGL((tfe_mc_merge_kernel<4, true>), grid, block, 0, st, *o);
    }
    return 0;
}

}  // namespace

extern "C" int pulse_tfe_mc_rollout(const PulseTfeMCRollout* o, void* stream) {
    if (int rc = rollout(o, stream, false, false, "pulse_tfe_mc_rollout")) return rc;
    return finish_launch("pulse_tfe_mc_rollout launch");
}

extern "C" int pulse_tfe_mc_rollout_canon(const PulseTfeMCRollout* o, void* stream) {
    if (int rc = rollout(o, stream, true, false, "pulse_tfe_mc_rollout_canon")) return rc;
    return finish_launch("pulse_tfe_mc_rollout_canon launch");
}

extern "C" int pulse_tfe_mc_evaluate(const PulseTfeMCEval* e, void* stream) {
    if (int rc = evaluate(e, 0.0, stream, false, "pulse_tfe_mc_evaluate")) return rc;
    return finish_launch("pulse_tfe_mc_evaluate launch");
}

extern "C" int pulse_tfe_mc_table_merge(const PulseTfeMCMerge* o, void* stream) {
    if (int rc = merge(o, stream, false, "pulse_tfe_mc_table_merge")) return rc;
    return finish_launch("pulse_tfe_mc_table_merge launch");
}

extern "C" int pulse_tfe_mc_learn(const PulseTfeMCLearn* o, void* stream) {
    if (int rc = check_common(o, "pulse_tfe_mc_learn")) return rc;
    hipLaunchKernelGGL(tfe_mc_learn_kernel<false>, dim3((unsigned)((o->n_games + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, *o);
    return finish_launch("pulse_tfe_mc_learn launch");
}

// ---- the afterstate mode: the same structs and checks, V(board after the move) in cnt[0] / sum[0]
extern "C" int pulse_tfe_mc_rollout_after(const PulseTfeMCRollout* o, void* stream) {
    if (int rc = rollout(o, stream, false, true, "pulse_tfe_mc_rollout_after")) return rc;
    return finish_launch("pulse_tfe_mc_rollout_after launch");
}

extern "C" int pulse_tfe_mc_rollout_after_canon(const PulseTfeMCRollout* o, void* stream) {
    if (int rc = rollout(o, stream, true, true, "pulse_tfe_mc_rollout_after_canon")) return rc;
    return finish_launch("pulse_tfe_mc_rollout_after_canon launch");
}

extern "C" int pulse_tfe_mc_learn_after(const PulseTfeMCLearn* o, void* stream) {
    if (int rc = check_common(o, "pulse_tfe_mc_learn_after")) return rc;
    hipLaunchKernelGGL(tfe_mc_learn_kernel<true>, dim3((unsigned)((o->n_games + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, *o);
    return finish_launch("pulse_tfe_mc_learn_after launch");
}

extern "C" int pulse_tfe_mc_evaluate_after(const PulseTfeMCEval* e, double gamma, void* stream) {
    if (int rc = evaluate(e, gamma, stream, true, "pulse_tfe_mc_evaluate_after")) return rc;
    return finish_launch("pulse_tfe_mc_evaluate_after launch");
}

extern "C" int pulse_tfe_mc_table_fold_after(const PulseTfeMCMerge* o, void* stream) {
    if (int rc = merge(o, stream, true, "pulse_tfe_mc_table_fold_after")) return rc;
    return finish_launch("pulse_tfe_mc_table_fold_after launch");
}
