// qnet_train_device.h -- what the training kernels of qnet.hip (qnet_train_kernel: four wavefronts per tile,
// qnet_train8_kernel: eight) and qnet_act_rows_kernel share, each phase once: the row lists, the per-candidate bookkeeping,
// the TD head, the stability totals, the gradient slice and its products, the launch's prologue.  NT is the
// workgroup's thread count (256 / 512).  Not part of the ABI.
#pragma once
#include "qnet_device.h"

namespace pulse_qnet {

constexpr int kMeetUsed = 400;                 // meet[400]: how many of the training launch's workgroups wrote a slice (workgroups 0 .. that - 1)
struct TrainArgs {
    FlatNet net, tgt;
    float* partials;                          // [gridDim.x][kSlicePitch]: gradient blocks, biases, then the 8 statistics (kSliceStats)
    float* scal;                              // scal[0] = squared gradient norm of the reduce launch: cleared here for it
    int n_params;
    const float* states; long long stride;
    const int64_t* actions; const float* rewards;
    const float* next_states; long long next_stride;
    const uint8_t* dones;
    const int32_t* sel_rows; const int32_t* sel_counts;   // the row lists: sel_rows[(w << win_shift) + i], i < sel_counts[w]
    int win_shift;                                        // 8: the select launch's windows; 7: the act launch's
    const uint8_t* row_mask; uint8_t* terminated; int book; // book: the per-candidate bookkeeping is done here (lists from act)
    unsigned* meet;
    int n_rows;
    uint64_t seed, step, table_id0;
    float gamma, drop_p;
};

// ---- row lists: the listed rows of the whole batch, in window order, are positions [0, T) --------------------------------
// Every workgroup computes the same exclusive sums of the windows' counts: thread t owns windows [t per, (t + 1) per) and
// leaves the first position of its range in chunk[t] (chunk[NT ..]: the wavefronts' totals).  Returns T.  All NT threads.
template <int NT>
__device__ __forceinline__ int list_positions(int* __restrict__ chunk, const int32_t* __restrict__ counts, int n_windows, int per, int wv, int lane) {
    int mine = 0;
    for (int j = 0; j < per; ++j) { const int w = threadIdx.x * per + j; mine += w < n_windows ? counts[w] : 0; }
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off); incl += lane >= off ? o : 0; }
    int* wtot = chunk + NT;
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int base = 0, T = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) { const int n = wtot[i]; base += i < wv ? n : 0; T += n; }
    chunk[threadIdx.x] = base + incl - mine;
    __syncthreads();
    return T;
}
// the row at position p < T: its thread by bisection of the first positions (the last t with chunk[t] <= p has a non-empty
// range holding p), then along that thread's windows (a dependent load each)
template <int NT>
__device__ __forceinline__ int list_row(const int* __restrict__ chunk, const int32_t* __restrict__ counts, const int32_t* __restrict__ rows,
                                        int per, int shift, int p) {
    int t = 0;
#pragma unroll
    for (int s = NT / 2; s >= 1; s >>= 1) t += (chunk[t + s] <= p) ? s : 0;
    int w = t * per, acc = chunk[t], cnt = counts[w];
    while (p >= acc + cnt) { acc += cnt; ++w; cnt = counts[w]; }
    return rows[((size_t)w << shift) + (p - acc)];
}
// column c of tile ti of an even split of [0, T) into n_tiles pieces of <= 32 rows, or -1
template <int NT>
__device__ __forceinline__ int tile_row(const int* __restrict__ chunk, const TrainArgs& a, int per, int T, int n_tiles, int ti, int c) {
    const int lo = (int)((long long)ti * T / n_tiles), hi = (int)((long long)(ti + 1) * T / n_tiles);
    return lo + c < hi ? list_row<NT>(chunk, a.sel_counts, a.sel_rows, per, a.win_shift, lo + c) : -1;
}

// What the select launch does per candidate row, when the act launch made the lists (a.book): `terminated |= dones`
// (trainGPU.py:86) and the reward sum over the row_mask rows, before the status filter (trainGPU.py:96) -- this wavefront's
// part of it, lane-replicated.
template <int NT>
__device__ __forceinline__ float book_candidates(const TrainArgs& a) {
    float reward_sum = 0.0f;
    for (int win = blockIdx.x; win * NT < a.n_rows; win += gridDim.x) {
        const int row = win * NT + threadIdx.x;
        const bool cand = row < a.n_rows && (a.row_mask == nullptr || a.row_mask[row] != 0);
        float rew = cand ? a.rewards[row] : 0.0f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rew += __shfl_xor(rew, off);
        reward_sum += rew;
        if (a.terminated && row < a.n_rows && a.dones[row]) a.terminated[row] = 1;
    }
    return reward_sum;
}

// ---- stability totals (PulseQNetTrain.stability): sum |td|, sum Q(s, a), min / max Q(s, a) over rows ------------------------
struct StabTotals {
    float td = 0.0f, q = 0.0f, qmin = INFINITY, qmax = -INFINITY;
    __device__ __forceinline__ void add(float td_row, float qa) { td += fabsf(td_row); q += qa; qmin = fminf(qmin, qa); qmax = fmaxf(qmax, qa); }
    __device__ __forceinline__ void add(const StabTotals& o) { td += o.td; q += o.q; qmin = fminf(qmin, o.qmin); qmax = fmaxf(qmax, o.qmax); }
    __device__ __forceinline__ void reduce() {                   // over the wavefront; lane-replicated afterwards
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            td += __shfl_xor(td, off); q += __shfl_xor(q, off);
            qmin = fminf(qmin, __shfl_xor(qmin, off)); qmax = fmaxf(qmax, __shfl_xor(qmax, off));
        }
    }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(td, q, qmin, qmax); }
    __device__ static __forceinline__ StabTotals load(const float* p) {
        const float4 s4 = *reinterpret_cast<const float4*>(p);
        StabTotals s; s.td = s4.x; s.q = s4.y; s.qmin = s4.z; s.qmax = s4.w;
        return s;
    }
};

// ---- TD head (Player.py:270-279), on the wavefront that holds the output tile ---------------------------------------------
// max_a' Q_target(s', a') of this lane's column over the valid rows of the target network's output tile
__device__ __forceinline__ float max_q_target(const f32x16& qn, int A, int h) {
    float best = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) if (rho(r) + 4 * h < A) best = fmaxf(best, qn[r]);
    return fmaxf(best, __shfl_xor(best, 32));
}
// target = r + gamma max Q_target (1 - done) (:275-277); delta_5 = 2 (Q(s, a) - target) on the action's row -> Da; the loss terms
template <bool STAB>
__device__ __forceinline__ void td_head(const f32x16& qv, float best, float gamma, float row_reward, float row_done, int act, bool live,
                                        float* __restrict__ Da, int c, int h, float& rows_sum, float& sq_sum, StabTotals& st) {
    const float target = row_reward + gamma * best * (1.0f - row_done);
    float qa = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) qa += (rho(r) + 4 * h == act) ? qv[r] : 0.0f;
    qa += __shfl_xor(qa, 32);
    const float td = live ? qa - target : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) Da[(rho(r) + 4 * h) * kLd + c] = (rho(r) + 4 * h == act) ? 2.0f * td : 0.0f;
    float sq = (h == 0) ? td * td : 0.0f, cnt = (h == 0 && live) ? 1.0f : 0.0f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { sq += __shfl_xor(sq, off); cnt += __shfl_xor(cnt, off); }
    rows_sum += cnt; sq_sum += sq;
    if (STAB && h == 0 && live) st.add(td, qa);
}

// ---- the gradient slice ---------------------------------------------------------------------------------------------------
// A workgroup's gradient slice is private scratch, so its layout is the accumulators' own: 35 blocks of 32x32 (layer 1:
// 4x2, layer 2: 4x4, layer 3: 2x4, layer 4: 1x2, layer 5: 1x1 -- padded rows / columns included; NetShape::blk), each
// stored as [lane][16 registers], then the five bias vectors (NetShape::bias), then 8 statistics.  A wavefront then writes
// a block with four 16-byte stores per lane instead of sixteen 4-byte ones (global stores are issue-bound: the dword form
// made the weight-gradient blocks 4x slower than their MFMAs); qnet_grad_reduce_kernel maps parameters to this layout.
// Statistics: {rows, sum td^2, reward, used}, then -- written by the STAB instances only (PulseQNetTrain.stability) --
// StabTotals over the workgroup's rows (+inf / -inf for a workgroup without rows).
constexpr NetShape kSlice = net_shape(64, 32);                  // (blocks and bias words: the same for every state_dim / n_actions)
constexpr int kSliceBlk1 = kSlice.blk[0], kSliceBlk2 = kSlice.blk[1], kSliceBlk3 = kSlice.blk[2], kSliceBlk4 = kSlice.blk[3],
              kSliceBlk5 = kSlice.blk[4], kSliceBlocks = kSlice.blk[5];
constexpr int kSliceBias = kSliceBlocks * 1024;
constexpr int kSliceStats = kSliceBias + kSlice.bias[5], kSlicePitch = kSliceStats + 8;
static_assert(kSliceBlocks == 35 && kSlice.bias[5] == 384, "slice layout");

// block `blk` (= dW rows [32 ot, +32) x columns [32 it, +32) of its layer) += delta . a^T for this tile (`first`: nothing
// accumulated yet); delta in D, a_{l-1} in Ap; bsum: this tile's db rows of tile ot
__device__ __forceinline__ void dw_accum(const float* __restrict__ D, const float* __restrict__ Ap, float* __restrict__ slice, int blk,
                                         int ot, int it, int c, int h, bool first, float* bsum) {
    // registers 4q .. 4q+3 of all 64 lanes form one contiguous KB of the slice: a store instruction writes whole lines.  The
    // block's old values are asked for FIRST (not after the MFMAs, where every call waited out their round trip: with ~20 tiles
    // per workgroup at 2,000,000 tables the slices live in the Infinity Cache, not in L2)
    float4* dst = reinterpret_cast<float4*>(slice + (size_t)blk * 1024) + (c + 32 * h);
    float4 old[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { old[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); if (!first) old[q] = dst[64 * q]; }
    float ad[16], ap[16]; float bs = 0.0f;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) { ad[s2] = D[(32 * ot + c) * kLd + 2 * s2 + h]; ap[s2] = Ap[(32 * it + c) * kLd + 2 * s2 + h]; }
    __builtin_amdgcn_sched_barrier(0);                            // (all 32 LDS reads ahead of the MFMAs, as in mfma_w)
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) bs += ad[s2];
    if (bsum) *bsum += bs + __shfl_xor(bs, 32);
    f32x16 acc = zero16();
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ad[s2], ap[s2], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        dst[64 * q] = make_float4(acc[4 * q] + old[q].x, acc[4 * q + 1] + old[q].y, acc[4 * q + 2] + old[q].z, acc[4 * q + 3] + old[q].w);
}

// flat parameter index (order w1,b1,...,w5,b5) of slice element j, or -1 for a padding element
__device__ __forceinline__ int slice_param(int j, int K1, int A) {
    constexpr NetShape s = net_shape(64, 32);                    // (blocks and bias words: the same for every state_dim / n_actions)
    int n_out[5], n_in[5], w[5], b[5], acc = 0;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        n_out[l] = l == 4 ? A : s.n_out[l]; n_in[l] = l == 0 ? K1 : s.n_in[l];
        w[l] = acc; acc += n_out[l] * n_in[l]; b[l] = acc; acc += n_out[l];
    }
    if (j >= kSliceBias) {
        const int u = j - kSliceBias;
#pragma unroll
        for (int l = 0; l < 5; ++l)
            if (u >= s.bias[l] && u < s.bias[l + 1]) return (u - s.bias[l]) < n_out[l] ? b[l] + (u - s.bias[l]) : -1;
        return -1;
    }
    const int blk = j >> 10, lane = (j >> 2) & 63, r = 4 * ((j >> 8) & 3) + (j & 3), c = lane & 31, h = lane >> 5;   // [block][q][lane][4]
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (blk >= s.blk[l] && blk < s.blk[l + 1]) {
            const int bl = blk - s.blk[l], ot = bl / s.col_tiles[l], it = bl - ot * s.col_tiles[l];
            const int o = 32 * ot + rho(r) + 4 * h, in = 32 * it + c;
            return (o < n_out[l] && in < n_in[l]) ? w[l] + o * n_in[l] + in : -1;
        }
    }
    return -1;
}

// tile `it` of delta_{l-1} = (W^T . delta_l) * g_{l-1} -> Dn[32 it ..]; W is n_out x n_in, delta_l = units [0, KU) of D.
// back_load: the KU / 2 weights (one per MFMA, down a column of W: coalesced), issued a phase ahead by the caller.
template <int KU>
__device__ __forceinline__ void back_load(float (&wa)[KU / 2], const float* __restrict__ w, int n_out, int n_in, int it, int c, int h) {
#pragma unroll
    for (int i = 0; i < KU / 2; ++i) {
        const int k = 2 * i + h;
        wa[i] = k < n_out ? w[(size_t)k * n_in + 32 * it + c] : 0.0f;
    }
}
template <int KU>
__device__ __forceinline__ void back_mul(const float (&wa)[KU / 2], int it, const float* __restrict__ D, const float* __restrict__ G,
                                         float* __restrict__ Dn, int c, int h) {
    float dv[KU / 2], gv[16];
#pragma unroll
    for (int i = 0; i < KU / 2; ++i) dv[i] = D[(2 * i + h) * kLd + c];
#pragma unroll
    for (int r = 0; r < 16; ++r) gv[r] = G[(32 * it + rho(r) + 4 * h) * kLd + c];
    __builtin_amdgcn_sched_barrier(0);                            // (LDS reads ahead of the MFMAs)
    f32x16 acc = zero16();
#pragma unroll
    for (int i = 0; i < KU / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[i], dv[i], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) Dn[(32 * it + rho(r) + 4 * h) * kLd + c] = acc[r] * gv[r];
}

// ---- prologue of a training launch -----------------------------------------------------------------------------------------
// The fused reduce launch's arrival counters are cleared here for it; so is scal[0], which every workgroup of the previous
// step's AdamW launch reads and this step's reduce launch accumulates: this kernel sits between the two on the stream.
__device__ __forceinline__ void train_prologue(const TrainArgs& a) {
    if (blockIdx.x == 0 && threadIdx.x < 8) a.meet[threadIdx.x] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.scal[0] = 0.0f;
    QSTAMP(0);
}

}  // namespace pulse_qnet
