// TransMIL (reference: model/dim1/TransMIL.py + the nystrom_attention package its TransLayer builds), MI355X path.
//
// The Nystrom core of one bag is a chain of per-head products with the three softmax maps materialised
// (A1 [n_pad, 256], A2 [256, 256], A3 [256, n_pad] per head), so every stage here is either
//  - a batched fp32-MFMA product over general strides (k_tm_bgemm): the per-head operands are read straight out of the
//    merged [n_pad, 3 x 512] q|k|v rows of to_qkv, and the results are written straight into merged-head rows, with the
//    `c I - P` epilogue of the Newton-Schulz pseudo-inverse and split-K (atomic accumulation) for the long-K products;
//  - a row-wise pass (softmax fwd/bwd, landmark means, the 33-tap residual conv on v, the pseudo-inverse's scale), or
//  - the PPEG depthwise 7 x 7 (the 7 / 5 / 3 kernels and the identity folded into one) and the row gather of the
//    sequence assembly ([cls | tokens | repeats], front zero pad).
// Heads fixed at 8 x 64 (TransLayer: dim 512, dim_head 64), 256 landmarks, conv kernel 33.
//
// Every sum that crosses workgroups - the split-K products, the gather's backward, <dZ0, Z0>, the res_conv and PPEG weight
// gradients - has two forms: float atomics (the default), and the mil_tm_*_fixed entries at the end of the file, whose
// kernels are the same loops templated on FIXED: partial sums go to a caller's workspace with plain stores and a second
// launch (k_tm_fold, k_tm_bgemm_fold) adds them in ascending chunk order, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "tm_bgemm.h"
#include "tm_packed.h"
#include "tm_ppeg_packed.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int TM_H = 8, TM_DH = 64, TM_D = 512, TM_QKV = 3 * TM_D, TM_M = 256, TM_CONV = 33;
constexpr int BG_BK = 16, BG_LD = 64 + 4, BG_FOLD = BG_FOLD_K / BG_BK;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// C[b] = alpha A[b] B[b] + beta D[b] + diag I (D = C when null; D[b] laid out like C[b]), element (i, k) of A[b] at
// A + b sAb + i sAi + k sAk (likewise B, C).
// 64 x 64 tile, 2 x 2 waves of one 32 x 32 MFMA accumulator each, K staged 16 at a time through LDS (k-major images,
// the register copy of the next slice loaded while the current one is multiplied).  blockIdx.z = batch * splits + split;
// splits > 1 adds the partial products atomically (the caller has C initialised; beta must be 1, D null).
// FIXED (splits > 1 only): split p stores alpha x its partial tile with plain stores into ws[p][batch][M][N] (C then holds the
// workspace, D, beta and diag are unused; an empty split stores zeros) and k_tm_bgemm_fold adds the splits in ascending order.
template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_bgemm(const float* __restrict__ A, long sAb, long sAi, long sAk,
                                                  const float* __restrict__ B, long sBb, long sBk, long sBj, float* C,
                                                  long sCb, long sCi, long sCj, const float* D, int M, int N, int K,
                                                  float alpha, float beta, float diag, int splits) {
    __shared__ float as[BG_BK][BG_LD];
    __shared__ float bs[BG_BK][BG_LD];
    const int bz = blockIdx.z / splits, split = blockIdx.z % splits;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    A += (long)bz * sAb;
    B += (long)bz * sBb;
    C += (long)bz * sCb;
    if (D != nullptr) D += (long)bz * sCb;
    const int kslices = (K + BG_BK - 1) / BG_BK;
    const int per = (kslices + splits - 1) / splits;
    const int s0 = split * per, s1 = min(kslices, s0 + per);
    const bool a_krow = sAk == 1, b_jrow = sBj == 1;

    float ra[4], rb[4];
    auto load = [&](int ks) {
        const int k0 = ks * BG_BK;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int e = tid + 256 * p;
            const int ai = a_krow ? e >> 4 : e & 63, ak = a_krow ? e & 15 : e >> 6;
            const int gi = i0 + ai, gk = k0 + ak;
            ra[p] = (gi < M && gk < K) ? A[gi * sAi + gk * sAk] : 0.f;
            const int bj = b_jrow ? e & 63 : e >> 4, bk = b_jrow ? e >> 6 : e & 15;
            const int gj = j0 + bj, gk2 = k0 + bk;
            rb[p] = (gj < N && gk2 < K) ? B[gk2 * sBk + gj * sBj] : 0.f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int e = tid + 256 * p;
            const int ai = a_krow ? e >> 4 : e & 63, ak = a_krow ? e & 15 : e >> 6;
            as[ak][ai] = ra[p];
            const int bj = b_jrow ? e & 63 : e >> 4, bk = b_jrow ? e >> 6 : e & 15;
            bs[bk][bj] = rb[p];
        }
    };

    // two levels: the MFMA chain runs over BG_FOLD slices (512 of K), then folds into `tot` - one running fp32 sum over a
    // K of 7936 loses 19 x what the float32 product on the CPU loses (tests/test_gpu_transmil_stages.py, docs/lab_notes.md)
    f32x16 acc, tot;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = tot[i] = 0.f;
    if (s0 < s1) load(s0);
    for (int ks = s0; ks < s1; ++ks) {
        store();
        __syncthreads();
        if (ks + 1 < s1) load(ks + 1);
#pragma unroll
        for (int kk = 0; kk < BG_BK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * kk + h][32 * wi + r], bs[2 * kk + h][32 * wj + r], acc, 0, 0, 0);
        if (((ks - s0) & (BG_FOLD - 1)) == BG_FOLD - 1) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { tot[i] += acc[i]; acc[i] = 0.f; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] += tot[i];

    tm_bgemm_store<FIXED>(acc, C, sCi, sCj, D, M, N, i0 + 32 * wi, j0 + 32 * wj + r, h, alpha, beta, diag, splits, split);
}

// out[e] = sum_c ws[c * stride + e] for c = 0, 1, .. chunks - 1 in that order, e < n: the second launch of every fixed-order
// sum whose output is contiguous (the partials come from the launch in front, plain stores, no counters)
__global__ __launch_bounds__(256) void k_tm_fold(const float* __restrict__ ws, long stride, int chunks, int n, float* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = ws[e];
    for (int c = 1; c < chunks; ++c) v += ws[c * stride + e];
    out[e] = v;
}

inline void tm_fold(const float* ws, long stride, int chunks, int n, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_tm_fold, dim3((n + 255) / 256), dim3(256), 0, stream, ws, stride, chunks, n, out);
}

// in place: x[row] = softmax(x[row]); one wave per row
__global__ __launch_bounds__(256) void k_tm_softmax(float* x, long rows, int cols) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* p = x + row * cols;
    float m = -INFINITY;
    for (int j = lane; j < cols; j += 64) m = fmaxf(m, p[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < cols; j += 64) s += __expf(p[j] - m);
    s = wave_sum(s);
    const float inv = 1.f / s;
    for (int j = lane; j < cols; j += 64) p[j] = __expf(p[j] - m) * inv;
}

// in place: dp[row] = p (dp - <p, dp>)
__global__ __launch_bounds__(256) void k_tm_softmax_bwd(const float* p, float* dp, long rows, int cols) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* pr = p + row * cols;
    float* dr = dp + row * cols;
    float s = 0.f;
    for (int j = lane; j < cols; j += 64) s += pr[j] * dr[j];
    s = wave_sum(s);
    for (int j = lane; j < cols; j += 64) dr[j] = pr[j] * (dr[j] - s);
}

// dst[r] = idx[r] >= 0 ? src[idx[r]] : idx[r] == -2 && extra ? extra : 0 (a null `extra` reads as a row of zeros)
__global__ __launch_bounds__(256) void k_tm_gather(const float* __restrict__ src, const float* __restrict__ extra,
                                                   const int32_t* __restrict__ idx, int E, float* __restrict__ dst) {
    const int r = blockIdx.x, id = idx[r];
    const float* s = id >= 0 ? src + (long)id * E : (id == -2 ? extra : nullptr);
    for (int c = threadIdx.x; c < E; c += 256) dst[(long)r * E + c] = s != nullptr ? s[c] : 0.f;
}

__global__ __launch_bounds__(256) void k_tm_gather_bwd(const float* __restrict__ ddst, const int32_t* __restrict__ idx, int E,
                                                       float* dsrc, float* dextra) {
    const int r = blockIdx.x, id = idx[r];
    if (id == -1 || (id == -2 && dextra == nullptr)) return;
    float* d = id >= 0 ? dsrc + (long)id * E : dextra;
    for (int c = threadIdx.x; c < E; c += 256) atomicAdd(d + c, ddst[(long)r * E + c]);
}

// The same sums in an order the index alone fixes.  meta [src_rows][3] int32 (zeroed by k_tm_gather_meta_zero): how many rows
// of idx name source row i, and the first and the last of them as rows - first and last + 1 under atomicMax - integer
// atomics, whose results do not depend on the order they land in.
__global__ __launch_bounds__(256) void k_tm_gather_meta_zero(int32_t* __restrict__ meta, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) meta[e] = 0;
}

__global__ __launch_bounds__(256) void k_tm_gather_meta(const int32_t* __restrict__ idx, int rows, int src_rows, int32_t* meta) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int id = idx[r];
    if (id < 0 || id >= src_rows) return;
    atomicAdd(meta + 3 * id, 1);
    atomicMax(meta + 3 * id + 1, rows - r);
    atomicMax(meta + 3 * id + 2, r + 1);
}

// out[c] = sum of ddst[r][c] over the rows r in [r_lo, r_hi] with idx[r] == target, r ascending: the whole workgroup walks idx in
// chunks of 256, each wave ballots its 64 entries, and every thread adds the rows of the set bits, lowest first, to its column
__device__ __forceinline__ void tm_gather_scan_sum(const float* __restrict__ ddst, const int32_t* __restrict__ idx, int r_lo,
                                                   int r_hi, int target, int E, float* __restrict__ out) {
    __shared__ unsigned long long hit[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int c0 = 0; c0 < E; c0 += 256) {
        const int c = c0 + tid;
        float acc = 0.f;
        for (int base = r_lo; base <= r_hi; base += 256) {
            const int r = base + tid;
            const unsigned long long b = __ballot(r <= r_hi && idx[r] == target);
            if (lane == 0) hit[wv] = b;
            __syncthreads();
            for (int w = 0; w < 4; ++w) {
                unsigned long long m = hit[w];
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (c < E) acc += ddst[(long)(base + 64 * w + j) * E + c];
                }
            }
            __syncthreads();
        }
        if (c < E) out[c] = acc;
    }
}

// workgroup i < src_rows writes dsrc[i]: zeros, a copy, ddst[first] + ddst[last], or (named more than twice) the ascending scan
// between its first and last row; workgroup src_rows (launched when dextra is not null) scans all of idx for the -2 rows
__global__ __launch_bounds__(256) void k_tm_gather_bwd_fixed(const float* __restrict__ ddst, const int32_t* __restrict__ idx, int rows,
                                                             int E, const int32_t* __restrict__ meta, int src_rows,
                                                             float* __restrict__ dsrc, float* __restrict__ dextra) {
    const int i = blockIdx.x;
    if (i == src_rows) {
        tm_gather_scan_sum(ddst, idx, 0, rows - 1, -2, E, dextra);
        return;
    }
    const int cnt = meta[3 * i], first = rows - meta[3 * i + 1], last = meta[3 * i + 2] - 1;
    float* d = dsrc + (long)i * E;
    if (cnt > 2) {
        tm_gather_scan_sum(ddst, idx, first, last, i, E, d);
        return;
    }
    for (int c = threadIdx.x; c < E; c += 256) {
        float v = 0.f;
        if (cnt >= 1) v = ddst[(long)first * E + c];
        if (cnt == 2) v += ddst[(long)last * E + c];
        d[c] = v;
    }
}

// Grid sides of up to TM_MAX_BAGS bags, by value: what a captured step of those sides is keyed by.  The lengths are read from
// the device, so one graph per tuple of sides serves every bag with (s - 1)^2 < N <= s^2.
constexpr int TM_MAX_BAGS = 16;
struct TmSides {
    int s[TM_MAX_BAGS];
};

// length of bag b as the index may use it: clamped into its side's bucket, so that no index leaves the capacity
__device__ __forceinline__ int tm_len(const int32_t* __restrict__ len_dev, const TmSides& sd, int b) {
    const int s = sd.s[b], lo = (s - 1) * (s - 1) + 1, hi = s * s;
    return min(max(len_dev[b], lo), hi);
}

// idx[r] of the sequence assembly, thread per entry: bag b owns 1 + s_b^2 entries, [-2 | off .. off + N - 1 | off .. off +
// add - 1] with off = the rows of the bags in front (bags are packed back to back by their true lengths).  Thread 0 also
// writes the true row count and raises `flag` when a length lies outside its bucket (sticky: never cleared here).
__global__ __launch_bounds__(256) void k_tm_seq_index(const int32_t* __restrict__ len_dev, int B, TmSides sd, int total,
                                                      int32_t* __restrict__ idx, int32_t* __restrict__ rows_out,
                                                      int32_t* __restrict__ flag) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) {
        int rows = 0, bad = 0;
        for (int b = 0; b < B; ++b) {
            const int n = tm_len(len_dev, sd, b);
            bad |= n != len_dev[b];
            rows += n;
        }
        if (rows_out) rows_out[0] = rows;
        if (bad && flag) flag[0] = 1;
    }
    if (r >= total) return;
    int b = 0, first = 0, off = 0;
    for (; b < B - 1; ++b) {
        const int seq = 1 + sd.s[b] * sd.s[b];
        if (r < first + seq) break;
        first += seq;
        off += tm_len(len_dev, sd, b);
    }
    const int j = r - first, n = tm_len(len_dev, sd, b);
    idx[r] = j == 0 ? -2 : (j <= n ? off + j - 1 : off + j - 1 - n);
}

// x rows [sum of the lengths, x_rows) <- 0: the rows of a slot behind this step's bags hold an earlier step's data
__global__ __launch_bounds__(256) void k_tm_zero_tail(const int32_t* __restrict__ len_dev, int B, TmSides sd, float* __restrict__ x,
                                                      int x_rows, int L) {
    int rows = 0;
    for (int b = 0; b < B; ++b) rows += tm_len(len_dev, sd, b);
    const int row = x_rows - 1 - (int)blockIdx.x;
    if (row < rows || row < 0) return;
    float4* p = reinterpret_cast<float4*>(x + (long)row * L);
    for (int c = threadIdx.x; c < L / 4; c += 256) p[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The sequence index of bags whose rows do NOT lie back to back (the fusion model's multi-modal bag: [all patches | small
// blocks] in memory, [tokens | patches] per bag in upstream's sequence order).  tab [B, TM_SEG_STRIDE] int32 on the device: per
// bag its grid side s, then TM_SEG_MAX segments (first row in the source, length) in sequence order, unused ones of length 0.
// Thread per entry, bag b owns 1 + s_b^2 entries: -2, the segments walked in order (L_b rows), the first s_b^2 - L_b of
// those again.  The position within the bag is clamped into [0, L_b - 1] and a resolved row outside [0, x_rows) becomes -1
// (a zero row), so no entry leaves the source whatever the table holds.  `flag` is raised (sticky) when L_b is outside
// ((s_b - 1)^2, s_b^2] or a row had to be dropped.  Any number of bags: the table is read, not passed by value.
constexpr int TM_SEG_MAX = 4, TM_SEG_STRIDE = 1 + 2 * TM_SEG_MAX;

__device__ __forceinline__ int tm_seg_side(const int32_t* __restrict__ tab, int b) {
    return min(max(tab[b * TM_SEG_STRIDE], 1), 4096);
}

__global__ __launch_bounds__(256) void k_tm_seq_index_segs(const int32_t* __restrict__ tab, int B, int total, int x_rows,
                                                           int32_t* __restrict__ idx, int32_t* __restrict__ flag) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= total) return;
    int b = 0, first = 0;
    for (; b < B - 1; ++b) {
        const int s = tm_seg_side(tab, b), seq = 1 + s * s;
        if (r < first + seq) break;
        first += seq;
    }
    const int32_t* t = tab + b * TM_SEG_STRIDE;
    const int s = tm_seg_side(tab, b), j = r - first;
    int len[TM_SEG_MAX], L = 0;
#pragma unroll
    for (int k = 0; k < TM_SEG_MAX; ++k) {
        len[k] = min(max(t[2 + 2 * k], 0), x_rows);          // x_rows < 2^31 / 4: the sum cannot wrap
        L += len[k];
    }
    if (j == 0) {
        if ((L > s * s || L <= (s - 1) * (s - 1)) && flag) flag[0] = 1;
        idx[r] = -2;
        return;
    }
    if (L == 0) {
        idx[r] = -1;
        return;
    }
    int pos = j - 1;
    if (pos >= L) pos -= L;                                  // the repeat of the first s^2 - L rows
    pos = min(max(pos, 0), L - 1);
    long row = -1;
    bool found = false;
#pragma unroll
    for (int k = 0; k < TM_SEG_MAX; ++k) {
        if (found) continue;
        if (pos < len[k]) {
            row = (long)t[1 + 2 * k] + pos;
            found = true;
        } else {
            pos -= len[k];
        }
    }
    if (row < 0 || row >= x_rows) {
        if (flag) flag[0] = 1;
        row = -1;
    }
    idx[r] = (int32_t)row;
}

// The same index for the fusion model's CAPACITY BUCKET (segments.FusionBucket), from the bag lengths on the device: the source
// rows are [cap patch rows | B tail_0 | B tail_1 | ..], bag b's pieces in sequence order are its tail segments in row order,
// (cap + B sum_{k<j} tail_k + b tail_j, tail_j), then its patches (len[0] + .. + len[b-1], len[b]).  Sides and tail counts come
// by value (what the captured step is keyed by), so there is no table and no host hop.  Entry by entry this is
// k_tm_seq_index_segs on those pieces: the position clamped into [0, L_b - 1], a row outside [0, cap + B sum tail) -> -1.
// Thread 0 of bag b's cls entry writes L_out[b] = len[b] + tail and raises `flag` (sticky) when L_b lies outside
// ((s_b - 1)^2, s_b^2]; thread 0 of the grid raises it when the lengths together exceed cap.
struct TmBucketGeo {
    int s[TM_MAX_BAGS];
    int tail[TM_SEG_MAX];
    int ntail;
};

__device__ __forceinline__ int tm_bucket_len(const int32_t* __restrict__ len_dev, int b, int x_rows) {
    return min(max(len_dev[b], 0), x_rows);                  // x_rows <= 2^29: L fits an int, the offsets are summed in long
}

__global__ __launch_bounds__(256) void k_tm_seq_index_bucket(const int32_t* __restrict__ len_dev, int B, int cap, TmBucketGeo geo,
                                                             int total, int x_rows, int32_t* __restrict__ idx,
                                                             int32_t* __restrict__ L_out, int32_t* __restrict__ flag) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0 && flag) {
        long rows = 0;
        for (int b = 0; b < B; ++b) rows += max(len_dev[b], 0);
        if (rows > cap) flag[0] = 1;
    }
    if (r >= total) return;
    int b = 0, first = 0;
    long off = 0;
    for (; b < B - 1; ++b) {
        const int seq = 1 + geo.s[b] * geo.s[b];
        if (r < first + seq) break;
        first += seq;
        off += tm_bucket_len(len_dev, b, x_rows);
    }
    const int s = geo.s[b], j = r - first, n = tm_bucket_len(len_dev, b, x_rows);
    int tails = 0;
#pragma unroll
    for (int k = 0; k < TM_SEG_MAX; ++k) tails += k < geo.ntail ? geo.tail[k] : 0;
    const int L = tails + n;                                 // >= 1: every tail segment holds a row
    if (j == 0) {
        if (L_out) L_out[b] = L;
        if ((L > s * s || L <= (s - 1) * (s - 1) || n != len_dev[b]) && flag) flag[0] = 1;
        idx[r] = -2;
        return;
    }
    int pos = j - 1;
    if (pos >= L) pos -= L;                                  // the repeat of the first s^2 - L rows
    pos = min(max(pos, 0), L - 1);
    long row = -1, base = cap;
    bool found = false;
#pragma unroll
    for (int k = 0; k < TM_SEG_MAX; ++k) {
        const int t = k < geo.ntail ? geo.tail[k] : 0;
        if (found) continue;
        if (pos < t) {
            row = base + (long)b * t + pos;
            found = true;
        } else {
            pos -= t;
            base += (long)B * t;
        }
    }
    if (!found) row = off + pos;                      // the patches: behind those of the bags in front
    if (row < 0 || row >= x_rows) {
        if (flag) flag[0] = 1;
        row = -1;
    }
    idx[r] = (int32_t)row;
}

// qL [8, 256, 64] = qscale * mean of l consecutive q rows, kL the same of k (no scale); thread per (landmark, q|k column)
__device__ __forceinline__ void tm_landmarks_body(const float* qkv, int l, float qscale, float* qL, float* kL) {
    const int j = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;        // c < 1024
    float s = 0.f;
    for (int t = 0; t < l; ++t) s += qkv[(long)(j * l + t) * TM_QKV + c];
    const int cc = c & (TM_D - 1), hh = cc >> 6, d = cc & 63;
    if (c < TM_D) qL[(hh * TM_M + j) * TM_DH + d] = s * (qscale / l);
    else kL[(hh * TM_M + j) * TM_DH + d] = s / l;
}

__global__ __launch_bounds__(256) void k_tm_landmarks(const float* __restrict__ qkv, int l, float qscale, float* qL, float* kL) {
    tm_landmarks_body(qkv, l, qscale, qL, kL);
}

// The packed forms below (csrc/tm_packed.h) run the single-bag bodies with the bag's own rows, group l_b and slices: the terms
// and the order of every sum of a bag are those of the single-bag kernel on that bag.
// blockIdx.z = the bag: the means of ITS l_b = blk_off[b + 1] - blk_off[b] rows, from its first row on, into slice b of qL / kL
__global__ __launch_bounds__(256) void k_tm_landmarks_packed(const float* __restrict__ qkv, const int32_t* __restrict__ tab, int nb,
                                                             int total_blocks, float qscale, float* qL, float* kL) {
    const int bag = blockIdx.z;
    int c0, c1;
    if (bag >= nb || !tm_packed_range(tab, total_blocks, bag, c0, c1)) return;
    const long small = (long)bag * TM_H * TM_M * TM_DH;
    tm_landmarks_body(qkv + (long)c0 * TM_PACKED_BLK * TM_QKV, c1 - c0, qscale, qL + small, kL + small);
}

// dqkv[i][q | k column] += coef * d(qL | kL)[head][i / l][d]; i counts from the bag's first row
__device__ __forceinline__ void tm_landmarks_bwd_body(const float* dqL, const float* dkL, int l, float qscale, float* dqkv, int i) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    const int cc = c & (TM_D - 1), hh = cc >> 6, d = cc & 63, j = i / l;
    const float g = c < TM_D ? dqL[(hh * TM_M + j) * TM_DH + d] * (qscale / l) : dkL[(hh * TM_M + j) * TM_DH + d] / l;
    dqkv[(long)i * TM_QKV + c] += g;
}

__global__ __launch_bounds__(256) void k_tm_landmarks_bwd(const float* __restrict__ dqL, const float* __restrict__ dkL, int l,
                                                          float qscale, float* dqkv) {
    tm_landmarks_bwd_body(dqL, dkL, l, qscale, dqkv, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_tm_landmarks_bwd_packed(const float* __restrict__ dqL, const float* __restrict__ dkL,
                                                                 const int32_t* __restrict__ tab, int nb, int total_blocks,
                                                                 float qscale, float* dqkv) {
    const int row = blockIdx.x;                                         // < 256 total_blocks: the grid
    const int bag = tm_packed_bag(tab, nb, total_blocks, row / TM_PACKED_BLK);
    int c0, c1;
    if (bag < 0 || !tm_packed_range(tab, total_blocks, bag, c0, c1)) return;
    const int i = row - c0 * TM_PACKED_BLK;                             // the row inside its bag
    if (i < 0 || i >= (c1 - c0) * TM_PACKED_BLK) return;                // a table whose two halves disagree
    const long small = (long)bag * TM_H * TM_M * TM_DH;
    tm_landmarks_bwd_body(dqL + small, dkL + small, c1 - c0, qscale, dqkv + (long)c0 * TM_PACKED_BLK * TM_QKV, i);
}

// The start of the pseudo-inverse and its backward, over nb bags at once: A2, Z0, dZ0, dA2 [nb, 8, 256, 256], scale
// [nb, PINV_SCALE] and arg [nb, PINV_ARG] dense over the bags.  Every kernel finds its bag from the block index and works on that
// bag's slices alone, so a bag's values and the order of its sums do not depend on nb; the single-bag entries launch the
// same kernels with nb = 1.  Offsets are long: nb <= 1024 bags of 2^19 floats reach 2^29 elements.
constexpr int PINV_SCALE = 3 + 2 * TM_H, PINV_ARG = 1 + TM_H;          // floats / ints per bag
constexpr int PINV_BAG = TM_H * TM_M * TM_M;                          // 2^19 elements of one bag's A2
constexpr int PINV_MAX_BAGS = 1024;

// per (bag, head h) (one workgroup each): out[3 + h] = max row abs-sum, out[11 + h] = max column abs-sum, arg[1 + h] = h * 256 +
// column of the largest column sum (first on ties), all local to the bag.  Rows: one wave per row, coalesced; columns: one
// thread per column.
__global__ __launch_bounds__(256) void k_tm_pinv_scale(const float* __restrict__ A2, float* out, int32_t* arg) {
    __shared__ float sr[4], sc[256];
    __shared__ int si[256];
    const int t = threadIdx.x, bag = blockIdx.x / TM_H, hh = blockIdx.x % TM_H, lane = t & 63, wv = t >> 6;
    const float* a = A2 + (long)blockIdx.x * TM_M * TM_M;
    out += bag * PINV_SCALE;
    arg += bag * PINV_ARG;
    float mr = 0.f;
    for (int i = wv; i < TM_M; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(a + i * TM_M + 4 * lane);
        mr = fmaxf(mr, wave_sum(fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[3])));
    }
    float cs = 0.f;
    for (int j = 0; j < TM_M; ++j) cs += fabsf(a[j * TM_M + t]);
    if (lane == 0) sr[wv] = mr;
    sc[t] = cs;
    si[t] = hh * TM_M + t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            const float c2 = sc[t + o];
            const int i2 = si[t + o];
            if (c2 > sc[t] || (c2 == sc[t] && i2 < si[t])) { sc[t] = c2; si[t] = i2; }
        }
        __syncthreads();
    }
    if (t == 0) {
        out[3 + hh] = fmaxf(fmaxf(sr[0], sr[1]), fmaxf(sr[2], sr[3]));
        out[3 + TM_H + hh] = sc[0];
        arg[1 + hh] = si[0];
    }
}

// the bag's scale from its own 8 heads' maxima (every thread, from cache), then Z0[h][i][j] = A2[h][j][i] / scale; the bag's
// first thread stores out[0] = max row abs-sum x max column abs-sum, out[1] / out[2] the two factors, arg[0] the arg-max column
__global__ __launch_bounds__(256) void k_tm_pinv_init(const float* __restrict__ A2, float* scale, int32_t* arg, float* Z) {
    const int bag = blockIdx.x / (PINV_BAG / 256);
    scale += bag * PINV_SCALE;
    arg += bag * PINV_ARG;
    float mr = 0.f, mc = -1.f;
    int ic = 0;
#pragma unroll
    for (int hh = 0; hh < TM_H; ++hh) {
        mr = fmaxf(mr, scale[3 + hh]);
        if (scale[3 + TM_H + hh] > mc) { mc = scale[3 + TM_H + hh]; ic = arg[1 + hh]; }
    }
    const float sv = mr * mc;
    const int e = (blockIdx.x % (PINV_BAG / 256)) * 256 + threadIdx.x;  // < 8 * 256 * 256, within the bag
    const int hh = e >> 16, i = (e >> 8) & 255, j = e & 255;
    const long off = (long)bag * PINV_BAG;
    Z[off + e] = A2[off + (hh << 16) + (j << 8) + i] / sv;
    if (e == 0) {
        scale[0] = sv;
        scale[1] = mr;
        scale[2] = mc;
        arg[0] = ic;
    }
}

// ws[bag] += <dZ0, Z0> over the bag's 2048-element chunks (ws caller-zeroed); FIXED: ws[bag * 256 + chunk] = the chunk's sum,
// a plain store
constexpr int PINV_CHUNKS = PINV_BAG / 2048;                 // 256 per bag: k_tm_pinv_init_bwd_s<true> has one thread per chunk
template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_pinv_dot(const float* __restrict__ dZ0, const float* __restrict__ Z0, float* ws) {
    __shared__ float red[4];
    const long base = (long)blockIdx.x * 2048;
    float s = 0.f;
    for (long e = base + threadIdx.x; e < base + 2048; e += 256) s += dZ0[e] * Z0[e];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = red[0] + red[1] + red[2] + red[3];
        if constexpr (FIXED) ws[blockIdx.x] = v;
        else atomicAdd(ws + blockIdx.x / PINV_CHUNKS, v);
    }
}

// dA2[h][i][j] += dZ0[h][j][i] / s, s the bag's own
__global__ __launch_bounds__(256) void k_tm_pinv_init_bwd_t(const float* __restrict__ dZ0, const float* __restrict__ scale,
                                                            float* dA2) {
    const int bag = blockIdx.x / (PINV_BAG / 256);
    const int e = (blockIdx.x % (PINV_BAG / 256)) * 256 + threadIdx.x;
    const int hh = e >> 16, i = (e >> 8) & 255, j = e & 255;
    const long off = (long)bag * PINV_BAG;
    dA2[off + e] += dZ0[off + (hh << 16) + (j << 8) + i] / scale[bag * PINV_SCALE];
}

// the scale's gradient ds = -<dZ0, Z0> / s (ws[bag], k_tm_pinv_dot) goes to the arg-max column through its column-sum
// factor: dA2[h*][i][j*] += ds * (max row abs-sum) (A2 > 0 after softmax, so |.|' = 1).  One workgroup per bag, one thread per row.
// FIXED: <dZ0, Z0> is the sum of the bag's 256 chunk sums in ws, by the xor butterfly of each wave and then wave 0 .. 3 in order.
template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_pinv_init_bwd_s(const float* __restrict__ ws, const float* __restrict__ scale,
                                                            const int32_t* __restrict__ arg, float* dA2) {
    const int t = threadIdx.x, bag = blockIdx.x;
    scale += bag * PINV_SCALE;
    arg += bag * PINV_ARG;
    float dot;
    if constexpr (FIXED) {
        __shared__ float red[4];
        const float s = wave_sum(ws[bag * PINV_CHUNKS + t]);
        if ((t & 63) == 0) red[t >> 6] = s;
        __syncthreads();
        dot = red[0] + red[1] + red[2] + red[3];
    } else {
        dot = ws[bag];
    }
    const float ds = -dot / scale[0];
    const int hh = arg[0] >> 8, jc = arg[0] & 255;
    dA2[(long)bag * PINV_BAG + (hh << 16) + (t << 8) + jc] += ds * scale[1];
}

// out[i][c] += sum_t w[head][t] v[i + t - 16][c] (v = columns 1024.. of qkv, zero outside [0, n_pad))
// The conv kernels clip the window at [lo, hi): the single-bag ones at [0, n), compiled to what they were; the packed ones
// (csrc/tm_packed.h) at the first and one-past-last row of the row's OWN bag, so that no tap reaches a neighbour's rows - the
// sums of a row are then those of the single-bag kernel on its bag.  The bodies' pointers carry no __restrict__: inlined, they
// ARE the kernel's arguments.
__device__ __forceinline__ void tm_resconv_body(const float* qkv, const float* w, int lo, int hi, float* out) {
    const int i = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, hh = c >> 6;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TM_CONV; ++t) {
        const int ii = i + t - TM_CONV / 2;
        if (ii >= lo && ii < hi) s += w[hh * TM_CONV + t] * qkv[(long)ii * TM_QKV + 2 * TM_D + c];
    }
    out[(long)i * TM_D + c] += s;
}

__global__ __launch_bounds__(256) void k_tm_resconv(const float* __restrict__ qkv, const float* __restrict__ w, int n, float* out) {
    tm_resconv_body(qkv, w, 0, n, out);
}

// the rows [lo, hi) of the bag that owns 256-row block `blk`, clamped into [0, 256 total_blocks); false: the workgroup returns
__device__ __forceinline__ bool tm_packed_rows(const int32_t* __restrict__ tab, int nb, int total_blocks, int blk, int& lo, int& hi) {
    const int bag = tm_packed_bag(tab, nb, total_blocks, blk);
    int c0, c1;
    if (bag < 0 || !tm_packed_range(tab, total_blocks, bag, c0, c1)) return false;
    lo = c0 * TM_PACKED_BLK;
    hi = c1 * TM_PACKED_BLK;
    return true;
}

__global__ __launch_bounds__(256) void k_tm_resconv_packed(const float* __restrict__ qkv, const float* __restrict__ w,
                                                           const int32_t* __restrict__ tab, int nb, int total_blocks, float* out) {
    int lo, hi;
    if (!tm_packed_rows(tab, nb, total_blocks, blockIdx.x / TM_PACKED_BLK, lo, hi)) return;
    tm_resconv_body(qkv, w, lo, hi, out);
}

// dv[i][c] += sum_t w[head][t] dout[i - t + 16][c], into the v columns of dqkv.  Templated as a whole (TmPackedArg), not
// built on a shared body: with its clip passed as arguments the single-bag kernel comes out three registers wider.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_tm_resconv_bwd_dv(const float* __restrict__ dout, const float* __restrict__ w, int n,
                                                           float* dqkv, TmPackedArg<PACKED> pk) {
    const int i = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, hh = c >> 6;
    float s = 0.f;
    if constexpr (PACKED) {
        int lo, hi;
        if (!tm_packed_rows(pk.tab, pk.nb, pk.total_blocks, i / TM_PACKED_BLK, lo, hi)) return;
#pragma unroll
        for (int t = 0; t < TM_CONV; ++t) {
            const int ii = i - t + TM_CONV / 2;
            if (ii >= lo && ii < hi) s += w[hh * TM_CONV + t] * dout[(long)ii * TM_D + c];
        }
    } else {
#pragma unroll
        for (int t = 0; t < TM_CONV; ++t) {
            const int ii = i - t + TM_CONV / 2;
            if (ii >= 0 && ii < n) s += w[hh * TM_CONV + t] * dout[(long)ii * TM_D + c];
        }
    }
    dqkv[(long)i * TM_QKV + 2 * TM_D + c] += s;
}

// dw[head][t] += sum over a chunk of rows i and d of dout[i][head, d] v[i + t - 16][head, d]; block (head * 33 + t, chunk)
// FIXED: dw is the workspace [chunks][8 x 33] and the chunk's sum a plain store into its row (k_tm_fold adds the rows)
// PACKED: n = 256 total_blocks, a chunk is a block of one bag and the window is clipped at that bag's rows; a chunk whose bag
// the table does not give adds nothing (FIXED: stores 0, so that the fold reads no stale float)
constexpr int RC_CHUNK = 256;
static_assert(RC_CHUNK == TM_PACKED_BLK, "a conv chunk of the packed form is one block");
template <bool FIXED, bool PACKED>
__device__ __forceinline__ void tm_resconv_bwd_dw_body(const float* dout, const float* qkv, int n, float* dw, const int32_t* tab,
                                                       int nb, int total_blocks) {
    __shared__ float red[4];
    const int hh = blockIdx.x / TM_CONV, t = blockIdx.x % TM_CONV;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = hh * TM_DH + lane;
    int r0 = blockIdx.y * RC_CHUNK, r1 = min(n, r0 + RC_CHUNK), lo = 0, hi = n;
    if constexpr (PACKED) {
        if (!tm_packed_rows(tab, nb, total_blocks, blockIdx.y, lo, hi)) r1 = r0;      // uniform per workgroup
    }
    float s = 0.f;
    for (int i = r0 + wv; i < r1; i += 4) {
        const int ii = i + t - TM_CONV / 2;
        if (ii >= lo && ii < hi) s += dout[(long)i * TM_D + c] * qkv[(long)ii * TM_QKV + 2 * TM_D + c];
    }
    s = wave_sum(s);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = red[0] + red[1] + red[2] + red[3];
        if constexpr (FIXED) dw[blockIdx.y * (TM_H * TM_CONV) + blockIdx.x] = v;
        else atomicAdd(dw + blockIdx.x, v);
    }
}

template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_resconv_bwd_dw(const float* __restrict__ dout, const float* __restrict__ qkv, int n,
                                                           float* dw) {
    tm_resconv_bwd_dw_body<FIXED, false>(dout, qkv, n, dw, nullptr, 0, 0);
}

template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_resconv_bwd_dw_packed(const float* __restrict__ dout, const float* __restrict__ qkv,
                                                                  float* dw, const int32_t* __restrict__ tab, int nb,
                                                                  int total_blocks) {
    tm_resconv_bwd_dw_body<FIXED, true>(dout, qkv, total_blocks * TM_PACKED_BLK, dw, tab, nb, total_blocks);
}

// PPEG: y[1 + i s + j][c] = bias[c] + sum_{a,b < 7} Wf[c][a][b] x[1 + (i + a - 3) s + (j + b - 3)][c], y[0] = x[0];
// Wf = W7 + pad(W5) + pad(W3) + delta, bias = b7 + b5 + b3.  flip = 1: the transposed map (dx from dy, no bias).
constexpr int PPEG_COLS = 8;      // grid columns per workgroup: s rows x 2 channel halves x ceil(s / 8) workgroups
__device__ __forceinline__ void tm_ppeg_fold(const float* W7, const float* W5, const float* W3, int c, float* wf) {
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            float v = W7[c * 49 + a * 7 + b];
            if (a >= 1 && a < 6 && b >= 1 && b < 6) v += W5[c * 25 + (a - 1) * 5 + (b - 1)];
            if (a >= 2 && a < 5 && b >= 2 && b < 5) v += W3[c * 9 + (a - 2) * 3 + (b - 2)];
            if (a == 3 && b == 3) v += 1.f;
            wf[a * 7 + b] = v;
        }
}

// The body of one workgroup: grid row i, channel half blockIdx.y, the columns of chunk jz of ONE bag whose rows start at x / y.
// The single-bag kernel passes blockIdx.x / blockIdx.z; the packed one the bag's grid row, with x and y moved to the bag's rows.
__device__ __forceinline__ void tm_ppeg_body(const float* __restrict__ x, int s, const float* __restrict__ W7,
                                             const float* __restrict__ b7, const float* __restrict__ W5,
                                             const float* __restrict__ b5, const float* __restrict__ W3,
                                             const float* __restrict__ b3, int flip, float* __restrict__ y, const int i,
                                             const int jz) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    float wf[49];
    tm_ppeg_fold(W7, W5, W3, c, wf);
    const float bias = flip ? 0.f : b7[c] + b5[c] + b3[c];
    if (i == 0 && jz == 0) y[c] = x[c];
    const int j0 = jz * PPEG_COLS, j1 = min(s, j0 + PPEG_COLS);
    for (int j = j0; j < j1; ++j) {
        float acc = bias;
#pragma unroll
        for (int a = 0; a < 7; ++a) {
            const int ii = flip ? i - (a - 3) : i + (a - 3);
            if (ii < 0 || ii >= s) continue;
#pragma unroll
            for (int b = 0; b < 7; ++b) {
                const int jj = flip ? j - (b - 3) : j + (b - 3);
                if (jj < 0 || jj >= s) continue;
                acc += wf[a * 7 + b] * x[(long)(1 + ii * s + jj) * TM_D + c];
            }
        }
        y[(long)(1 + i * s + j) * TM_D + c] = acc;
    }
}

__global__ __launch_bounds__(256) void k_tm_ppeg(const float* __restrict__ x, int s, const float* __restrict__ W7,
                                                 const float* __restrict__ b7, const float* __restrict__ W5,
                                                 const float* __restrict__ b5, const float* __restrict__ W3,
                                                 const float* __restrict__ b3, int flip, float* __restrict__ y) {
    tm_ppeg_body(x, s, W7, b7, W5, b5, W3, b3, flip, y, blockIdx.x, blockIdx.z);
}

// All bags of a step (csrc/tm_ppeg_packed.h): the single-bag grid flattened over the bags - blockIdx.x the packed grid row, the
// table gives its bag, that bag's side and first row and the grid row inside the bag; a workgroup past a smaller bag's column
// chunks returns.  Every bag's cls row passes through (its grid row 0, column chunk 0).
__global__ __launch_bounds__(256) void k_tm_ppeg_packed(const float* __restrict__ x, const float* __restrict__ W7,
                                                        const float* __restrict__ b7, const float* __restrict__ W5,
                                                        const float* __restrict__ b5, const float* __restrict__ W3,
                                                        const float* __restrict__ b3, int flip, float* __restrict__ y,
                                                        const int32_t* __restrict__ tab, int nb, int total_rows, int gmax) {
    int s, row, i;
    if (!tm_ppeg_gridrow(tab, nb, total_rows, gmax, blockIdx.x, s, row, i)) return;
    if ((int)blockIdx.z * PPEG_COLS >= s) return;
    const long off = (long)row * TM_D;
    tm_ppeg_body(x + off, s, W7, b7, W5, b5, W3, b3, flip, y + off, i, blockIdx.z);
}

// dWf[c][tap] (tap < 49) and db[c] (tap 49) += sums over a chunk of 8 grid rows; thread per (tap, channel)
// FIXED: dWf is the workspace [chunks][50 x 512], a chunk's row laid out [dWf 512 x 49 | db 512], plain stores (db unused)
// The body of one workgroup: the chunk of grid rows [r0, r0 + 8) of ONE bag whose rows start at dy / x; FIXED: into row `chunk`.
constexpr int PPEG_ROWS = 8;
static_assert(PPEG_ROWS == TM_PPEG_CHUNK && TM_D == TM_PPEG_D, "the PPEG table's chunks are those of k_tm_ppeg_dw");
template <bool FIXED>
__device__ __forceinline__ void tm_ppeg_dw_body(const float* __restrict__ dy, const float* __restrict__ x, int s, float* dWf,
                                                float* db, const int r0, const int chunk) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 50 * TM_D) return;
    const int tap = e / TM_D, c = e % TM_D, a = tap / 7 - 3, b = tap % 7 - 3;
    const int r1 = min(s, r0 + PPEG_ROWS);
    float acc = 0.f;
    for (int i = r0; i < r1; ++i) {
        if (tap == 49) {
            for (int j = 0; j < s; ++j) acc += dy[(long)(1 + i * s + j) * TM_D + c];
            continue;
        }
        const int ii = i + a;
        if (ii < 0 || ii >= s) continue;
        for (int j = max(0, -b); j < min(s, s - b); ++j)
            acc += dy[(long)(1 + i * s + j) * TM_D + c] * x[(long)(1 + ii * s + j + b) * TM_D + c];
    }
    if constexpr (FIXED) {
        dWf[(long)chunk * (50 * TM_D) + (tap == 49 ? 49 * TM_D + c : c * 49 + tap)] = acc;
    } else {
        if (tap == 49) atomicAdd(db + c, acc);
        else atomicAdd(dWf + c * 49 + tap, acc);
    }
}

template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_ppeg_dw(const float* __restrict__ dy, const float* __restrict__ x, int s, float* dWf,
                                                    float* db) {
    tm_ppeg_dw_body<FIXED>(dy, x, s, dWf, db, blockIdx.y * PPEG_ROWS, blockIdx.y);
}

// All bags of a step: blockIdx.y the packed chunk (bag 0's chunks first, ascending), the table gives its bag and first grid row.
// A chunk the table does not place adds nothing; FIXED: it stores 0 into its row when the fold will read that row (k below the
// table's chunk count), so that the fold reads no stale float, and touches nothing otherwise.
template <bool FIXED>
__global__ __launch_bounds__(256) void k_tm_ppeg_dw_packed(const float* __restrict__ dy, const float* __restrict__ x, float* dWf,
                                                           float* db, const int32_t* __restrict__ tab, int nb, int total_rows,
                                                           int gmax, int cmax) {
    const int k = blockIdx.y;
    int s, row, r0;
    if (!tm_ppeg_chunk(tab, nb, total_rows, gmax, cmax, k, s, row, r0)) {
        if constexpr (FIXED) {
            const int e = blockIdx.x * 256 + threadIdx.x;
            if (k < tm_ppeg_chunks(tab, nb, cmax) && e < 50 * TM_D) dWf[(long)k * (50 * TM_D) + e] = 0.f;
        }
        return;
    }
    if constexpr (FIXED)
        if (k >= tm_ppeg_chunks(tab, nb, cmax)) return;             // behind the rows the workspace holds
    const long off = (long)row * TM_D;
    tm_ppeg_dw_body<FIXED>(dy + off, x + off, s, dWf, db, r0, k);
}

// dWf [512 x 49] | db [512] <- the sum of the workspace rows [dWf | db] of the table's chunks, chunk 0, 1, 2 .. in that order
__global__ __launch_bounds__(256) void k_tm_ppeg_fold_packed(const float* __restrict__ ws, const int32_t* __restrict__ tab, int nb,
                                                             int cmax, float* __restrict__ dWf, float* __restrict__ db) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 50 * TM_D) return;
    const int chunks = tm_ppeg_chunks(tab, nb, cmax);
    float v = chunks > 0 ? ws[e] : 0.f;
    for (int c = 1; c < chunks; ++c) v += ws[(long)c * (50 * TM_D) + e];
    if (e < 49 * TM_D) dWf[e] = v;
    else db[e - 49 * TM_D] = v;
}

// Per-patch cls-token attention: the cls row (padded row `pad`) of A1 Z A3 without the [n_pad, n_pad] map, in two launches.
// t[h][:] = A1[h][pad][:] Z[h] comes from a tiny launch of its own (8 x 4 workgroups into an [8, 256] workspace) rather than
// a per-workgroup recompute: every workgroup of the stream below would otherwise re-read its head's 256 KiB of Z.
// Workgroup (64 columns of Z, head); wave w sums k in [64 w, 64 w + 64), the four partial sums are added in a fixed order.
__global__ __launch_bounds__(256) void k_tm_cls_t(const float* __restrict__ A1, const float* __restrict__ Z, int n_pad, int pad,
                                                  float* __restrict__ t) {
    __shared__ float red[4][64];
    const int hh = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
    const float* a = A1 + ((long)hh * n_pad + pad) * TM_M + 64 * wv;
    const float* z = Z + ((long)hh * TM_M + 64 * wv) * TM_M + j;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) s += a[k] * z[k * TM_M];
    red[wv][lane] = s;
    __syncthreads();
    if (wv == 0) t[hh * TM_M + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// out[h][i] = sum_m t[h][m] (A3[h][m][pad + 1 + i] + (i < add ? A3[h][m][pad + 1 + N + i] : 0)) for i < N, 0 for N <= i < s^2:
// a repeated patch gets the sum of its two keys.  One pass over the sequence columns of A3 with lanes along the column
// index; the front-pad columns and the cls column are never read.  Workgroup (64 V patches, head): the thread of patches
// i0 .. i0 + V - 1 forms both of their column sums over the 64 rows of its wave, the four waves' partial sums are added in a
// fixed order.  V = 4 (16-byte loads) wants pad + 1 = n_pad - s^2 a multiple of 4, i.e. an even side; the repeats' columns
// start at N, so their loads are wide only where N % 4 == 0 and the whole group lies below add.
// len_dev != null: N is bag `bag`'s length on the device, clamped into the side's bucket as k_tm_seq_index does (which also
// raises the out-of-bucket flag), so no column index leaves [pad + 1, n_pad).
template <int V>
__global__ __launch_bounds__(256) void k_tm_cls_row(const float* __restrict__ t, const float* __restrict__ A3, int n_pad, int pad,
                                                    int s, int n_host, const int32_t* __restrict__ len_dev, int bag,
                                                    float* __restrict__ out) {
    __shared__ float red[4][64 * V];
    const int S2 = s * s;
    const int N = len_dev != nullptr ? min(max(len_dev[bag], (s - 1) * (s - 1) + 1), S2) : n_host;
    const int add = S2 - N;
    const int hh = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = (blockIdx.x * 64 + lane) * V;
    const bool p_on = i0 < N, r_on = i0 < add;                       // i0 < N <= S2: every primary load stays in the row
    const bool r_wide = V == 4 && (N & 3) == 0 && i0 + V <= add;
    const float* tt = t + hh * TM_M + 64 * wv;
    const float* a = A3 + ((long)hh * TM_M + 64 * wv) * n_pad + pad + 1 + i0;
    float acc[V], rep[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = rep[v] = 0.f;
    if (p_on) {
#pragma unroll 8
        for (int m = 0; m < 64; ++m) {
            const float tm = tt[m];
            const float* row = a + (long)m * n_pad;
            if constexpr (V == 4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(row);
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[v] += tm * x[v];
            } else {
                acc[0] += tm * row[0];
            }
            if (r_on) {
                if constexpr (V == 4) {
                    if (r_wide) {
                        const f32x4 y = *reinterpret_cast<const f32x4*>(row + N);
#pragma unroll
                        for (int v = 0; v < 4; ++v) rep[v] += tm * y[v];
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                            if (i0 + v < add) rep[v] += tm * row[N + v];
                    }
                } else {
                    rep[0] += tm * row[N];
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) red[wv][lane * V + v] = acc[v] + rep[v];
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = i0 + v, e = lane * V + v;
        if (i < S2) out[(long)hh * S2 + i] = i < N ? (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]) : 0.f;
    }
}

inline int launch_rc() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MIL_OK : (int)e;
}

// the launches of the pseudo-inverse's start over nb bags; the entries below check their arguments first
void tm_pinv_init_launch(const float* A2, int nb, float* scale, int32_t* arg, float* Z0, hipStream_t st) {
    hipLaunchKernelGGL(k_tm_pinv_scale, dim3(nb * TM_H), dim3(256), 0, st, A2, scale, arg);
    hipLaunchKernelGGL(k_tm_pinv_init, dim3(nb * (PINV_BAG / 256)), dim3(256), 0, st, A2, scale, arg, Z0);
}

template <bool FIXED>
void tm_pinv_init_bwd_launch(const float* dZ0, const float* Z0, const float* scale, const int32_t* arg, int nb, float* dA2,
                                    float* ws, hipStream_t st) {
    hipLaunchKernelGGL(k_tm_pinv_init_bwd_t, dim3(nb * (PINV_BAG / 256)), dim3(256), 0, st, dZ0, scale, dA2);
    hipLaunchKernelGGL(k_tm_pinv_dot<FIXED>, dim3(nb * PINV_CHUNKS), dim3(256), 0, st, dZ0, Z0, ws);
    hipLaunchKernelGGL(k_tm_pinv_init_bwd_s<FIXED>, dim3(nb), dim3(256), 0, st, ws, scale, arg, dA2);
}

}  // namespace

extern "C" {

int mil_tm_bgemm(const float* A, long sAb, long sAi, long sAk, const float* B, long sBb, long sBk, long sBj, float* C, long sCb,
                 long sCi, long sCj, const float* D, int batch, int M, int N, int K, float alpha, float beta, float diag,
                 int splits, void* stream) {
    if (!tm_bgemm_args_ok(A, B, C, batch, M, N, K, splits, 64) || !tm_bgemm_atomic_ok(beta, D, splits)) return MIL_EINVAL;
    dim3 grid((N + 63) / 64, (M + 63) / 64, batch * splits);
    hipLaunchKernelGGL(k_tm_bgemm<false>, grid, dim3(256), 0, (hipStream_t)stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb, sCi,
                       sCj, D, M, N, K, alpha, beta, diag, splits);
    return launch_rc();
}

int mil_tm_softmax_rows(float* x, long rows, int cols, void* stream) {
    if (!x || rows <= 0 || cols <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_softmax, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, rows, cols);
    return launch_rc();
}

int mil_tm_softmax_rows_bwd(const float* p, float* dp, long rows, int cols, void* stream) {
    if (!p || !dp || rows <= 0 || cols <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_softmax_bwd, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, dp, rows, cols);
    return launch_rc();
}

int mil_tm_row_gather(const float* src, const float* extra, const int32_t* idx, int rows, int E, float* dst, void* stream) {
    if (!src || !idx || !dst || rows <= 0 || E <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_gather, dim3(rows), dim3(256), 0, (hipStream_t)stream, src, extra, idx, E, dst);
    return launch_rc();
}

int mil_tm_row_gather_bwd(const float* ddst, const int32_t* idx, int rows, int E, float* dsrc, float* dextra, void* stream) {
    if (!ddst || !idx || !dsrc || rows <= 0 || E <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_gather_bwd, dim3(rows), dim3(256), 0, (hipStream_t)stream, ddst, idx, E, dsrc, dextra);
    return launch_rc();
}

int mil_tm_seq_index(const int32_t* len_dev, int B, const int32_t* s_of_bag, int32_t* idx_out, int idx_rows, int32_t* rows_dev_out,
                     int32_t* flag_dev, float* x_tail, int x_rows, int L, void* stream) {
    if (!len_dev || !s_of_bag || !idx_out || B <= 0 || B > TM_MAX_BAGS) return MIL_EINVAL;
    TmSides sd{};
    long total = 0, cap = 0, slack = 0;
    for (int b = 0; b < B; ++b) {
        const int s = s_of_bag[b];
        if (s < 1 || s > 4096) return MIL_EINVAL;
        sd.s[b] = s;
        total += 1 + (long)s * s;
        cap += (long)s * s;
        slack += 2 * (long)s - 2;                    // s^2 minus the shortest length of the side, (s - 1)^2 + 1
    }
    if (total > idx_rows) return MIL_EINVAL;
    if (x_tail && (x_rows < cap || L <= 0 || (L & 3) || (reinterpret_cast<uintptr_t>(x_tail) & 15))) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_seq_index, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, len_dev, B, sd,
                       (int)total, idx_out, rows_dev_out, flag_dev);
    const long tail = x_tail ? (long)x_rows - cap + slack : 0;     // most rows that can lie behind the bags
    if (tail > 0)
        hipLaunchKernelGGL(k_tm_zero_tail, dim3((unsigned)(tail < x_rows ? tail : x_rows)), dim3(256), 0, (hipStream_t)stream, len_dev,
                           B, sd, x_tail, x_rows, L);
    return launch_rc();
}

int mil_tm_seq_index_segs(const int32_t* table_dev, int B, int total, int x_rows, int32_t* idx_out, int idx_rows, int32_t* flag_dev,
                          void* stream) {
    if (!table_dev || !idx_out || B <= 0 || B > 65536 || total <= 0 || total > idx_rows || x_rows <= 0 || x_rows > (1 << 29))
        return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_seq_index_segs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table_dev, B,
                       total, x_rows, idx_out, flag_dev);
    return launch_rc();
}

int mil_tm_seq_index_bucket(const int32_t* len_dev, int B, int cap, const int32_t* tail, int ntail, const int32_t* s_of_bag,
                            int32_t* idx_out, int idx_rows, int32_t* L_dev_out, int32_t* flag_dev, void* stream) {
    if (!len_dev || !tail || !s_of_bag || !idx_out || B <= 0 || B > TM_MAX_BAGS || cap <= 0 || ntail < 1 || ntail > TM_SEG_MAX)
        return MIL_EINVAL;
    TmBucketGeo geo{};
    long total = 0, x_rows = cap;
    for (int b = 0; b < B; ++b) {
        const int s = s_of_bag[b];
        if (s < 1 || s > 4096) return MIL_EINVAL;
        geo.s[b] = s;
        total += 1 + (long)s * s;
    }
    for (int k = 0; k < ntail; ++k) {
        if (tail[k] < 1 || tail[k] > (1 << 20)) return MIL_EINVAL;
        geo.tail[k] = tail[k];
        x_rows += (long)B * tail[k];
    }
    geo.ntail = ntail;
    if (total > idx_rows || x_rows > (1 << 29)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_seq_index_bucket, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, len_dev, B,
                       cap, geo, (int)total, (int)x_rows, idx_out, L_dev_out, flag_dev);
    return launch_rc();
}

int mil_tm_landmarks(const float* qkv, int n_pad, float qscale, float* qL, float* kL, void* stream) {
    if (!qkv || !qL || !kL || n_pad <= 0 || n_pad % TM_M) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_landmarks, dim3(TM_M, 4), dim3(256), 0, (hipStream_t)stream, qkv, n_pad / TM_M, qscale, qL, kL);
    return launch_rc();
}

int mil_tm_landmarks_bwd(const float* dqL, const float* dkL, int n_pad, float qscale, float* dqkv, void* stream) {
    if (!dqL || !dkL || !dqkv || n_pad <= 0 || n_pad % TM_M) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_landmarks_bwd, dim3(n_pad, 4), dim3(256), 0, (hipStream_t)stream, dqL, dkL, n_pad / TM_M, qscale, dqkv);
    return launch_rc();
}

int mil_tm_pinv_init(const float* A2, float* scale, int32_t* arg, float* Z0, void* stream) {
    if (!A2 || !scale || !arg || !Z0) return MIL_EINVAL;
    tm_pinv_init_launch(A2, 1, scale, arg, Z0, (hipStream_t)stream);
    return launch_rc();
}

int mil_tm_pinv_init_bwd(const float* dZ0, const float* Z0, const float* scale, const int32_t* arg, float* dA2, float* ws,
                         void* stream) {
    if (!dZ0 || !Z0 || !scale || !arg || !dA2 || !ws) return MIL_EINVAL;
    tm_pinv_init_bwd_launch<false>(dZ0, Z0, scale, arg, 1, dA2, ws, (hipStream_t)stream);
    return launch_rc();
}

int mil_tm_pinv_init_bags(const float* A2, int nb, float* scale, int32_t* arg, float* Z0, void* stream) {
    if (!A2 || !scale || !arg || !Z0 || nb < 1 || nb > PINV_MAX_BAGS) return MIL_EINVAL;
    tm_pinv_init_launch(A2, nb, scale, arg, Z0, (hipStream_t)stream);
    return launch_rc();
}

int mil_tm_pinv_init_bwd_bags(const float* dZ0, const float* Z0, const float* scale, const int32_t* arg, int nb, float* dA2,
                              float* ws, void* stream) {
    if (!dZ0 || !Z0 || !scale || !arg || !dA2 || !ws || nb < 1 || nb > PINV_MAX_BAGS) return MIL_EINVAL;
    tm_pinv_init_bwd_launch<false>(dZ0, Z0, scale, arg, nb, dA2, ws, (hipStream_t)stream);
    return launch_rc();
}

int mil_tm_resconv(const float* qkv, const float* w, int n_pad, float* out, void* stream) {
    if (!qkv || !w || !out || n_pad <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_resconv, dim3(n_pad, 2), dim3(256), 0, (hipStream_t)stream, qkv, w, n_pad, out);
    return launch_rc();
}

int mil_tm_resconv_bwd(const float* dout, const float* qkv, const float* w, int n_pad, float* dqkv, float* dw, void* stream) {
    if (!dout || !qkv || !w || !dqkv || !dw || n_pad <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_resconv_bwd_dv<false>, dim3(n_pad, 2), dim3(256), 0, (hipStream_t)stream, dout, w, n_pad, dqkv,
                       TmPackedArg<false>{});
    hipLaunchKernelGGL(k_tm_resconv_bwd_dw<false>, dim3(TM_H * TM_CONV, (n_pad + RC_CHUNK - 1) / RC_CHUNK), dim3(256), 0,
                       (hipStream_t)stream, dout, qkv, n_pad, dw);
    return launch_rc();
}

int mil_tm_ppeg_fwd(const float* x, int s, const float* W7, const float* b7, const float* W5, const float* b5, const float* W3,
                    const float* b3, float* y, void* stream) {
    if (!x || !W7 || !b7 || !W5 || !b5 || !W3 || !b3 || !y || s <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_ppeg, dim3(s, 2, (s + PPEG_COLS - 1) / PPEG_COLS), dim3(256), 0, (hipStream_t)stream, x, s, W7, b7, W5, b5, W3, b3, 0, y);
    return launch_rc();
}

int mil_tm_ppeg_bwd(const float* dy, const float* x, int s, const float* W7, const float* W5, const float* W3, float* dx,
                    float* dWf, float* db, void* stream) {
    if (!dy || !x || !W7 || !W5 || !W3 || !dx || !dWf || !db || s <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_ppeg, dim3(s, 2, (s + PPEG_COLS - 1) / PPEG_COLS), dim3(256), 0, (hipStream_t)stream, dy, s, W7, W7, W5, W5, W3, W3, 1, dx);
    hipLaunchKernelGGL(k_tm_ppeg_dw<false>, dim3((50 * TM_D + 255) / 256, (s + PPEG_ROWS - 1) / PPEG_ROWS), dim3(256), 0,
                       (hipStream_t)stream, dy, x, s, dWf, db);
    return launch_rc();
}

int mil_tm_cls_attn(const float* A1, const float* Z, const float* A3, int n_pad, int pad, int s, int n, const int32_t* len_dev,
                    int bag, float* t_ws, float* out, void* stream) {
    if (!A1 || !Z || !A3 || !t_ws || !out || n_pad <= 0 || n_pad % TM_M || s < 1 || s > 4096) return MIL_EINVAL;
    const long S2 = (long)s * s;
    if (pad < 0 || (long)pad + 1 + S2 != n_pad) return MIL_EINVAL;
    if (len_dev != nullptr ? (bag < 0 || bag >= TM_MAX_BAGS) : (n > S2 || n <= (long)(s - 1) * (s - 1))) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_cls_t, dim3(TM_M / 64, TM_H), dim3(256), 0, (hipStream_t)stream, A1, Z, n_pad, pad, t_ws);
    const bool wide = (s & 1) == 0 && !(reinterpret_cast<uintptr_t>(A3) & 15);
    if (wide)
        hipLaunchKernelGGL(k_tm_cls_row<4>, dim3((unsigned)((S2 + 255) / 256), TM_H), dim3(256), 0, (hipStream_t)stream, t_ws, A3,
                           n_pad, pad, s, n, len_dev, bag, out);
    else
        hipLaunchKernelGGL(k_tm_cls_row<1>, dim3((unsigned)((S2 + 63) / 64), TM_H), dim3(256), 0, (hipStream_t)stream, t_ws, A3,
                           n_pad, pad, s, n, len_dev, bag, out);
    return launch_rc();
}

// ---- the fixed-order entries: every partial sum a plain store into the caller's workspace, added in ascending order by a
// second launch; no float atomic, no counter, the launch boundary is the barrier
size_t mil_tm_bgemm_ws_floats(int batch, int M, int N, int splits) {
    if (batch <= 0 || M <= 0 || N <= 0 || splits <= 1) return 0;
    return (size_t)splits * batch * M * N;
}

int mil_tm_bgemm_fixed(const float* A, long sAb, long sAi, long sAk, const float* B, long sBb, long sBk, long sBj, float* C,
                       long sCb, long sCi, long sCj, const float* D, int batch, int M, int N, int K, float alpha, float beta,
                       float diag, int splits, float* ws, void* stream) {
    if (splits == 1)
        return mil_tm_bgemm(A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb, sCi, sCj, D, batch, M, N, K, alpha, beta, diag, 1, stream);
    if (!ws || !tm_bgemm_args_ok(A, B, C, batch, M, N, K, splits, 64) || !tm_bgemm_fold_ok(batch, M, N)) return MIL_EINVAL;
    dim3 grid((N + 63) / 64, (M + 63) / 64, batch * splits);
    hipLaunchKernelGGL(k_tm_bgemm<true>, grid, dim3(256), 0, (hipStream_t)stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, ws,
                       (long)M * N, (long)N, 1L, (const float*)nullptr, M, N, K, alpha, 0.f, 0.f, splits);
    tm_bgemm_fold(ws, splits, C, sCb, sCi, sCj, D, batch, M, N, beta, diag, (hipStream_t)stream);
    return launch_rc();
}

size_t mil_tm_row_gather_ws_floats(int src_rows) { return src_rows > 0 ? (size_t)3 * src_rows : 0; }

int mil_tm_row_gather_bwd_fixed(const float* ddst, const int32_t* idx, int rows, int E, float* dsrc, int src_rows, float* dextra,
                                float* ws, void* stream) {
    if (!ddst || !idx || !dsrc || !ws || rows <= 0 || E <= 0 || src_rows <= 0 || src_rows > (1 << 29)) return MIL_EINVAL;
    int32_t* meta = reinterpret_cast<int32_t*>(ws);
    hipLaunchKernelGGL(k_tm_gather_meta_zero, dim3((3 * src_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, meta, 3 * src_rows);
    hipLaunchKernelGGL(k_tm_gather_meta, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, rows, src_rows, meta);
    hipLaunchKernelGGL(k_tm_gather_bwd_fixed, dim3(src_rows + (dextra != nullptr ? 1 : 0)), dim3(256), 0, (hipStream_t)stream, ddst,
                       idx, rows, E, meta, src_rows, dsrc, dextra);
    return launch_rc();
}

size_t mil_tm_pinv_ws_floats(void) { return PINV_CHUNKS; }

int mil_tm_pinv_init_bwd_fixed(const float* dZ0, const float* Z0, const float* scale, const int32_t* arg, float* dA2, float* ws,
                               void* stream) {
    if (!dZ0 || !Z0 || !scale || !arg || !dA2 || !ws) return MIL_EINVAL;
    tm_pinv_init_bwd_launch<true>(dZ0, Z0, scale, arg, 1, dA2, ws, (hipStream_t)stream);
    return launch_rc();
}

size_t mil_tm_pinv_ws_floats_bags(int nb) { return nb >= 1 && nb <= PINV_MAX_BAGS ? (size_t)nb * PINV_CHUNKS : 0; }

int mil_tm_pinv_init_bwd_bags_fixed(const float* dZ0, const float* Z0, const float* scale, const int32_t* arg, int nb, float* dA2,
                                    float* ws, void* stream) {
    if (!dZ0 || !Z0 || !scale || !arg || !dA2 || !ws || nb < 1 || nb > PINV_MAX_BAGS) return MIL_EINVAL;
    tm_pinv_init_bwd_launch<true>(dZ0, Z0, scale, arg, nb, dA2, ws, (hipStream_t)stream);
    return launch_rc();
}

size_t mil_tm_resconv_ws_floats(int n_pad) {
    return n_pad > 0 ? (size_t)((n_pad + RC_CHUNK - 1) / RC_CHUNK) * (TM_H * TM_CONV) : 0;
}

int mil_tm_resconv_bwd_fixed(const float* dout, const float* qkv, const float* w, int n_pad, float* dqkv, float* dw, float* ws,
                             void* stream) {
    if (!dout || !qkv || !w || !dqkv || !dw || !ws || n_pad <= 0) return MIL_EINVAL;
    const int chunks = (n_pad + RC_CHUNK - 1) / RC_CHUNK;
    hipLaunchKernelGGL(k_tm_resconv_bwd_dv<false>, dim3(n_pad, 2), dim3(256), 0, (hipStream_t)stream, dout, w, n_pad, dqkv,
                       TmPackedArg<false>{});
    hipLaunchKernelGGL(k_tm_resconv_bwd_dw<true>, dim3(TM_H * TM_CONV, chunks), dim3(256), 0, (hipStream_t)stream, dout, qkv, n_pad, ws);
    tm_fold(ws, TM_H * TM_CONV, chunks, TM_H * TM_CONV, dw, (hipStream_t)stream);
    return launch_rc();
}

// ---- a step's bags as one packed sequence (csrc/tm_packed.h): the landmarks and the residual conv over all bags' rows
int mil_tm_landmarks_packed(const float* qkv, float qscale, float* qL, float* kL, const int32_t* blk_off, int nb, int total_blocks,
                            void* stream) {
    if (!qkv || !qL || !kL || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_landmarks_packed, dim3(TM_M, 4, nb), dim3(256), 0, (hipStream_t)stream, qkv, blk_off, nb, total_blocks,
                       qscale, qL, kL);
    return launch_rc();
}

int mil_tm_landmarks_bwd_packed(const float* dqL, const float* dkL, float qscale, float* dqkv, const int32_t* blk_off, int nb,
                                int total_blocks, void* stream) {
    if (!dqL || !dkL || !dqkv || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_landmarks_bwd_packed, dim3(total_blocks * TM_PACKED_BLK, 4), dim3(256), 0, (hipStream_t)stream, dqL, dkL,
                       blk_off, nb, total_blocks, qscale, dqkv);
    return launch_rc();
}

int mil_tm_resconv_packed(const float* qkv, const float* w, float* out, const int32_t* blk_off, int nb, int total_blocks,
                          void* stream) {
    if (!qkv || !w || !out || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_resconv_packed, dim3(total_blocks * TM_PACKED_BLK, 2), dim3(256), 0, (hipStream_t)stream, qkv, w, blk_off,
                       nb, total_blocks, out);
    return launch_rc();
}

// the dw kernels count the chunks in gridDim.y
inline bool tm_packed_conv_ok(const void* tab, int nb, int total_blocks) {
    return tm_packed_ok(tab, nb, total_blocks) && total_blocks <= 65535;
}

int mil_tm_resconv_bwd_packed(const float* dout, const float* qkv, const float* w, float* dqkv, float* dw, const int32_t* blk_off,
                              int nb, int total_blocks, void* stream) {
    if (!dout || !qkv || !w || !dqkv || !dw || !tm_packed_conv_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_resconv_bwd_dv<true>, dim3(total_blocks * TM_PACKED_BLK, 2), dim3(256), 0, (hipStream_t)stream, dout, w,
                       total_blocks * TM_PACKED_BLK, dqkv, TmPackedArg<true>{blk_off, nb, total_blocks});
    hipLaunchKernelGGL(k_tm_resconv_bwd_dw_packed<false>, dim3(TM_H * TM_CONV, total_blocks), dim3(256), 0, (hipStream_t)stream, dout,
                       qkv, dw, blk_off, nb, total_blocks);
    return launch_rc();
}

size_t mil_tm_resconv_packed_ws_floats(int total_blocks, int nb, int backward) {
    if (!tm_packed_conv_ok(&nb, nb, total_blocks) || !backward) return 0;
    return (size_t)total_blocks * (TM_H * TM_CONV);
}

int mil_tm_resconv_bwd_packed_fixed(const float* dout, const float* qkv, const float* w, float* dqkv, float* dw, float* ws,
                                    const int32_t* blk_off, int nb, int total_blocks, void* stream) {
    if (!dout || !qkv || !w || !dqkv || !dw || !ws || !tm_packed_conv_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tm_resconv_bwd_dv<true>, dim3(total_blocks * TM_PACKED_BLK, 2), dim3(256), 0, (hipStream_t)stream, dout, w,
                       total_blocks * TM_PACKED_BLK, dqkv, TmPackedArg<true>{blk_off, nb, total_blocks});
    hipLaunchKernelGGL(k_tm_resconv_bwd_dw_packed<true>, dim3(TM_H * TM_CONV, total_blocks), dim3(256), 0, (hipStream_t)stream, dout,
                       qkv, ws, blk_off, nb, total_blocks);
    tm_fold(ws, TM_H * TM_CONV, total_blocks, TM_H * TM_CONV, dw, (hipStream_t)stream);
    return launch_rc();
}

size_t mil_tm_ppeg_ws_floats(int s) { return s > 0 ? (size_t)((s + PPEG_ROWS - 1) / PPEG_ROWS) * (50 * TM_D) : 0; }

int mil_tm_ppeg_bwd_fixed(const float* dy, const float* x, int s, const float* W7, const float* W5, const float* W3, float* dx,
                          float* dWf, float* db, float* ws, void* stream) {
    if (!dy || !x || !W7 || !W5 || !W3 || !dx || !dWf || !db || !ws || s <= 0) return MIL_EINVAL;
    const int chunks = (s + PPEG_ROWS - 1) / PPEG_ROWS;
    hipLaunchKernelGGL(k_tm_ppeg, dim3(s, 2, (s + PPEG_COLS - 1) / PPEG_COLS), dim3(256), 0, (hipStream_t)stream, dy, s, W7, W7, W5, W5, W3, W3, 1, dx);
    hipLaunchKernelGGL(k_tm_ppeg_dw<true>, dim3((50 * TM_D + 255) / 256, chunks), dim3(256), 0, (hipStream_t)stream, dy, x, s, ws,
                       (float*)nullptr);
    tm_fold(ws, 50 * TM_D, chunks, 49 * TM_D, dWf, (hipStream_t)stream);
    tm_fold(ws + 49 * TM_D, 50 * TM_D, chunks, TM_D, db, (hipStream_t)stream);
    return launch_rc();
}

// ---- PPEG of a step's bags in one launch set (csrc/tm_ppeg_packed.h): the launch shapes come from (nb, total_rows) alone
int mil_tm_ppeg_fwd_packed(const float* x, const float* W7, const float* b7, const float* W5, const float* b5, const float* W3,
                           const float* b3, float* y, const int32_t* tab, int nb, int total_rows, void* stream) {
    if (!x || !W7 || !b7 || !W5 || !b5 || !W3 || !b3 || !y || !tm_ppeg_ok(tab, nb, total_rows)) return MIL_EINVAL;
    const TmPpegDims d = tm_ppeg_dims(nb, total_rows);
    hipLaunchKernelGGL(k_tm_ppeg_packed, dim3(d.gmax, 2, d.zmax), dim3(256), 0, (hipStream_t)stream, x, W7, b7, W5, b5, W3, b3, 0, y,
                       tab, nb, total_rows, d.gmax);
    return launch_rc();
}

int mil_tm_ppeg_bwd_packed(const float* dy, const float* x, const float* W7, const float* W5, const float* W3, float* dx,
                           float* dWf, float* db, const int32_t* tab, int nb, int total_rows, void* stream) {
    if (!dy || !x || !W7 || !W5 || !W3 || !dx || !dWf || !db || !tm_ppeg_ok(tab, nb, total_rows)) return MIL_EINVAL;
    const TmPpegDims d = tm_ppeg_dims(nb, total_rows);
    hipLaunchKernelGGL(k_tm_ppeg_packed, dim3(d.gmax, 2, d.zmax), dim3(256), 0, (hipStream_t)stream, dy, W7, W7, W5, W5, W3, W3, 1,
                       dx, tab, nb, total_rows, d.gmax);
    hipLaunchKernelGGL(k_tm_ppeg_dw_packed<false>, dim3((50 * TM_D + 255) / 256, d.cmax), dim3(256), 0, (hipStream_t)stream, dy, x,
                       dWf, db, tab, nb, total_rows, d.gmax, d.cmax);
    return launch_rc();
}

size_t mil_tm_ppeg_packed_ws_floats(int total_chunks) {
    return total_chunks >= 1 && total_chunks <= INT_MAX / (50 * TM_D) ? (size_t)total_chunks * (50 * TM_D) : 0;
}

int mil_tm_ppeg_bwd_packed_fixed(const float* dy, const float* x, const float* W7, const float* W5, const float* W3, float* dx,
                                 float* dWf, float* db, float* ws, const int32_t* tab, int nb, int total_rows, void* stream) {
    if (!dy || !x || !W7 || !W5 || !W3 || !dx || !dWf || !db || !ws || !tm_ppeg_ok(tab, nb, total_rows)) return MIL_EINVAL;
    const TmPpegDims d = tm_ppeg_dims(nb, total_rows);
    hipLaunchKernelGGL(k_tm_ppeg_packed, dim3(d.gmax, 2, d.zmax), dim3(256), 0, (hipStream_t)stream, dy, W7, W7, W5, W5, W3, W3, 1,
                       dx, tab, nb, total_rows, d.gmax);
    hipLaunchKernelGGL(k_tm_ppeg_dw_packed<true>, dim3((50 * TM_D + 255) / 256, d.cmax), dim3(256), 0, (hipStream_t)stream, dy, x, ws,
                       (float*)nullptr, tab, nb, total_rows, d.gmax, d.cmax);
    hipLaunchKernelGGL(k_tm_ppeg_fold_packed, dim3((50 * TM_D + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, tab, nb, d.cmax,
                       dWf, db);
    return launch_rc();
}

}  // extern "C"
