// Split-K reduce of the gate weight gradient, shared by the fp32 and bf16 dW kernels (included in both
// translation units: device code is not linked across them).
#pragma once
#include "mil_common.h"
#define GR_NG 384
#define GR_NB 16          // lanes per bias / w / b output in the reduce

// Transposing fragment read of a k-major bf16 LDS image (rows = k, WB_S elements apart), shared by k_gate_bwd_dw_bf16 and
// k_gate_bwd_dw2_pieces; the lane mapping and the conflict-free stride are described at k_gate_bwd_dw_bf16.
#define WB_S 160
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef unsigned short gp_u16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ gp_u16x8 tr_frag(const unsigned short* img, int row, int col) {
    // 8 consecutive rows [row, row + 8) of column (col + lane column), as one 32x32x16 operand fragment
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + row * WB_S + col));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + (row + 4) * WB_S + col));
    gp_u16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
}

// Parameter gradients of the head (model/aggregator.py:128-131: z = M Wf^T + bf):  dWf[c][j] = sum_b dz[b][c] M[b][j],
// dbf[c] = sum_b dz[b][c], plus the step's loss = sum_b loss_bag[b].  A handful of workgroups of latency-bound work that
// depends only on the fused per-bag tail: it rides at the end of the gate reduce launch (blocks >= first) instead of
// being a launch of its own.  Same arithmetic as k_head_bwd_params (head_loss.hip).
struct HeadBwdArgs {
    const float* dz;            // [B, C] or NULL (no head work in this launch)
    const float* M;             // [B, L]
    float* dWf;                 // [C, L]
    float* dbf;                 // [C]
    const float* loss_bag;      // [B] or NULL
    float* loss_out;            // [1]
    int B, L, C;
    int accumulate;             // != 0: add to dWf / dbf / loss_out (gradient accumulation over micro-batches)
    // The deferred pool (mpart != NULL, C == 2): M is formed HERE, from the sums the m == 0 workgroups of
    // k_gate_bwd_dw2_pieces_mp left in mpart [S][MP_SLOTS][MP_ROWS][L] (chunks of kc rows), and written with Mdrop (NULL in
    // eval mode: the head saw M itself); the M above is not read
    const float* mpart;
    const int32_t* tile_map;    // [T][4] of the aligned layout: tile t = rows 32 t ..
    const int32_t* bag_tile_off;
    float *M_out, *Mdrop_out;
    const uint32_t* mbits;      // [B][L/32] keep words of the head's dropout, with Mdrop_out
    float mscale, xscale;       // survivors' scales of the head's and of the patches' dropout
    int kc;
};
#define MP_SLOTS 4                      /* bags a row chunk may touch (the plan refuses the route beyond) */
#define MP_ROWS 16                      /* staging rows of k_gate_bwd_dw2_pieces: thread >> 5 */
static_assert(MP_SLOTS == MIL_POOL_DEFERRED_SLOTS, "header and kernels disagree on the slot count");

// The head's weight gradient on the deferred pool (C == 2).  Workgroup jb owns 16 columns: thread (g = tid >> 2, q = tid & 3)
// takes the bags g, g + 64, .. and the float4 column q - one bag per thread at 32 bags, so the loads of a bag's one to four
// chunks are all the thread waits for.  M_b = xscale * (sum over the row chunks the bag's rows lie in, in order, of the sixteen
// staging rows in order; slot = bag - bag of the chunk's first row), then Mdrop = M keep mscale, both stored here.
// dWf[c][j] = sum_b dz[b][c] Mhead_b[j]: per thread over its bags, then the 64 groups in order.
#define MP_HEAD_COLS 16
static __device__ __forceinline__ void head_bwd_params_mpool(const HeadBwdArgs& a, int jb, float* red, const AdamFuse& ad) {
    const int q = threadIdx.x & 3, g = threadIdx.x >> 2, j = jb * MP_HEAD_COLS + 4 * q;
    f32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
    for (int b = g; b < a.B; b += 64) {
        const int r0 = a.bag_tile_off[b] * MIL_POOL_TILE, r1 = a.bag_tile_off[b + 1] * MIL_POOL_TILE;
        f32x4 m = {0, 0, 0, 0};
        if (r1 > r0)
            for (int s = r0 / a.kc; s <= (r1 - 1) / a.kc; ++s) {
                const int slot = b - a.tile_map[4 * ((s * a.kc) / MIL_POOL_TILE)];
                if ((unsigned)slot >= MP_SLOTS) continue;
                const float* src = a.mpart + (size_t)((s * MP_SLOTS + slot) * MP_ROWS) * a.L + j;
                f32x4 u[MP_ROWS];
#pragma unroll
                for (int e = 0; e < MP_ROWS; ++e) u[e] = *reinterpret_cast<const f32x4*>(src + (size_t)e * a.L);
#pragma unroll
                for (int e = 0; e < MP_ROWS; ++e) m += u[e];
            }
        m *= a.xscale;
        f32x4 md = m;
        if (a.Mdrop_out != nullptr && a.mbits != nullptr) {
            const unsigned mm = a.mbits[(size_t)b * (a.L >> 5) + (j >> 5)] >> (j & 31);
#pragma unroll
            for (int e = 0; e < 4; ++e) md[e] = m[e] * (((mm >> e) & 1u) ? a.mscale : 0.f);
        }
        *reinterpret_cast<f32x4*>(a.M_out + (size_t)b * a.L + j) = m;
        if (a.Mdrop_out != nullptr) *reinterpret_cast<f32x4*>(a.Mdrop_out + (size_t)b * a.L + j) = md;
        v0 += a.dz[b * 2] * md;
        v1 += a.dz[b * 2 + 1] * md;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[(0 * 64 + g) * MP_HEAD_COLS + 4 * q + e] = v0[e];
        red[(1 * 64 + g) * MP_HEAD_COLS + 4 * q + e] = v1[e];
    }
    __syncthreads();
    if (threadIdx.x < 2 * MP_HEAD_COLS) {
        const int c = threadIdx.x / MP_HEAD_COLS, col = threadIdx.x % MP_HEAD_COLS;
        float* o = a.dWf + (size_t)c * a.L + jb * MP_HEAD_COLS + col;
        float t = 0.f;
#pragma unroll 8
        for (int gg = 0; gg < 64; ++gg) t += red[(c * 64 + gg) * MP_HEAD_COLS + col];
        if (a.accumulate) t += *o;
        *o = t;
        adam_fused(ad, o, t);
    }
}
static __device__ __forceinline__ void head_bwd_params_block(const HeadBwdArgs& a, int blk, float (*red)[64],   /* [32][64] */
                                                             const AdamFuse& ad) {
    const int nlb = (a.L + 63) / 64;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (a.mpart != nullptr) {            // the deferred pool: L / MP_HEAD_COLS workgroups form M and dWf, the last one dbf and the loss
        if (blk < a.L / MP_HEAD_COLS) {
            head_bwd_params_mpool(a, blk, &red[0][0], ad);
            return;
        }
        blk = a.C * nlb;
    }
    if (blk < a.C * nlb) {
        const int c = blk / nlb, j = (blk % nlb) * 64 + lane;
        float v = 0.f;
        if (j < a.L)
            for (int b0 = g; b0 < a.B; b0 += 32) {                  // eight (dz, M) pairs in flight per thread, not one
                float dzv[8], mv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int b = min(b0 + 4 * e, a.B - 1);
                    dzv[e] = a.dz[b * a.C + c];
                    mv[e] = a.M[(size_t)b * a.L + j];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v = b0 + 4 * e < a.B ? fmaf(dzv[e], mv[e], v) : v;
            }
        red[g][lane] = v;
        __syncthreads();
        if (g == 0 && j < a.L) {
            float* o = a.dWf + (size_t)c * a.L + j;
            float t = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
            if (a.accumulate) t += *o;
            *o = t;
            adam_fused(ad, o, t);
        }
    } else {
        if ((int)threadIdx.x < a.C) {
            const int c = threadIdx.x;
            float v = 0.f;
            for (int b0 = 0; b0 < a.B; b0 += 16) {
                float u[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) u[e] = a.dz[min(b0 + e, a.B - 1) * a.C + c];
#pragma unroll
                for (int e = 0; e < 16; ++e) v += b0 + e < a.B ? u[e] : 0.f;
            }
            if (a.accumulate) v += a.dbf[c];
            a.dbf[c] = v;
            adam_fused(ad, a.dbf + c, v);
        }
        if (a.loss_bag != nullptr && g == 1) {
            float v = 0.f;
            for (int b = lane; b < a.B; b += 64) v += a.loss_bag[b];
            v = wave_allsum(v);
            if (lane == 0) a.loss_out[0] = a.accumulate ? a.loss_out[0] + v : v;
        }
    }
}

// Sum the split-K partials and un-permute the gate index.  One thread per output float4.
// One thread per output float4 (8 independent 16-byte loads in flight), un-permuting the gate index; the last
// 577 threads fold the bias / w / b partials.  (A 4-threads-per-output variant with 4x the workgroups measured
// slower: 14.3 vs 12.1 us for the 31 MB of partials at L = 512.)
// SB: number of bias slabs [4][192] in pbias (S for kernels whose jt == 0 workgroups publish a chunk's sums, S * NJ for
// k_gate_bwd_dw2, where every column-tile workgroup publishes its share).
static __global__ __launch_bounds__(256) void k_gate_bwd_reduce(const float* __restrict__ part, const float* __restrict__ pbias,
                                                                int S, int SB, int L, float* __restrict__ dWv, float* __restrict__ dbv,
                                                                float* __restrict__ dWu, float* __restrict__ dbu,
                                                                float* __restrict__ dw, float* __restrict__ db, int accumulate,
                                                                float wscale, int head_first = 1 << 30,
                                                                HeadBwdArgs head = HeadBwdArgs{}, AdamFuse ad_in = AdamFuse{},
                                                                unsigned short* __restrict__ Wv16 = nullptr,
                                                                unsigned short* __restrict__ Wu16 = nullptr,
                                                                unsigned short* __restrict__ Wp = nullptr) {
    // Wv16 / Wu16 (bf16-storage step with Adam applied here): the bf16 shadows of the gate weights the forward reads are
    // refreshed by the thread that has just updated their fp32 masters - no cast launches after the update.  Wp (fp32 step
    // with Adam applied here): the same for the three-piece planes of the split-bf16 gate forward.
    __shared__ float bcs[2];
    const int L4 = L / 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nW = GR_NG * L4;
    const bool wrole = (int)blockIdx.x < head_first && idx < nW;
    // Round 4: the launch is a chain of dependent round trips (step counter -> bias corrections -> learning rate -> partials 8
    // + 8 + 5 x ONE at a time -> p, m, v).  The first 24 partials of a weight thread (every split the step's shapes produce) and
    // its Adam state are now requested BEFORE the workgroup waits for the bias corrections, the tail of the partial list as
    // one masked batch: the loads of a thread are in flight together.
    constexpr int GR_PRE = 24;
    f32x4 t[GR_PRE], pm[3];
    const int gi = wrole ? idx / L4 : 0, c4 = wrole ? idx % L4 : 0;
    const float* src = part + (size_t)gi * L + 4 * c4;
    const size_t stride = (size_t)GR_NG * L;
    const int mm_ = gi >> 7, ii = gi & 127;
    const size_t woff = (size_t)(ii < 64 ? 64 * mm_ + ii : 64 * mm_ + ii - 64) * L + 4 * c4;
    float* dst = (ii < 64 ? dWv : dWu) + woff;
    if (wrole) {
#pragma unroll
        for (int e = 0; e < GR_PRE; ++e) t[e] = *reinterpret_cast<const f32x4*>(src + (size_t)min(e, S - 1) * stride);
        if (ad_in.param != nullptr) {
            const size_t i = (size_t)(dst - ad_in.grad_base);
            pm[0] = *reinterpret_cast<const f32x4*>(ad_in.param + i);
            pm[1] = *reinterpret_cast<const f32x4*>(ad_in.m + i);
            pm[2] = *reinterpret_cast<const f32x4*>(ad_in.v + i);
        }
    }
    const AdamFuse ad = adam_fuse_resolve(ad_in, bcs);
    if ((int)blockIdx.x >= head_first) {          // appended workgroups: the head's parameter gradients (uniform branch)
        __shared__ float hred[32][64];      // [4][64] of head_bwd_params_block, [2][64][16] of head_bwd_params_mpool
        head_bwd_params_block(head, blockIdx.x - head_first, hred, ad);
        return;
    }
    if (idx < nW) {
        f32x4 v = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < GR_PRE; ++e) v += e < S ? t[e] : f32x4{0, 0, 0, 0};
        for (int s = GR_PRE; s < S; s += 8) {       // longer splits: masked batches of eight
            f32x4 u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = *reinterpret_cast<const f32x4*>(src + (size_t)min(s + e, S - 1) * stride);
#pragma unroll
            for (int e = 0; e < 8; ++e) v += s + e < S ? u[e] : f32x4{0, 0, 0, 0};
        }
        v *= wscale;             // train mode: the 1/(1-p) of the patch dropout (x entered the product as keep-masked x)
        if (accumulate) v += *reinterpret_cast<const f32x4*>(dst);
        *reinterpret_cast<f32x4*>(dst) = v;
        f32x4 pnew = v;
        if (ad.param != nullptr) {                 // adam_fused4 on the prefetched state
            const size_t i = (size_t)(dst - ad.grad_base);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pm[0][e], me = pm[1][e], ve = pm[2][e];
                adam_one(pe, v[e], me, ve, ad.lr_bc1, ad.b1, ad.b2, ad.eps, ad.wd, ad.gscale, ad.bc2_sqrt);
                pm[0][e] = pe; pm[1][e] = me; pm[2][e] = ve;
            }
            *reinterpret_cast<f32x4*>(ad.param + i) = pm[0];
            *reinterpret_cast<f32x4*>(ad.m + i) = pm[1];
            *reinterpret_cast<f32x4*>(ad.v + i) = pm[2];
            pnew = pm[0];
        }
        if (Wv16 != nullptr && ad.param != nullptr) {
            ushort4 o;                                  // the conversion k_cast_bf16 uses (round to nearest even)
            o.x = __builtin_bit_cast(unsigned short, (__bf16)pnew[0]);
            o.y = __builtin_bit_cast(unsigned short, (__bf16)pnew[1]);
            o.z = __builtin_bit_cast(unsigned short, (__bf16)pnew[2]);
            o.w = __builtin_bit_cast(unsigned short, (__bf16)pnew[3]);
            *reinterpret_cast<ushort4*>((ii < 64 ? Wv16 : Wu16) + woff) = o;
        }
        if (Wp != nullptr && ad.param != nullptr)
            gp_store4(Wp, (ii < 64 ? 0 : MIL_GATE_D) + (int)(woff / L), 4 * c4, pnew);
    } else if (idx < nW + GR_NB * (3 * 192 + 1)) {
        // bias / w / b: GR_NB lanes per output, each sums every GR_NB-th slab (loads in flight), then a fixed-order
        // shuffle fold.  (One thread per output walked the S * NJ slabs of the low-VALU kernel serially: 9.5 us.)
        const int k = (idx - nW) / GR_NB, sub = (idx - nW) % GR_NB;
        const int which = k / 192, d = k % 192;
        float v = 0.f;
        for (int s0 = sub; s0 < SB; s0 += 8 * GR_NB) {              // eight slabs in flight per lane (they were one at a time)
            float u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = pbias[((size_t)min(s0 + e * GR_NB, SB - 1) * 4 + which) * 192 + d];
#pragma unroll
            for (int e = 0; e < 8; ++e) v += s0 + e * GR_NB < SB ? u[e] : 0.f;
        }
#pragma unroll
        for (int mm = GR_NB / 2; mm >= 1; mm >>= 1) v += __shfl_xor(v, mm);
        if (sub != 0) return;
        float* dst = which == 0 ? dbv + d : which == 1 ? dbu + d : which == 2 ? dw + d : db;
        if (accumulate) v += *dst;
        *dst = v;
        adam_fused(ad, dst, v);
    }
}

// ---- host side: the one place that launches the fold
// SB as above.  head (nullable): the head's parameter gradients and the loss as appended workgroups; ad (nullable): Adam
// on the spot, with the bf16 shadows Wv16 / Wu16 or the weight pieces Wp of the gate weights rewritten by the same threads.
static inline int launch_gate_bwd_reduce(const float* part, const float* pbias, int S, int SB, int L, float* dWv, float* dbv,
                                         float* dWu, float* dbu, float* dw, float* db, int accumulate, float wscale,
                                         hipStream_t st, const HeadBwdArgs* head = nullptr, const AdamFuse* ad = nullptr,
                                         uint16_t* Wv16 = nullptr, uint16_t* Wu16 = nullptr, uint16_t* Wp = nullptr) {
    const int nthreads = GR_NG * (L / 4) + GR_NB * (3 * 192 + 1);
    const int nred = (nthreads + 255) / 256;
    const int nhead = !head ? 0 : head->mpart ? head->L / MP_HEAD_COLS + 1 : head->C * ((head->L + 63) / 64) + 1;
    hipLaunchKernelGGL(k_gate_bwd_reduce, dim3(nred + nhead), dim3(256), 0, st, part, pbias, S, SB, L, dWv, dbv, dWu, dbu, dw, db,
                       accumulate, wscale, head ? nred : 1 << 30, head ? *head : HeadBwdArgs{}, ad ? *ad : AdamFuse{},
                       (unsigned short*)Wv16, (unsigned short*)Wu16, (unsigned short*)Wp);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// The AdamFuse of a fold launch that updates the parameters it has the gradients of: every gradient must lie inside the
// flat buffer (16-byte aligned where it is stored as float4), and `step` >= 1 is the update's number unless a device
// counter (step_dev) carries it.  MIL_EINVAL otherwise.
static inline int gate_adam_fuse(const float* dWv, const float* dbv, const float* dWu, const float* dbu, const float* dw,
                                 const float* db, const HeadBwdArgs& head, float* param_flat, const float* grad_flat,
                                 size_t n_param, float* exp_avg, float* exp_avg_sq, int step, const int* step_dev, float lr,
                                 const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                 int* done, AdamFuse* out) {
    if (!param_flat || !grad_flat || !exp_avg || !exp_avg_sq || (step_dev == nullptr && step < 1)) return MIL_EINVAL;
    const float* outs[8] = {dWv, dbv, dWu, dbu, dw, db, head.dWf, head.dbf};
    const size_t lens[8] = {(size_t)192 * head.L, 192, (size_t)192 * head.L, 192, 192, 1, (size_t)head.C * head.L, (size_t)head.C};
    for (int i = 0; i < 8; ++i)
        if (outs[i] < grad_flat || outs[i] + lens[i] > grad_flat + n_param) return MIL_EINVAL;
    if (((dWv - grad_flat) | (dWu - grad_flat)) & 3) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param_flat) | reinterpret_cast<uintptr_t>(grad_flat) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    if (step_dev != nullptr) step = 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    // the kernel forms the same single-precision quotient k_adam forms (lr / (float)bc1): the two routes stay bit-identical
    *out = AdamFuse{param_flat, grad_flat, exp_avg, exp_avg_sq, (float)bc1, beta1, beta2, eps, weight_decay, grad_scale,
                    (float)sqrt(bc2), step_dev, lr, lr_dev, step_dev ? done : nullptr};
    return MIL_OK;
}
