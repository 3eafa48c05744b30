// K3a, token side: nn.Linear on a handful of rows (M <= 64: one text token per bag, model/aggregator.py:44-68,
// model/sam/transformer.py:413-416 and sam/common.py:21-26 applied to the [B*T, 512] query stream).
// These products are latency-bound (a 512 x 512 weight is read once for 32 rows), so the tiled 128 x 128 GEMM of
// linear.hip wastes its launch on 1-4 workgroups walking all of K.  Here the output is cut into 16 x 16 tiles
// (v_mfma_f32_16x16x4_f32), one workgroup each, so even a [32, 512] result spreads over 64 CUs:
//   k_small_fwd   workgroup = one 16 x 16 tile of y; its waves split K, operands go global -> registers (16-byte
//                 loads along k, the k-permutation feeding 4 MFMAs per load, a whole trip of loads issued before the
//                 first MFMA), the partial tiles are folded through LDS and the bias / activation / residual epilogue
//                 is applied in the same launch.
//   k_small_bwd   ONE launch for the whole backward of the layer: workgroups [0, nW) form dW = dpre^T x (32 x 32
//                 tiles, contraction over the few rows) and the bias gradient, workgroups [nW, nW + nX) form
//                 dx = dpre W in 16 x 16 tiles; dpre = dy * act'(.) is evaluated on the fly, so no activation-backward
//                 pass, no column-sum pass and no split-K reduce exist.
// fp32 MFMA rounds like an fmaf chain, so results match the tiled path to accumulation order.
#include "mil_common.h"

#define SL_WAVES 8         // waves per workgroup; SL_WAVES_DEEP for contractions >= 1024
#define SL_WAVES_DEEP 16
enum { SL_NONE = 0, SL_TANH = 1, SL_RELU = 2, SL_QUICKGELU = 3, SL_SIGMOID = 4 };

__device__ __forceinline__ float sl_act(float v, int act) {
    if (act == SL_TANH) return tanhf(v);
    if (act == SL_RELU) return fmaxf(v, 0.f);
    if (act == SL_QUICKGELU) return v / (1.0f + expf(-1.702f * v));
    if (act == SL_SIGMOID) return 1.0f / (1.0f + expf(-v));
    return v;
}
// dy * act'(.), from the activation OUTPUT for tanh / relu / sigmoid and from the PRE-activation for QuickGELU
__device__ __forceinline__ float sl_dact(float g, float yv, int act) {
    if (act == SL_TANH) return g * (1.0f - yv * yv);
    if (act == SL_RELU) return yv > 0.f ? g : 0.f;
    if (act == SL_QUICKGELU) {
        const float s = 1.0f / (1.0f + expf(-1.702f * yv));
        return g * s * (1.0f + 1.702f * yv * (1.0f - s));
    }
    if (act == SL_SIGMOID) return g * yv * (1.0f - yv);
    return g;
}

// Fold the waves' 16 x 16 partial tiles (lane l holds column l & 15 of rows 4 (l >> 4) + i) and store with epilogue.
// The epilogue's two operands (bias and residual of the thread's output element) are fetched by sl_epi_prefetch at the START
// of the kernel: loaded after the last barrier they were one more exposed L2 round trip per launch of the token-side chain.
struct SlEpi {
    float b, r;
};
__device__ __forceinline__ SlEpi sl_epi_prefetch(int tid, int M, int N, int m0, int n0, const float* __restrict__ bias,
                                                 const float* __restrict__ residual, int ldr) {
    SlEpi e{0.f, 0.f};
    if (tid < 256) {
        const int i = tid >> 6, l = tid & 63;
        const int row = m0 + 4 * (l >> 4) + i, col = n0 + (l & 15);
        if (row < M && col < N) {
            if (bias != nullptr) e.b = bias[col];
            if (residual != nullptr) e.r = residual[(size_t)row * ldr + col];
        }
    }
    return e;
}
template <int NW>
__device__ __forceinline__ void sl_fold_store(float (*red)[4][64], const f32x4 acc, int tid, int M, int N, int m0, int n0,
                                              const SlEpi epi, int act, float* __restrict__ out, int ldo) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    if (tid < 256) {
        const int i = tid >> 6, l = tid & 63;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += red[w][i][l];
        const int row = m0 + 4 * (l >> 4) + i, col = n0 + (l & 15);
        if (row < M && col < N) out[(size_t)row * ldo + col] = sl_act(v + epi.b, act) + epi.r;
    }
}

// Operands through LDS (round 2).  The first form loaded them "global -> registers" in the MFMA's own layout: lane (r, kq)
// took 16 bytes of ITS row, so every quarter-wave touched 16 different rows - 64 cache-line look-ups per load instruction
// where a contiguous 1 KB needs 8 - and a wave with fewer than 8 chunks of K re-issued its last chunk to fill the trip:
// for a 512-deep layer 16 such instructions per wave, ~3.4 us of L1 tag time per workgroup out of a 6.4 us kernel
// (the same finding as k_apool_dots).  Now the workgroup loads both 16-row operand slabs with contiguous 1 KB wave
// instructions, K in chunks of 512 (the next chunk's loads in flight under this chunk's MFMAs), stages them in LDS (row
// stride 516 floats: the 16 lanes of a fragment read hit 64 different banks) and the waves split the chunk's 16-k blocks.
#define SL_KCH 512
#define SL_LS (SL_KCH + 4)
// x2 / xin (round 4, both or neither): the layer's input is x + x2 (queries + their positional embedding,
// sam/transformer.py:114) - added while the operand is staged, and written once (column tile 0) to xin [M, K] for the weight
// gradient: the elementwise add launch in front of the layer is gone.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_small_fwd(const float* __restrict__ x, int ldx, const float* __restrict__ W,
                                                       int ldw, const float* __restrict__ bias, int act,
                                                       const float* __restrict__ residual, int ldr,
                                                       float* __restrict__ y, int ldy, int M, int N, int K,
                                                       const float* __restrict__ x2, int ldx2, float* __restrict__ xin) {
    __shared__ float red[NW][4][64];
    __shared__ __attribute__((aligned(16))) float opx[16 * SL_LS], opw[16 * SL_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    constexpr int NT = 64 * NW, LPT = (16 * SL_KCH / 4) / NT;          // 16-byte loads per thread, operand and chunk
    const SlEpi epi = sl_epi_prefetch(tid, M, N, m0, n0, bias, residual, ldr);
    f32x4 rx[LPT], rw[LPT];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + i * NT, row = idx >> 7, kk = k0 + 4 * (idx & 127);
            if (kk < K) {
                rx[i] = *reinterpret_cast<const f32x4*>(x + (size_t)min(m0 + row, M - 1) * ldx + kk);
                if (x2 != nullptr) {
                    rx[i] += *reinterpret_cast<const f32x4*>(x2 + (size_t)min(m0 + row, M - 1) * ldx2 + kk);
                    if (blockIdx.x == 0 && m0 + row < M) *reinterpret_cast<f32x4*>(xin + (size_t)(m0 + row) * K + kk) = rx[i];
                }
                rw[i] = *reinterpret_cast<const f32x4*>(W + (size_t)min(n0 + row, N - 1) * ldw + kk);
            } else {
                rx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                rw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    gload(0);
    for (int k0 = 0; k0 < K; k0 += SL_KCH) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + i * NT, row = idx >> 7, c = idx & 127;
            *reinterpret_cast<f32x4*>(opx + row * SL_LS + 4 * c) = rx[i];
            *reinterpret_cast<f32x4*>(opw + row * SL_LS + 4 * c) = rw[i];
        }
        __syncthreads();
        if (k0 + SL_KCH < K) gload(k0 + SL_KCH);
        const int nblk = min(SL_KCH, K - k0) >> 4, per = (nblk + NW - 1) / NW;
        const int b1 = min(nblk, (wave + 1) * per);
        for (int blk = wave * per; blk < b1; ++blk) {
            const f32x4 fa = *reinterpret_cast<const f32x4*>(opx + r * SL_LS + 16 * blk + 4 * kq);
            const f32x4 fb = *reinterpret_cast<const f32x4*>(opw + r * SL_LS + 16 * blk + 4 * kq);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[jj], fb[jj], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    sl_fold_store<NW>(red, acc, tid, M, N, m0, n0, epi, act, y, ldy);
}

// The gradient of a layer's output that SEVERAL consumers wrote (round 4): dy + dy2 + dy3 + dy4 (each [M, N] contiguous,
// nullable) summed while the operand is staged - autograd's elementwise add launches between the token-side layers are gone
// (ops.fan_out) - and written once to dysum [M, N] (nullable) for the deferred weight-gradient launch.
// EX = true: the extras are loaded UNCONDITIONALLY (a missing one points at dy with weight 0) - a branch per addend made
// every staged load wait for the one before it (+1.5 us per launch, measured on the launches that have no extras at all).
struct SmallDyExtra {
    const float* dy2;
    const float* dy3;
    const float* dy4;
    float w2, w3, w4;
    float* dysum;
};
// The dW role, shared by k_small_bwd (workgroups [0, nW)) and k_small_dw_grouped: dW[n][k] = sum_m dpre[m][n] x[m][k] on a
// 64 (n) x 128 (k) tile per workgroup of 8 waves, one 32 x 32 MFMA tile per wave, + the bias gradient (kt == 0).
struct SlDwArgs {
    const float* dy;
    const float* yv;
    const float* x;
    float* dW;
    float* db;
    int lddy, ldyv, ldx, lddw, act, M, N, K;
};
template <bool EX>
__device__ __forceinline__ void sl_dw_role(const SlDwArgs& d, const int wg, const SmallDyExtra& ex) {
    const int M = d.M, N = d.N, K = d.K, act = d.act;
    const int nKt = (K + 127) / 128;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int kt = wg % nKt, nt = wg / nKt;
    const int wn = wave >> 2, wk = wave & 3;
    const int n = 64 * nt + 32 * wn + r, k = 128 * kt + 32 * wk + r;
    const int nc = min(n, N - 1), kc = min(k, K - 1);
    const float* __restrict__ dy = d.dy;
    const float* __restrict__ yv = d.yv;
    const float* __restrict__ x = d.x;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float bsum = 0.f;
    const __amdgpu_buffer_rsrc_t srd_dy = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, ((M - 1) * d.lddy + N) * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_x = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, ((M - 1) * d.ldx + K) * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_yv =
        __builtin_amdgcn_make_buffer_rsrc((void*)(yv != nullptr ? yv : dy), 0, ((M - 1) * d.ldyv + N) * 4, MIL_SRD_FLAGS);
    const int voff_dy = 4 * (h * d.lddy + nc), voff_x = 4 * (h * d.ldx + kc), voff_yv = 4 * (h * d.ldyv + nc);
    const int voff_ex = 4 * (h * N + nc);
    const __amdgpu_buffer_rsrc_t srd_e2 = __builtin_amdgcn_make_buffer_rsrc((void*)(EX ? ex.dy2 : dy), 0, M * N * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_e3 = __builtin_amdgcn_make_buffer_rsrc((void*)(EX ? ex.dy3 : dy), 0, M * N * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_e4 = __builtin_amdgcn_make_buffer_rsrc((void*)(EX ? ex.dy4 : dy), 0, M * N * 4, MIL_SRD_FLAGS);
    const int steps = (M + 1) >> 1;
    for (int s0 = 0; s0 < steps; s0 += 16) {
        // every load of the trip first, unconditionally (clamped rows, masked afterwards), THEN the activation derivative under
        // one wave-uniform switch: with the per-element `if (act ..)` / `m < M` forms the compiler emitted a load - wait -
        // compute sequence per u, 16 dependent L2 round trips per workgroup (8.4 us for ONE 512 x 512 layer, 30 us for the 19
        // layers of the fusion step against 7 us of write time)
        // Buffer loads: ONE address register per operand (lane part: row parity h and the column; the row pair of trip u is a
        // scalar offset), rows >= M read as zero through the resource's bounds check - 64-bit addresses per load held the kernel
        // at 145 VGPRs = one workgroup per CU.
        float fa[16], fb[16], yy[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            fa[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_dy, voff_dy, 8 * (s0 + u) * d.lddy, 0));
            if (EX) {            // the other consumers' gradients ([M, N] contiguous; a missing one: dy again with weight 0)
                const float e2 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_e2, voff_ex, 8 * (s0 + u) * N, 0));
                const float e3 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_e3, voff_ex, 8 * (s0 + u) * N, 0));
                const float e4 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_e4, voff_ex, 8 * (s0 + u) * N, 0));
                fa[u] += ex.w2 * e2 + ex.w3 * e3 + ex.w4 * e4;
            }
            fb[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_x, voff_x, 8 * (s0 + u) * d.ldx, 0));
        }
        if (act != SL_NONE) {
#pragma unroll
            for (int u = 0; u < 16; ++u)
                yy[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd_yv, voff_yv, 8 * (s0 + u) * d.ldyv, 0));
            switch (act) {
            case SL_TANH:
#pragma unroll
                for (int u = 0; u < 16; ++u) fa[u] *= 1.0f - yy[u] * yy[u];
                break;
            case SL_RELU:
#pragma unroll
                for (int u = 0; u < 16; ++u) fa[u] = yy[u] > 0.f ? fa[u] : 0.f;
                break;
            case SL_SIGMOID:
#pragma unroll
                for (int u = 0; u < 16; ++u) fa[u] *= yy[u] * (1.0f - yy[u]);
                break;
            default:
#pragma unroll
                for (int u = 0; u < 16; ++u) fa[u] = sl_dact(fa[u], yy[u], SL_QUICKGELU);
                break;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            bsum += fa[u];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[u], fb[u], acc, 0, 0, 0);
        }
    }
    if (d.dW != nullptr && k < K) {
        // buffer stores: lane part (column k, the half's 4 rows) in one register, the register's row as a scalar offset; rows
        // >= N fall outside the resource and are dropped by the bounds check
        const int nbase = 64 * nt + 32 * wn;
        const __amdgpu_buffer_rsrc_t srd_w = __builtin_amdgcn_make_buffer_rsrc((void*)d.dW, 0, ((N - 1) * d.lddw + K) * 4, MIL_SRD_FLAGS);
        const int voff_w = 4 * ((nbase + 4 * h) * d.lddw + k);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float v = acc[i];
            asm volatile("" : "+v"(v));          // (hipcc 7.2 stored register 0 of the accumulator sixteen times without this)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), srd_w, voff_w, 4 * ((i & 3) + 8 * (i >> 2)) * d.lddw, 0);
        }
    }
    if (d.db != nullptr && kt == 0 && wk == 0) {
        const float tot = bsum + __shfl_xor(bsum, 32);
        if (h == 0 && n < N) d.db[n] = tot;
    }
}

template <int NW, bool EX>
__global__ __launch_bounds__(64 * NW) void k_small_bwd(const float* __restrict__ dy, int lddy, const float* __restrict__ yv,
                                                       int ldyv, int act, const float* __restrict__ x, int ldx,
                                                       const float* __restrict__ W, int ldw, float* __restrict__ dx,
                                                       int lddx, float* __restrict__ dW, int lddw, float* __restrict__ db,
                                                       int M, int N, int K, int nW, int nKt, SmallDyExtra ex) {
    __shared__ float red[NW][4][64];
    __shared__ __attribute__((aligned(16))) float opa[16 * SL_LS];       // dx role: dpre of the tile's 16 rows, one n chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x < nW) {
        // ---- dW[n][k] = sum_m dpre[m][n] x[m][k]: 64 (n) x 128 (k) per workgroup, one 32 x 32 tile per wave (0..7)
        if (wave >= 8 || blockIdx.y != 0) return;
        const SlDwArgs d{dy, yv, x, dW, db, lddy, ldyv, ldx, lddw, act, M, N, K};
        sl_dw_role<EX>(d, (int)blockIdx.x, ex);
        return;
    }
    // ---- dx[m][k] = sum_n dpre[m][n] W[n][k]: one 16 x 16 tile per workgroup, the waves split n.  dpre = dy * act'(.) of
    // the tile's 16 rows is formed ONCE per workgroup from contiguous 1 KB wave loads and staged in LDS, n in chunks of 512
    // (as k_small_fwd: in the MFMA's own layout a quarter-wave touched 16 rows per load instruction); the W^T operand is
    // strided by nature (64 bytes per row of W) and stays on direct loads, all of a wave's blocks issued up front.
    const int r = lane & 15, kq = lane >> 4;
    const int bx = (int)blockIdx.x - nW;
    const int nK16 = (K + 15) >> 4;
    const int k0 = (bx % nK16) * 16, m0 = (bx / nK16) * 16;
    const int kc = min(k0 + r, K - 1);
    constexpr int NT = 64 * NW, LPT = (16 * SL_KCH / 4) / NT, MAXPER = (SL_KCH / 16 + NW - 1) / NW;
    f32x4 rg[LPT], ry[LPT];
    auto gload = [&](int n0c) {
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + i * NT, row = idx >> 7, nn = n0c + 4 * (idx & 127);
            const int mrow = min(m0 + row, M - 1);
            if (nn < N) {
                rg[i] = *reinterpret_cast<const f32x4*>(dy + (size_t)mrow * lddy + nn);
                if (EX) {
                    const f32x4 e2 = *reinterpret_cast<const f32x4*>(ex.dy2 + (size_t)mrow * N + nn);
                    const f32x4 e3 = *reinterpret_cast<const f32x4*>(ex.dy3 + (size_t)mrow * N + nn);
                    const f32x4 e4 = *reinterpret_cast<const f32x4*>(ex.dy4 + (size_t)mrow * N + nn);
                    rg[i] += ex.w2 * e2 + ex.w3 * e3 + ex.w4 * e4;
                }
                if (act != SL_NONE) ry[i] = *reinterpret_cast<const f32x4*>(yv + (size_t)mrow * ldyv + nn);
            } else {
                rg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                ry[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    // gridDim.y > 1 (mil_linear_small_bwd_split): workgroup (.., s) contracts over n in [s N / S, (s + 1) N / S) only and writes
    // the partial dx_s - the contraction of a 2048-wide layer (mlp.lin1) was a 17 us walk of four operand chunks per workgroup
    // on 64 workgroups; the partials are summed by the next backward kernel while it stages them (mil_linear_small_ln_bwd5)
    const int nsl = N / (int)gridDim.y, nbeg = (int)blockIdx.y * nsl, nend = nbeg + nsl;
    dx += (size_t)blockIdx.y * M * lddx;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    gload(nbeg);
    for (int n0c = nbeg; n0c < nend; n0c += SL_KCH) {
        // the chunk's W^T fragments are requested BEFORE the staging barrier (they depend on nothing in LDS): behind it they
        // were a second exposed L2 round trip per launch
        const int nblk = min(SL_KCH, nend - n0c) >> 4, per = (nblk + NW - 1) / NW;
        const int b0 = wave * per, b1 = min(nblk, b0 + per);
        float fb[MAXPER][4];
#pragma unroll
        for (int u = 0; u < MAXPER; ++u) {
            const int nb = n0c + 16 * min(b0 + u, max(b1 - 1, 0)) + 4 * kq;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) fb[u][jj] = W[(size_t)(nb + jj) * ldw + kc];      // clamped block: unused where b0 + u >= b1
        }
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int idx = tid + i * NT, row = idx >> 7, c = idx & 127;
            f32x4 g = rg[i];
            if (EX && ex.dysum != nullptr && k0 == 0 && m0 + row < M && n0c + 4 * c < N)
                *reinterpret_cast<f32x4*>(ex.dysum + (size_t)(m0 + row) * N + n0c + 4 * c) = g;      // the summed dy, before act'
            switch (act) {              // wave-uniform: one branch per 16-byte piece, not one per element and activation
            case SL_NONE: break;
            case SL_TANH: g = g * (1.0f - ry[i] * ry[i]); break;
            case SL_RELU:
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) g[jj] = ry[i][jj] > 0.f ? g[jj] : 0.f;
                break;
            case SL_SIGMOID: g = g * ry[i] * (1.0f - ry[i]); break;
            default:
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) g[jj] = sl_dact(g[jj], ry[i][jj], SL_QUICKGELU);
                break;
            }
            *reinterpret_cast<f32x4*>(opa + row * SL_LS + 4 * c) = g;
        }
        __syncthreads();
        if (n0c + SL_KCH < nend) gload(n0c + SL_KCH);
#pragma unroll
        for (int u = 0; u < MAXPER; ++u) {
            if (b0 + u < b1) {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(opa + r * SL_LS + 16 * (b0 + u) + 4 * kq);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[jj], fb[u][jj], acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    sl_fold_store<NW>(red, acc, tid, M, K, m0, k0, SlEpi{0.f, 0.f}, SL_NONE, dx, lddx);
}

// ---------------------------------------------------------------------------------------------- LayerNorm folded into its neighbours
// The token stream of the two-way block is a string of dependent launches, P -> LayerNorm -> C (sam/transformer.py:287-300:
// out_proj -> norm -> next projection), each ~4 us whatever it computes.  Two kernels remove the LayerNorm launches of both
// directions (E = 512 = one operand chunk):
//   k_small_fwd_ln   C's forward with the norm applied while its x operand is staged:  xn = LN(u) gamma + beta,
//                    xin = xn + x2 (optional second addend: queries + query_pe), y = act(xin W^T + b) + residual.
//                    Every workgroup normalises its 16 rows redundantly (it loads them whole anyway: the contraction runs
//                    over the norm's width); the workgroups of column tile 0 write xn, xin and the row statistics.
//   k_small_bwd_ln   P's input gradient with the norm's BACKWARD applied while its dy operand is staged: the gradient that
//                    reaches the norm's output is g1 + g2 (C's dx plus whatever the output's other consumer sent - no add
//                    launch), du = rstd (g - mean(g) - xhat mean(g xhat)), g = (g1 + g2) gamma, dx = du W_P; the
//                    workgroups of k tile 0 write du (the residual branch's gradient and the dy of P's deferred weight
//                    gradient), one extra workgroup forms dgamma / dbeta over the <= 64 rows.
#define SLN_E 512
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_small_fwd_ln(const float* __restrict__ u, int ldu, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          const float* __restrict__ x2, int ldx2,
                                                          const float* __restrict__ W, int ldw, const float* __restrict__ bias,
                                                          int act, const float* __restrict__ residual, int ldr,
                                                          float* __restrict__ y, int ldy, float* __restrict__ xn,
                                                          float* __restrict__ xin, float* __restrict__ stats, int M, int N) {
    static_assert(NW == 8, "16 rows x 32 threads");
    __shared__ float red[NW][4][64];
    __shared__ __attribute__((aligned(16))) float opx[16 * SL_LS], opw[16 * SL_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    constexpr int K = SLN_E, NT = 64 * NW, LPT = (16 * SL_KCH / 4) / NT;
    const SlEpi epi = sl_epi_prefetch(tid, M, N, m0, n0, bias, residual, ldr);
    // the norm's own operands (gamma, beta, the second addend) requested with the staging loads, not behind the first barrier
    f32x4 pg[4], pbt[4], px2[4];
    {
        const int p = tid & 31, grow = m0 + (tid >> 5);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * p + 128 * j;
            pg[j] = *reinterpret_cast<const f32x4*>(gamma + c);
            pbt[j] = *reinterpret_cast<const f32x4*>(beta + c);
            px2[j] = x2 != nullptr ? *reinterpret_cast<const f32x4*>(x2 + (size_t)min(grow, M - 1) * ldx2 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
        const int idx = tid + i * NT, row = idx >> 7, c = idx & 127;
        *reinterpret_cast<f32x4*>(opx + row * SL_LS + 4 * c) =
            *reinterpret_cast<const f32x4*>(u + (size_t)min(m0 + row, M - 1) * ldu + 4 * c);
        *reinterpret_cast<f32x4*>(opw + row * SL_LS + 4 * c) =
            *reinterpret_cast<const f32x4*>(W + (size_t)min(n0 + row, N - 1) * ldw + 4 * c);
    }
    __syncthreads();
    {
        // row (tid >> 5) by its 32 threads: columns 4 p + 128 j
        const int row = tid >> 5, p = tid & 31, grow = m0 + row;
        f32x4 v[4];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = *reinterpret_cast<const f32x4*>(opx + row * SL_LS + 4 * p + 128 * j);
            s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        float mean = s / K;
        // The float32 sum of 512 values near m is off by a few ulp(512 m) / 512: for rows of mean 30 and std 1 that alone cost
        // 1e-6 of xn (16 x what the float32 restatement loses).  u - mean is (nearly) exact, so the mean of the differences is
        // what the sum lost: one more reduction puts the centred row and the stored mean right to the last bit or two.
        float sc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = v[j] - mean;
            sc += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) sc += __shfl_xor(sc, m);
        const float corr = sc / K;
        mean += corr;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = v[j] - corr;
            const f32x4 q = v[j] * v[j];
            ss += (q[0] + q[1]) + (q[2] + q[3]);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) ss += __shfl_xor(ss, m);
        const float rstd = 1.0f / sqrtf(ss / K + eps);
        const bool wr = blockIdx.x == 0 && grow < M;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * p + 128 * j;
            f32x4 o = v[j] * rstd * pg[j] + pbt[j];
            if (wr) *reinterpret_cast<f32x4*>(xn + (size_t)grow * K + c) = o;
            if (x2 != nullptr) {
                o += px2[j];
                if (wr) *reinterpret_cast<f32x4*>(xin + (size_t)grow * K + c) = o;
            }
            *reinterpret_cast<f32x4*>(opx + row * SL_LS + c) = o;
        }
        if (wr && p == 0) { stats[2 * grow] = mean; stats[2 * grow + 1] = rstd; }
    }
    __syncthreads();
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    constexpr int per = (K / 16) / NW;
    for (int blk = wave * per; blk < (wave + 1) * per; ++blk) {
        const f32x4 fa = *reinterpret_cast<const f32x4*>(opx + r * SL_LS + 16 * blk + 4 * kq);
        const f32x4 fb = *reinterpret_cast<const f32x4*>(opw + r * SL_LS + 16 * blk + 4 * kq);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[jj], fb[jj], acc, 0, 0, 0);
    }
    sl_fold_store<NW>(red, acc, tid, M, N, m0, n0, epi, act, y, ldy);
}

struct SmallLnMore {          // addends four and five of the gradient at the norm's output ([M, 512] contiguous; weight 0: absent)
    const float* g4;
    const float* g5;
    float w4, w5;
};
template <int NW, bool MORE>
__global__ __launch_bounds__(64 * NW) void k_small_bwd_ln(const float* __restrict__ g1, int ldg1, const float* __restrict__ g2,
                                                          int ldg2, const float* __restrict__ g3, int ldg3, float w2, float w3,
                                                          SmallLnMore mo, const float* __restrict__ u, int ldu,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ W, int ldw, float* __restrict__ dx,
                                                          int lddx, float* __restrict__ du, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, int M, int K, int nX) {
    static_assert(NW == 8, "16 rows x 32 threads");
    __shared__ float red[NW][4][64];
    __shared__ __attribute__((aligned(16))) float opa[16 * SL_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int N = SLN_E;
    if ((int)blockIdx.x >= nX) {
        // dgamma[c] = sum_m g[m][c] xhat[m][c], dbeta[c] = sum_m g[m][c].  Four workgroups of 128 columns; thread (column,
        // row group q) takes rows q, q + 4, ... with eight rows' loads in flight (one thread per column walking the rows in
        // turn was a chain of up to 64 dependent round trips: 5 us of a 9 us launch), folded through LDS in group order.
        float* fold = &red[0][0][0];                           // [2][3][128]
        const int c = 128 * ((int)blockIdx.x - nX) + (tid & 127), q = tid >> 7;
        float dg = 0.f, db = 0.f;
        for (int mb = q; mb < M; mb += 32) {
            float gv[8], uv[8], mu[8], rs[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int m = min(mb + 4 * e, M - 1);
                gv[e] = g1[(size_t)m * ldg1 + c];
                gv[e] += w2 * g2[(size_t)m * ldg2 + c] + w3 * g3[(size_t)m * ldg3 + c];
                if (MORE) gv[e] += mo.w4 * mo.g4[(size_t)m * N + c] + mo.w5 * mo.g5[(size_t)m * N + c];
                uv[e] = u[(size_t)m * ldu + c];
                mu[e] = stats[2 * m];
                rs[e] = stats[2 * m + 1];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (mb + 4 * e < M) { dg += gv[e] * ((uv[e] - mu[e]) * rs[e]); db += gv[e]; }
        }
        if (q > 0) { fold[((q - 1) * 2 + 0) * 128 + (tid & 127)] = dg; fold[((q - 1) * 2 + 1) * 128 + (tid & 127)] = db; }
        __syncthreads();
        if (q == 0 && dgamma != nullptr) {
#pragma unroll
            for (int e = 0; e < 3; ++e) { dg += fold[(e * 2 + 0) * 128 + tid]; db += fold[(e * 2 + 1) * 128 + tid]; }
            dgamma[c] = dg;
            dbeta[c] = db;
        }
        return;
    }
    const int r = lane & 15, kq = lane >> 4;
    const int nK16 = (K + 15) >> 4;
    const int k0 = ((int)blockIdx.x % nK16) * 16, m0 = ((int)blockIdx.x / nK16) * 16;
    const int kc = min(k0 + r, K - 1);
    // W^T fragments of this wave's n blocks: requested with the staging loads, not behind the barrier (one L2 round trip less)
    constexpr int per = (N / 16) / NW;
    const int b0 = wave * per;
    float fb[per][4];
    if (dx != nullptr) {
#pragma unroll
        for (int uu = 0; uu < per; ++uu) {
            const int nb = 16 * (b0 + uu) + 4 * kq;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) fb[uu][jj] = W[(size_t)(nb + jj) * ldw + kc];
        }
    }
    {
        const int row = tid >> 5, p = tid & 31, grow = min(m0 + row, M - 1);
        const float mean = stats[2 * grow], rstd = stats[2 * grow + 1];
        f32x4 gg[4], xh[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * p + 128 * j;
            f32x4 g = *reinterpret_cast<const f32x4*>(g1 + (size_t)grow * ldg1 + c);
            g += w2 * *reinterpret_cast<const f32x4*>(g2 + (size_t)grow * ldg2 + c) +
                 w3 * *reinterpret_cast<const f32x4*>(g3 + (size_t)grow * ldg3 + c);
            if (MORE)
                g += mo.w4 * *reinterpret_cast<const f32x4*>(mo.g4 + (size_t)grow * N + c) +
                     mo.w5 * *reinterpret_cast<const f32x4*>(mo.g5 + (size_t)grow * N + c);
            xh[j] = (*reinterpret_cast<const f32x4*>(u + (size_t)grow * ldu + c) - mean) * rstd;
            gg[j] = g * *reinterpret_cast<const f32x4*>(gamma + c);
            const f32x4 t = gg[j] * xh[j];
            s1 += (gg[j][0] + gg[j][1]) + (gg[j][2] + gg[j][3]);
            s2 += (t[0] + t[1]) + (t[2] + t[3]);
        }
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) { s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
        s1 /= N;
        s2 /= N;
        const bool wr = k0 == 0 && m0 + row < M && du != nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * p + 128 * j;
            const f32x4 d = rstd * (gg[j] - s1 - xh[j] * s2);
            *reinterpret_cast<f32x4*>(opa + row * SL_LS + c) = d;
            if (wr) *reinterpret_cast<f32x4*>(du + (size_t)(m0 + row) * N + c) = d;
        }
    }
    __syncthreads();
    if (dx == nullptr) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int uu = 0; uu < per; ++uu) {
        const f32x4 fa = *reinterpret_cast<const f32x4*>(opa + r * SL_LS + 16 * (b0 + uu) + 4 * kq);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[jj], fb[uu][jj], acc, 0, 0, 0);
    }
    sl_fold_store<NW>(red, acc, tid, M, K, m0, k0, SlEpi{0.f, 0.f}, SL_NONE, dx, lddx);
}

// Weight / bias gradients of up to MIL_SMALL_DW_MAX few-rows layers in ONE launch (grid.y = layer): the dW role of
// k_small_bwd, taken out of the layer-by-layer backward chain.  In the backward pass of the token side every layer's dx is
// needed before the previous layer can start, its dW only by the optimizer: the chain launches dx alone (half the time of
// the combined launch) and the host queues (dy, y, x, dW, db) of every layer; this kernel forms all of them at the end of
// the pass.  Descriptors travel as kernel arguments (no device-side table to build or upload).
struct SmallDwBatch {
    mil_small_dw_desc d[MIL_SMALL_DW_MAX];
    int first[MIL_SMALL_DW_MAX + 1];          // first workgroup of every layer (prefix sums of the tile counts): no idle workgroups
    int n;
};

__global__ __launch_bounds__(512) void k_small_dw_grouped(const SmallDwBatch batch) {
    int layer = 0;
#pragma unroll
    for (int stp = MIL_SMALL_DW_MAX / 2; stp >= 1; stp >>= 1)                                // 5 dependent scalar loads, not <= 31
        if (layer + stp < batch.n && (int)blockIdx.x >= batch.first[layer + stp]) layer += stp;
    const mil_small_dw_desc& dd = batch.d[layer];
    const SlDwArgs d{dd.dy, dd.yv, dd.x, dd.dW, dd.db, dd.lddy, dd.ldyv, dd.ldx, dd.lddw, dd.act, dd.M, dd.N, dd.K};
    sl_dw_role<false>(d, (int)blockIdx.x - batch.first[layer], SmallDyExtra{});
}

static inline bool sl_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// y = act((x + x2) W^T + b) (+ residual); xin [M, K] contiguous = x + x2 (written for the weight gradient).  x2 == NULL:
// mil_linear_small_fwd.
extern "C" int mil_linear_small_fwd_add(const float* x, int ldx, const float* x2, int ldx2, float* xin, const float* W, int ldw,
                                        const float* bias, int act, const float* residual, int ldr, float* y, int ldy, int M,
                                        int N, int K, void* stream) {
    if (!x || !W || !y || M <= 0 || M > MIL_SMALL_ROWS || N <= 0 || K <= 0) return MIL_EINVAL;
    if ((K & 15) || (ldx & 3) || (ldw & 3) || act < 0 || act > 4) return MIL_EINVAL;
    if (!sl_aligned16(x) || !sl_aligned16(W)) return MIL_EINVAL;
    if ((x2 != nullptr) != (xin != nullptr)) return MIL_EINVAL;
    if (x2 && ((ldx2 & 3) || !sl_aligned16(x2) || !sl_aligned16(xin))) return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((N + 15) / 16, (M + 15) / 16);
    if (K >= 1024)
        hipLaunchKernelGGL((k_small_fwd<SL_WAVES_DEEP>), grid, dim3(64 * SL_WAVES_DEEP), 0, st, x, ldx, W, ldw, bias, act,
                           residual, ldr, y, ldy, M, N, K, x2, ldx2, xin);
    else
        hipLaunchKernelGGL((k_small_fwd<SL_WAVES>), grid, dim3(64 * SL_WAVES), 0, st, x, ldx, W, ldw, bias, act, residual,
                           ldr, y, ldy, M, N, K, x2, ldx2, xin);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
extern "C" int mil_linear_small_fwd(const float* x, int ldx, const float* W, int ldw, const float* bias, int act,
                                    const float* residual, int ldr, float* y, int ldy, int M, int N, int K,
                                    void* stream) {
    return mil_linear_small_fwd_add(x, ldx, nullptr, 0, nullptr, W, ldw, bias, act, residual, ldr, y, ldy, M, N, K, stream);
}

// mil_linear_small_bwd on the gradient dy + dy2 + dy3 + dy4 (extras [M, N] contiguous, nullable); dysum [M, N] (nullable;
// needs dx): the sum, for a weight gradient formed later.
extern "C" int mil_linear_small_bwd_sum(const float* dy, int lddy, const float* dy2, const float* dy3, const float* dy4,
                                        float* dysum, const float* y_or_pre, int ldyv, int act, const float* x, int ldx,
                                        const float* W, int ldw, float* dx, int lddx, float* dW, int lddw, float* db, int M,
                                        int N, int K, void* stream) {
    if (!dy || M <= 0 || M > MIL_SMALL_ROWS || N <= 0 || K <= 0 || act < 0 || act > 4) return MIL_EINVAL;
    if (dysum && !dx) return MIL_EINVAL;
    if ((dy2 && !sl_aligned16(dy2)) || (dy3 && !sl_aligned16(dy3)) || (dy4 && !sl_aligned16(dy4)) || (dysum && !sl_aligned16(dysum)))
        return MIL_EINVAL;
    const bool has_ex = dy2 || dy3 || dy4 || dysum;
    const SmallDyExtra ex{dy2 ? dy2 : dy, dy3 ? dy3 : dy, dy4 ? dy4 : dy, dy2 ? 1.f : 0.f, dy3 ? 1.f : 0.f, dy4 ? 1.f : 0.f, dysum};
    if (has_ex && lddy != N) return MIL_EINVAL;               // the stand-in pointers are read with the extras' stride
    if (act != SL_NONE && !y_or_pre) return MIL_EINVAL;
    if ((dW || db) && !x) return MIL_EINVAL;
    if (dx && !W) return MIL_EINVAL;
    if ((N & 15) || (lddy & 3) || (act != SL_NONE && (ldyv & 3)) || !sl_aligned16(dy) ||
        (act != SL_NONE && !sl_aligned16(y_or_pre)))
        return MIL_EINVAL;
    const int nKt = (K + 127) / 128;
    const int nW = (dW || db) ? ((N + 63) / 64) * nKt : 0;
    const int nX = dx ? ((K + 15) / 16) * ((M + 15) / 16) : 0;
    if (nW + nX == 0) return MIL_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nW + nX);
    if (dx != nullptr && N >= 1024) {
        if (has_ex)
            hipLaunchKernelGGL((k_small_bwd<SL_WAVES_DEEP, true>), grid, dim3(64 * SL_WAVES_DEEP), 0, st, dy, lddy, y_or_pre, ldyv,
                               act, x, ldx, W, ldw, dx, lddx, dW, lddw, db, M, N, K, nW, nKt, ex);
        else
            hipLaunchKernelGGL((k_small_bwd<SL_WAVES_DEEP, false>), grid, dim3(64 * SL_WAVES_DEEP), 0, st, dy, lddy, y_or_pre, ldyv,
                               act, x, ldx, W, ldw, dx, lddx, dW, lddw, db, M, N, K, nW, nKt, ex);
    } else {
        if (has_ex)
            hipLaunchKernelGGL((k_small_bwd<SL_WAVES, true>), grid, dim3(64 * SL_WAVES), 0, st, dy, lddy, y_or_pre, ldyv, act, x, ldx,
                               W, ldw, dx, lddx, dW, lddw, db, M, N, K, nW, nKt, ex);
        else
            hipLaunchKernelGGL((k_small_bwd<SL_WAVES, false>), grid, dim3(64 * SL_WAVES), 0, st, dy, lddy, y_or_pre, ldyv, act, x, ldx,
                               W, ldw, dx, lddx, dW, lddw, db, M, N, K, nW, nKt, ex);
    }
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
// dx of mil_linear_small_bwd as `nsplit` PARTIAL sums over n (nsplit in {2, 4}, N / nsplit a multiple of 512):
// dx_parts [nsplit][M][K] contiguous, part s = dpre[:, s N / S : (s + 1) N / S] W[s N / S : .., :]; their sum is dx.
extern "C" int mil_linear_small_bwd_split(const float* dy, int lddy, const float* y_or_pre, int ldyv, int act, const float* W,
                                          int ldw, float* dx_parts, int M, int N, int K, int nsplit, void* stream) {
    if (!dy || !W || !dx_parts || M <= 0 || M > MIL_SMALL_ROWS || N <= 0 || K <= 0 || act < 0 || act > 4) return MIL_EINVAL;
    if (act != SL_NONE && !y_or_pre) return MIL_EINVAL;
    if ((nsplit != 2 && nsplit != 4) || (N % (nsplit * SL_KCH)) != 0) return MIL_EINVAL;
    if ((lddy & 3) || (act != SL_NONE && (ldyv & 3)) || !sl_aligned16(dy) || (act != SL_NONE && !sl_aligned16(y_or_pre))) return MIL_EINVAL;
    const int nX = ((K + 15) / 16) * ((M + 15) / 16);
    const SmallDyExtra ex{dy, dy, dy, 0.f, 0.f, 0.f, nullptr};
    const dim3 grid(nX, nsplit);
    hipStream_t st = (hipStream_t)stream;
    if (N / nsplit >= 1024)
        hipLaunchKernelGGL((k_small_bwd<SL_WAVES_DEEP, false>), grid, dim3(64 * SL_WAVES_DEEP), 0, st, dy, lddy, y_or_pre, ldyv, act,
                           (const float*)nullptr, 0, W, ldw, dx_parts, K, (float*)nullptr, 0, (float*)nullptr, M, N, K, 0, 1, ex);
    else
        hipLaunchKernelGGL((k_small_bwd<SL_WAVES, false>), grid, dim3(64 * SL_WAVES), 0, st, dy, lddy, y_or_pre, ldyv, act,
                           (const float*)nullptr, 0, W, ldw, dx_parts, K, (float*)nullptr, 0, (float*)nullptr, M, N, K, 0, 1, ex);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_linear_small_bwd(const float* dy, int lddy, const float* y_or_pre, int ldyv, int act, const float* x,
                                    int ldx, const float* W, int ldw, float* dx, int lddx, float* dW, int lddw,
                                    float* db, int M, int N, int K, void* stream) {
    return mil_linear_small_bwd_sum(dy, lddy, nullptr, nullptr, nullptr, nullptr, y_or_pre, ldyv, act, x, ldx, W, ldw, dx, lddx,
                                    dW, lddw, db, M, N, K, stream);
}

// out = a + b (+ c) (+ d), n floats (n % 4 == 0, 16-byte aligned): the one place a gradient sum of the token side is still
// materialised - a layer whose input carries no gradient has no dx launch to ride on (the text projection in front of the
// two-way transformer) - in ONE launch instead of autograd's one add per extra consumer.
__global__ __launch_bounds__(256) void k_sum4(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                              const float* __restrict__ d, float wc, float wd, float* __restrict__ out, int n4) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 va = reinterpret_cast<const f32x4*>(a)[i], vb = reinterpret_cast<const f32x4*>(b)[i];
    const f32x4 vc = reinterpret_cast<const f32x4*>(c)[i], vd = reinterpret_cast<const f32x4*>(d)[i];
    reinterpret_cast<f32x4*>(out)[i] = (va + vb) + (wc * vc + wd * vd);
}
extern "C" int mil_sum4(const float* a, const float* b, const float* c, const float* d, float* out, int n, void* stream) {
    if (!a || !b || !out || n < 0 || (n & 3) || (d && !c)) return MIL_EINVAL;
    if (!sl_aligned16(a) || !sl_aligned16(b) || (c && !sl_aligned16(c)) || (d && !sl_aligned16(d)) || !sl_aligned16(out)) return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    hipLaunchKernelGGL(k_sum4, dim3((n / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, b, c ? c : a, d ? d : a, c ? 1.f : 0.f,
                       d ? 1.f : 0.f, out, n / 4);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_linear_small_dw_grouped(const mil_small_dw_desc* descs, int n, void* stream) {
    if (n < 0 || n > MIL_SMALL_DW_MAX || (n > 0 && !descs)) return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    SmallDwBatch batch;
    int total = 0;
    batch.n = n;
    for (int i = 0; i < n; ++i) {
        const mil_small_dw_desc& d = descs[i];
        if (!d.dy || !d.x || (!d.dW && !d.db) || d.M <= 0 || d.M > MIL_SMALL_ROWS || d.N <= 0 || d.K <= 0 || d.act < 0 || d.act > 4)
            return MIL_EINVAL;
        if (d.act != SL_NONE && !d.yv) return MIL_EINVAL;
        batch.d[i] = d;
        batch.first[i] = total;
        total += ((d.N + 63) / 64) * ((d.K + 127) / 128);
    }
    batch.first[n] = total;
    hipLaunchKernelGGL(k_small_dw_grouped, dim3(total), dim3(512), 0, (hipStream_t)stream, batch);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}


// y = act((LayerNorm(u) gamma + beta [+ x2]) W^T + b) [+ residual] in ONE launch; also writes xn = the norm's output, xin =
// xn + x2 (only with x2) and the row statistics.  u [M, 512], W [N, 512]; see k_small_fwd_ln.
extern "C" int mil_linear_small_ln_fwd(const float* u, int ldu, const float* gamma, const float* beta, float eps,
                                       const float* x2, int ldx2, const float* W, int ldw, const float* bias, int act,
                                       const float* residual, int ldr, float* y, int ldy, float* xn, float* xin, float* stats,
                                       int M, int N, void* stream) {
    if (!u || !gamma || !beta || !W || !y || !xn || !stats || M <= 0 || M > MIL_SMALL_ROWS || N <= 0) return MIL_EINVAL;
    if ((x2 != nullptr) != (xin != nullptr)) return MIL_EINVAL;
    if ((ldu & 3) || (ldw & 3) || (x2 && (ldx2 & 3)) || act < 0 || act > 4) return MIL_EINVAL;
    if (!sl_aligned16(u) || !sl_aligned16(W) || !sl_aligned16(gamma) || !sl_aligned16(beta) || !sl_aligned16(xn) ||
        (x2 && (!sl_aligned16(x2) || !sl_aligned16(xin))))
        return MIL_EINVAL;
    const dim3 grid((N + 15) / 16, (M + 15) / 16);
    hipLaunchKernelGGL((k_small_fwd_ln<SL_WAVES>), grid, dim3(64 * SL_WAVES), 0, (hipStream_t)stream, u, ldu, gamma, beta, eps, x2,
                       ldx2, W, ldw, bias, act, residual, ldr, y, ldy, xn, xin, stats, M, N);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// Input gradient of the layer P that FEEDS a LayerNorm, with the norm's backward applied on the way in (k_small_bwd_ln):
// g1 (+ g2) [M, 512] = gradient at the norm's output, u = P's output (the norm's input), stats from the forward;
// dx [M, K] = du W (W = P's weight [512, K]; NULL: du only), du [M, 512] (nullable), dgamma / dbeta [512] (both or neither).
extern "C" int mil_linear_small_ln_bwd5(const float* g1, int ldg1, const float* g2, int ldg2, const float* g3, int ldg3,
                                        const float* g4, const float* g5, const float* u, int ldu, const float* stats,
                                        const float* gamma, const float* W, int ldw, float* dx, int lddx, float* du,
                                        float* dgamma, float* dbeta, int M, int K, void* stream) {
    if (!g1 || !u || !stats || !gamma || M <= 0 || M > MIL_SMALL_ROWS) return MIL_EINVAL;
    if (g3 && ((ldg3 & 3) || !sl_aligned16(g3))) return MIL_EINVAL;
    if ((g4 && !sl_aligned16(g4)) || (g5 && !sl_aligned16(g5))) return MIL_EINVAL;
    if (ldg1 < SLN_E) return MIL_EINVAL;
    // the stand-in of a missing g4 / g5 is read with THEIR stride (512): the other of the two where there is one - g1 read
    // that way with ldg1 > 512 lands in the gap columns of g1's parent buffer, and 0 x NaN there is NaN.  (Both missing:
    // the kernel without them.)
    const float* const g45 = g4 ? g4 : g5;
    const SmallLnMore mo{g4 ? g4 : g45, g5 ? g5 : g45, g4 ? 1.f : 0.f, g5 ? 1.f : 0.f};
    if ((dx != nullptr) && (!W || K <= 0)) return MIL_EINVAL;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return MIL_EINVAL;
    if ((ldg1 & 3) || (g2 && (ldg2 & 3)) || (ldu & 3) || !sl_aligned16(g1) || (g2 && !sl_aligned16(g2)) || !sl_aligned16(u) ||
        !sl_aligned16(gamma) || (du && !sl_aligned16(du)))
        return MIL_EINVAL;
    const int kt = dx ? (K + 15) / 16 : 1;
    const int nX = kt * ((M + 15) / 16);
    auto kern = (g4 || g5) ? k_small_bwd_ln<SL_WAVES, true> : k_small_bwd_ln<SL_WAVES, false>;
    hipLaunchKernelGGL(kern, dim3(nX + (dgamma ? 4 : 0)), dim3(64 * SL_WAVES), 0, (hipStream_t)stream, g1, ldg1,
                       g2 ? g2 : g1, g2 ? ldg2 : ldg1, g3 ? g3 : g1, g3 ? ldg3 : ldg1, g2 ? 1.f : 0.f, g3 ? 1.f : 0.f, mo, u, ldu, stats, gamma,
                       W, ldw, dx, lddx, du, dgamma, dbeta, M, dx ? K : 16, nX);      // a missing g2 / g3: g1 again, weight 0 (no branch)
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
extern "C" int mil_linear_small_ln_bwd3(const float* g1, int ldg1, const float* g2, int ldg2, const float* g3, int ldg3,
                                        const float* u, int ldu, const float* stats, const float* gamma, const float* W,
                                        int ldw, float* dx, int lddx, float* du, float* dgamma, float* dbeta, int M, int K,
                                        void* stream) {
    return mil_linear_small_ln_bwd5(g1, ldg1, g2, ldg2, g3, ldg3, nullptr, nullptr, u, ldu, stats, gamma, W, ldw, dx, lddx, du,
                                    dgamma, dbeta, M, K, stream);
}
extern "C" int mil_linear_small_ln_bwd(const float* g1, int ldg1, const float* g2, int ldg2, const float* u, int ldu,
                                       const float* stats, const float* gamma, const float* W, int ldw, float* dx, int lddx,
                                       float* du, float* dgamma, float* dbeta, int M, int K, void* stream) {
    return mil_linear_small_ln_bwd3(g1, ldg1, g2, ldg2, nullptr, 0, u, ldu, stats, gamma, W, ldw, dx, lddx, du, dgamma, dbeta, M,
                                    K, stream);
}
