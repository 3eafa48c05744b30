// TransMIL: the token-query pass of the Nystrom core without its [8, n_pad, 256] softmax map (A1 of csrc/transmil.hip).
//
// Per head, Q = the q columns of the merged [n_pad, 1536] to_qkv rows read in place (every row a query, the zero front pad
// rows included: they get uniform weights), the keys kL [256, 64] (the landmarks, not scaled) and the values U [256, 64]:
// S = QSCALE Q kL^T, O = softmax(S) U and lse = logsumexp(S).  All 256 keys of a query are seen by one wave, so the forward is
// one launch without partials; nothing of size [n_pad, 256] reaches memory, in either direction.  The register orientation is
// that of csrc/landmark_attn.hip with the roles of rows and landmarks exchanged.
//
//  forward   k_tok_fwd    workgroup = (128 rows, head), 4 waves of 32 rows each, no LDS.  Per 32-landmark tile S^T = kL Q^T
//                         (landmarks down the accumulator registers, the row on the lane), a running maximum and sum per row,
//                         P^T straight back in as the B operand of O^T += U^T P^T.  Writes O / l and lse.
//  backward  k_tok_bwd    workgroup = (256-row chunk, head), 8 waves of 32 rows each, two per SIMD.  First sweep over the 8
//                         landmark tiles: P = exp(S - lse), dP = dO U^T (same orientation) and delta = rowsum(P o dP), a sum
//                         over the registers and the two lane halves.  Second sweep: P and dP again, dS = QSCALE P o (dP - delta);
//                         dq^T += kL^T dS takes dS as the B operand and stays in registers until the end (the rows are the
//                         wave's own); dU and dkL sum over the rows (the lane index), so P and dS go through 32 x 33 LDS
//                         tiles per wave into dU^T = dO^T P^T and dkL^T = Q^T dS^T over the wave's 32 rows; the eight waves'
//                         tiles are added in LDS in a fixed order and leave as one partial per (chunk, head, tile).
//            k_tok_reduce sums the partials chunk 0, 1, 2 .. in that order into dU and dkL.
// All products on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate); a 64-deep contraction pairs d with d + 32 in one MFMA
// step.  QSCALE = 64^-0.5 = 2^-3, so where it is applied does not change a bit.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int TA_H = 8, TA_DH = 64, TA_D = 512, TA_QKV = 3 * TA_D, TA_M = 256;
constexpr float TA_QSCALE = 0.125f;                 // 64^-0.5
constexpr int TA_FR = 128;                          // rows per forward workgroup (4 waves x 32)
constexpr int TA_BC = 256;                          // rows per backward workgroup (8 waves x 32)
constexpr int TA_PART = TA_M * TA_DH;               // floats of one backward partial: [8 landmark tiles][64 d][32 landmarks]
constexpr int TA_TLD = 33;

__device__ __forceinline__ void load32(const float* __restrict__ p, float (&v)[32]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 t = reinterpret_cast<const float4*>(p)[j];
        v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
    }
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

__global__ __launch_bounds__(256) void k_tok_fwd(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                 const float* __restrict__ U, int n_pad, float* __restrict__ O,
                                                 float* __restrict__ lse) {
    const int hd = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t row = (size_t)blockIdx.x * TA_FR + wave * 32 + r;
    float qr[32];
    load32(qkv + row * TA_QKV + hd * TA_DH + 32 * hh, qr);
    f32x16 o0 = zero16(), o1 = zero16();
    float m = -INFINITY, l = 0.f;               // of this lane's row; l over this lane half's landmarks until the end
    const float* kh = kL + (size_t)hd * TA_M * TA_DH;
    const float* uh = U + (size_t)hd * TA_M * TA_DH;
    for (int t = 0; t < TA_M / 32; ++t) {
        float kr[32];
        load32(kh + (32 * t + r) * TA_DH + 32 * hh, kr);
        f32x16 s = zero16();                    // S^T: landmark 32 t + mfma32_row(i, hh), this lane's row
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[kk], qr[kk], s, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] *= TA_QSCALE;
        float tm = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) tm = fmaxf(tm, s[i]);
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        const float sc = expf(m - mn);          // 0 on the first tile (m = -inf)
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s[i] = expf(s[i] - mn);
            ps += s[i];
        }
        l = l * sc + ps;
        m = mn;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o0[i] *= sc;
            o1[i] *= sc;
        }
        // O^T [d][row] += U^T [d][landmark] P^T [landmark][row]: step i sums the two landmarks register i holds in the lane halves
        const float* up = uh + (32 * t + 4 * hh) * TA_DH + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float* ur = up + ((i & 3) + 8 * (i >> 2)) * TA_DH;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ur[0], s[i], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ur[32], s[i], o1, 0, 0, 0);
        }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.f / l;
    if (hh == 0) lse[(size_t)hd * n_pad + row] = m + logf(l);
    float* op = O + row * TA_D + hd * TA_DH;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d = 8 * g + 4 * hh;             // registers 4 g .. 4 g + 3 are four consecutive d
        *reinterpret_cast<float4*>(op + d) = make_float4(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
        *reinterpret_cast<float4*>(op + d + 32) = make_float4(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
}

// P = exp(S - lse) and dP = dO U^T of one 32-landmark x 32-row tile, landmark 32 t + mfma32_row(i, hh) down the registers and
// the row on the lane.  kt / ut: this lane's landmark row of kL / U, qrow / dorow: its row of q / dO, all at d = 32 hh.
__device__ __forceinline__ void tok_tile(const float* __restrict__ kt, const float* __restrict__ ut,
                                         const float* __restrict__ qrow, const float* __restrict__ dorow, float lse_r,
                                         f32x16& p, f32x16& dp) {
    float a[32], b[32];
    load32(kt, a);
    load32(qrow, b);
    p = zero16();
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) p = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], p, 0, 0, 0);
    load32(ut, a);
    load32(dorow, b);
    dp = zero16();
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], dp, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = expf(p[i] * TA_QSCALE - lse_r);
}

__global__ __launch_bounds__(512) void k_tok_bwd(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                 const float* __restrict__ U, const float* __restrict__ lse,
                                                 const float* __restrict__ dO, int n_pad, float* __restrict__ dqkv,
                                                 float* __restrict__ wsU, float* __restrict__ wsK) {
    __shared__ float T[8][2][32 * TA_TLD];        // per wave: P and dS [landmark][row] of the current tile
    __shared__ float R[4][TA_DH * 32];            // per pair of waves (w, w + 4): a [d][landmark] tile, dU^T then dkL^T
    const int c = blockIdx.x, hd = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const size_t nb = (size_t)c * TA_BC + wave * 32, n = nb + r;      // this wave's 32 rows, this lane's row
    const float* qh = qkv + hd * TA_DH;           // q[row][0] of this head is qh + row * TA_QKV
    const float* doh = dO + hd * TA_DH;
    const float* kh = kL + (size_t)hd * TA_M * TA_DH;
    const float* uh = U + (size_t)hd * TA_M * TA_DH;
    const float* qrow = qh + n * TA_QKV + 32 * hh;
    const float* dorow = doh + n * TA_D + 32 * hh;
    const float lser = lse[(size_t)hd * n_pad + n];
    float del = 0.f;
    for (int t = 0; t < TA_M / 32; ++t) {
        f32x16 p, dp;
        tok_tile(kh + (32 * t + r) * TA_DH + 32 * hh, uh + (32 * t + r) * TA_DH + 32 * hh, qrow, dorow, lser, p, dp);
        float ts = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) ts += p[i] * dp[i];
        del += ts;
    }
    del += __shfl_xor(del, 32, 64);
    f32x16 dq0 = zero16(), dq1 = zero16();        // dq^T [d][row]: d = mfma32_row(i, hh) (+ 32), this lane's row
    for (int t = 0; t < TA_M / 32; ++t) {
        f32x16 p, ds;
        const float* dor = dorow;                 // the dO row is read again per tile (an L1 hit): held across the loop, its
        asm volatile("" : "+v"(dor));             // 32 values push the kernel past its 256 registers into scratch
        tok_tile(kh + (32 * t + r) * TA_DH + 32 * hh, uh + (32 * t + r) * TA_DH + 32 * hh, qrow, dor, lser, p, ds);
#pragma unroll
        for (int i = 0; i < 16; ++i) ds[i] = TA_QSCALE * (p[i] * (ds[i] - del));
        __builtin_amdgcn_sched_barrier(0);        // keeps the loads of the phases below from being hoisted over this one
        // dq^T [d][row] += kL^T [d][landmark] dS [landmark][row]: step i sums register i's two landmarks
        const float* kp = kh + (32 * t + 4 * hh) * TA_DH + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float* kr = kp + ((i & 3) + 8 * (i >> 2)) * TA_DH;
            dq0 = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[0], ds[i], dq0, 0, 0, 0);
            dq1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[32], ds[i], dq1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            T[wave][0][mfma32_row(i, hh) * TA_TLD + r] = p[i];
            T[wave][1][mfma32_row(i, hh) * TA_TLD + r] = ds[i];
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        // dU^T [d][landmark] = dO^T [d][row] P^T [row][landmark], then dkL^T = Q^T dS^T, over this wave's 32 rows: step j takes
        // rows j and j + 16.  The eight waves' tiles meet in four LDS slots: waves 0 .. 3 write, waves 4 .. 7 add onto the slot
        // of wave - 4, the four slots are summed as a tree - the same order in every run
        const size_t po = (((size_t)c * TA_H + hd) * (TA_M / 32) + t) * (TA_DH * 32);
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const float* src = which ? qh + nb * TA_QKV + r : doh + nb * TA_D + r;
            const int ld = which ? TA_QKV : TA_D;
            f32x16 g0 = zero16(), g1 = zero16();
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int nl = j + 16 * hh;
                const float bt = T[wave][which][r * TA_TLD + nl];
                const float* ap = src + (size_t)nl * ld;
                g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[0], bt, g0, 0, 0, 0);
                g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[32], bt, g1, 0, 0, 0);
            }
            if (wave < 4) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int d = mfma32_row(i, hh);
                    R[wave][d * 32 + r] = g0[i];
                    R[wave][(d + 32) * 32 + r] = g1[i];
                }
            }
            __syncthreads();
            if (wave >= 4) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int d = mfma32_row(i, hh);
                    R[wave - 4][d * 32 + r] += g0[i];
                    R[wave - 4][(d + 32) * 32 + r] += g1[i];
                }
            }
            __syncthreads();
            float* out = (which ? wsK : wsU) + po;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = tid + 512 * j;
                out[e] = (R[0][e] + R[1][e]) + (R[2][e] + R[3][e]);
            }
            __syncthreads();
        }
    }
    float* dqp = dqkv + n * TA_QKV + hd * TA_DH;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int d = 8 * g + 4 * hh;             // registers 4 g .. 4 g + 3 are four consecutive d
        *reinterpret_cast<float4*>(dqp + d) = make_float4(dq0[4 * g], dq0[4 * g + 1], dq0[4 * g + 2], dq0[4 * g + 3]);
        *reinterpret_cast<float4*>(dqp + d + 32) = make_float4(dq1[4 * g], dq1[4 * g + 1], dq1[4 * g + 2], dq1[4 * g + 3]);
    }
}

// block = (landmark tile, head, dU | dkL): element e = d * 32 + landmark of the [64][32] tile, thread tid owns e = tid + 256 j
__global__ __launch_bounds__(256) void k_tok_reduce(const float* __restrict__ ws, int nc, float* __restrict__ dU,
                                                    float* __restrict__ dkL) {
    const int lt = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
    const float* p = ws + (size_t)blockIdx.z * nc * TA_H * TA_PART + ((size_t)hd * (TA_M / 32) + lt) * (TA_DH * 32);
    float* dst = blockIdx.z ? dkL : dU;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int c = 0; c < nc; ++c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += p[tid + 256 * j];
        p += (size_t)TA_H * TA_PART;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = tid + 256 * j;
        dst[((size_t)hd * TA_M + lt * 32 + (e & 31)) * TA_DH + (e >> 5)] = acc[j];
    }
}

inline bool ta_shape_ok(int n_pad) { return n_pad > 0 && n_pad % TA_M == 0; }
inline bool ta_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

size_t mil_tm_tok_attn_ws_floats(int n_pad, int backward) {
    if (!ta_shape_ok(n_pad) || !backward) return 0;
    return (size_t)2 * (n_pad / TA_BC) * TA_H * TA_PART;
}

int mil_tm_tok_attn_fwd(const float* qkv, const float* kL, const float* U, int n_pad, float* O, float* lse, float* ws,
                        void* stream) {
    (void)ws;                                   // the forward needs no workspace: every row's 256 landmarks meet in one wave
    if (!qkv || !kL || !U || !O || !lse || !ta_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ta_aligned(qkv) || !ta_aligned(kL) || !ta_aligned(U) || !ta_aligned(O) || !ta_aligned(lse)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tok_fwd, dim3(n_pad / TA_FR, TA_H), dim3(256), 0, (hipStream_t)stream, qkv, kL, U, n_pad, O, lse);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int mil_tm_tok_attn_bwd(const float* qkv, const float* kL, const float* U, const float* lse, const float* dO, int n_pad,
                        float* dqkv, float* dU, float* dkL, float* ws, void* stream) {
    if (!qkv || !kL || !U || !lse || !dO || !dqkv || !dU || !dkL || !ws || !ta_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ta_aligned(qkv) || !ta_aligned(kL) || !ta_aligned(U) || !ta_aligned(lse) || !ta_aligned(dO) || !ta_aligned(dqkv) ||
        !ta_aligned(dU) || !ta_aligned(dkL) || !ta_aligned(ws))
        return MIL_EINVAL;
    const int nc = n_pad / TA_BC;
    hipLaunchKernelGGL(k_tok_bwd, dim3(nc, TA_H), dim3(512), 0, (hipStream_t)stream, qkv, kL, U, lse, dO, n_pad, dqkv, ws,
                       ws + (size_t)nc * TA_H * TA_PART);
    hipLaunchKernelGGL(k_tok_reduce, dim3(TA_M / 32, TA_H, 2), dim3(256), 0, (hipStream_t)stream, ws, nc, dU, dkL);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

}  // extern "C"
