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
//            k_ny_reduce  (csrc/nystrom_tile.h) sums the partials chunk 0, 1, 2 .. in that order into dU and dkL.
// All products on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate); a 64-deep contraction pairs d with d + 32 in one MFMA
// step.  QSCALE = 64^-0.5 = 2^-3, so where it is applied does not change a bit.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "nystrom_tile.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int TA_FR = 128;                          // rows per forward workgroup (4 waves x 32)
constexpr int TA_BC = 256;                          // rows per backward workgroup (8 waves x 32)
constexpr int TA_PART = NY_M * NY_DH;               // floats of one backward partial: [8 landmark tiles][64 d][32 landmarks]

// The two bodies serve two kernels each: the single-bag one (PACKED false: tab, nb, total_blocks are constants that fold away,
// and the kernel compiles to what it was before the bodies were shared) and the packed one (csrc/tm_packed.h), where the row
// tile runs over all bags' rows, n_pad is their count R, and kL / U are taken at the tile's bag.  The bodies' pointers carry no
// __restrict__: inlined, they ARE the kernel's restrict arguments, which is what keeps the single-bag code as it was.
template <bool PACKED>
__device__ __forceinline__ void tok_fwd_body(const float* qkv, const float* kL, const float* U, int n_pad, float* O, float* lse,
                                             const int32_t* tab, int nb, int total_blocks) {
    const int hd = blockIdx.y;
    if constexpr (PACKED) {                     // two 128-row tiles per block
        const int bag = tm_packed_bag(tab, nb, total_blocks, blockIdx.x / (TM_PACKED_BLK / TA_FR));
        if (bag < 0) return;
        kL += (size_t)bag * NY_H * NY_M * NY_DH;
        U += (size_t)bag * NY_H * NY_M * NY_DH;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t row = (size_t)blockIdx.x * TA_FR + wave * 32 + r;
    float qr[32];
    load32(qkv + row * NY_QKV + hd * NY_DH + 32 * hh, qr);
    f32x16 o0 = zero16(), o1 = zero16();
    float m = -INFINITY, l = 0.f;               // of this lane's row; l over this lane half's landmarks until the end
    const float* kh = kL + (size_t)hd * NY_M * NY_DH;
    const float* uh = U + (size_t)hd * NY_M * NY_DH;
    for (int t = 0; t < NY_M / 32; ++t) {
        float kr[32];
        load32(kh + (32 * t + r) * NY_DH + 32 * hh, kr);
        f32x16 s = dot64_tile(kr, qr);          // S^T: landmark 32 t + mfma32_row(i, hh), this lane's row
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] *= NY_QSCALE;
        online_softmax_step(s, m, l, o0, o1);
        // O^T [d][row] += U^T [d][landmark] P^T [landmark][row]
        acc_rows<NY_DH>(uh + (32 * t + 4 * hh) * NY_DH + r, s, o0, o1);
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.f / l;
    if (hh == 0) lse[(size_t)hd * n_pad + row] = m + logf(l);
    store_row64(O + row * NY_D + hd * NY_DH + 4 * hh, o0, o1, inv);
}

__global__ __launch_bounds__(256) void k_tok_fwd(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                 const float* __restrict__ U, int n_pad, float* __restrict__ O,
                                                 float* __restrict__ lse) {
    tok_fwd_body<false>(qkv, kL, U, n_pad, O, lse, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void k_tok_fwd_packed(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                        const float* __restrict__ U, int n_pad, float* __restrict__ O,
                                                        float* __restrict__ lse, const int32_t* __restrict__ tab, int nb,
                                                        int total_blocks) {
    tok_fwd_body<true>(qkv, kL, U, n_pad, O, lse, tab, nb, total_blocks);
}

// P = exp(S - lse) and dP = dO U^T of one 32-landmark x 32-row tile, landmark 32 t + mfma32_row(i, hh) down the registers and
// the row on the lane.  kt / ut: this lane's landmark row of kL / U, qrow / dorow: its row of q / dO, all at d = 32 hh.
__device__ __forceinline__ void tok_tile(const float* __restrict__ kt, const float* __restrict__ ut,
                                         const float* __restrict__ qrow, const float* __restrict__ dorow, float lse_r,
                                         f32x16& p, f32x16& dp) {
    float a[32], b[32];
    load32(kt, a);
    load32(qrow, b);
    p = dot64_tile(a, b);
    load32(ut, a);
    load32(dorow, b);
    dp = dot64_tile(a, b);
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = expf(p[i] * NY_QSCALE - lse_r);
}

template <bool PACKED>
__device__ __forceinline__ void tok_bwd_body(const float* qkv, const float* kL, const float* U, const float* lse, const float* dO,
                                             int n_pad, float* dqkv, float* wsU, float* wsK, const int32_t* tab, int nbags,
                                             int total_blocks) {
    __shared__ float T[8][2][32 * NY_TLD];        // per wave: P and dS [landmark][row] of the current tile
    __shared__ float R[4][NY_DH * 32];            // per pair of waves (w, w + 4): a [d][landmark] tile, dU^T then dkL^T
    const int c = blockIdx.x, hd = blockIdx.y;
    if constexpr (PACKED) {                       // TA_BC = 256: a chunk is a block; uniform per workgroup, ahead of every barrier
        const int bag = tm_packed_bag(tab, nbags, total_blocks, c);
        if (bag < 0) return;
        kL += (size_t)bag * NY_H * NY_M * NY_DH;
        U += (size_t)bag * NY_H * NY_M * NY_DH;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const size_t nb = (size_t)c * TA_BC + wave * 32, n = nb + r;      // this wave's 32 rows, this lane's row
    const float* qh = qkv + hd * NY_DH;           // q[row][0] of this head is qh + row * NY_QKV
    const float* doh = dO + hd * NY_DH;
    const float* kh = kL + (size_t)hd * NY_M * NY_DH;
    const float* uh = U + (size_t)hd * NY_M * NY_DH;
    const float* qrow = qh + n * NY_QKV + 32 * hh;
    const float* dorow = doh + n * NY_D + 32 * hh;
    const float lser = lse[(size_t)hd * n_pad + n];
    float del = 0.f;
    for (int t = 0; t < NY_M / 32; ++t) {
        f32x16 p, dp;
        tok_tile(kh + (32 * t + r) * NY_DH + 32 * hh, uh + (32 * t + r) * NY_DH + 32 * hh, qrow, dorow, lser, p, dp);
        float ts = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) ts += p[i] * dp[i];
        del += ts;
    }
    del += __shfl_xor(del, 32, 64);
    f32x16 dq0 = zero16(), dq1 = zero16();        // dq^T [d][row]: d = mfma32_row(i, hh) (+ 32), this lane's row
    for (int t = 0; t < NY_M / 32; ++t) {
        f32x16 p, ds;
        const float* dor = dorow;                 // the dO row is read again per tile (an L1 hit): held across the loop, its
        asm volatile("" : "+v"(dor));             // 32 values push the kernel past its 256 registers into scratch
        tok_tile(kh + (32 * t + r) * NY_DH + 32 * hh, uh + (32 * t + r) * NY_DH + 32 * hh, qrow, dor, lser, p, ds);
#pragma unroll
        for (int i = 0; i < 16; ++i) ds[i] = NY_QSCALE * (p[i] * (ds[i] - del));
        __builtin_amdgcn_sched_barrier(0);        // keeps the loads of the phases below from being hoisted over this one
        // dq^T [d][row] += kL^T [d][landmark] dS [landmark][row]
        acc_rows<NY_DH>(kh + (32 * t + 4 * hh) * NY_DH + r, ds, dq0, dq1);
        tile_put(T[wave][0], p, r, hh);
        tile_put(T[wave][1], ds, r, hh);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        // dU^T [d][landmark] = dO^T [d][row] P^T [row][landmark], then dkL^T = Q^T dS^T, over this wave's 32 rows: step j takes
        // rows j and j + 16.  The eight waves' tiles meet in four LDS slots: waves 0 .. 3 write, waves 4 .. 7 add onto the slot
        // of wave - 4, the four slots are summed as a tree - the same order in every run
        const size_t po = (((size_t)c * NY_H + hd) * (NY_M / 32) + t) * (NY_DH * 32);
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const float* src = which ? qh + nb * NY_QKV + r : doh + nb * NY_D + r;
            const int ld = which ? NY_QKV : NY_D;
            f32x16 g0 = zero16(), g1 = zero16();
            acc_tile_t(T[wave][which], src, ld, r, hh, g0, g1);
            if (wave < 4) rtile_put(R[wave], g0, g1, r, hh, false);
            __syncthreads();
            if (wave >= 4) rtile_put(R[wave - 4], g0, g1, r, hh, true);
            __syncthreads();
            rtile_sum4<512>(R, (which ? wsK : wsU) + po, tid);
            __syncthreads();
        }
    }
    store_row64(dqkv + n * NY_QKV + hd * NY_DH + 4 * hh, dq0, dq1, 1.f);
}

__global__ __launch_bounds__(512) void k_tok_bwd(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                 const float* __restrict__ U, const float* __restrict__ lse,
                                                 const float* __restrict__ dO, int n_pad, float* __restrict__ dqkv,
                                                 float* __restrict__ wsU, float* __restrict__ wsK) {
    tok_bwd_body<false>(qkv, kL, U, lse, dO, n_pad, dqkv, wsU, wsK, nullptr, 0, 0);
}

__global__ __launch_bounds__(512) void k_tok_bwd_packed(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                        const float* __restrict__ U, const float* __restrict__ lse,
                                                        const float* __restrict__ dO, int n_pad, float* __restrict__ dqkv,
                                                        float* __restrict__ wsU, float* __restrict__ wsK,
                                                        const int32_t* __restrict__ tab, int nbags, int total_blocks) {
    tok_bwd_body<true>(qkv, kL, U, lse, dO, n_pad, dqkv, wsU, wsK, tab, nbags, total_blocks);
}

}  // namespace

extern "C" {

size_t mil_tm_tok_attn_ws_floats(int n_pad, int backward) {
    if (!ny_shape_ok(n_pad) || !backward) return 0;
    return (size_t)2 * (n_pad / TA_BC) * NY_H * TA_PART;
}

int mil_tm_tok_attn_fwd(const float* qkv, const float* kL, const float* U, int n_pad, float* O, float* lse, float* ws,
                        void* stream) {
    (void)ws;                                   // the forward needs no workspace: every row's 256 landmarks meet in one wave
    if (!qkv || !kL || !U || !O || !lse || !ny_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(kL) || !ny_aligned(U) || !ny_aligned(O) || !ny_aligned(lse)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_tok_fwd, dim3(n_pad / TA_FR, NY_H), dim3(256), 0, (hipStream_t)stream, qkv, kL, U, n_pad, O, lse);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int mil_tm_tok_attn_bwd(const float* qkv, const float* kL, const float* U, const float* lse, const float* dO, int n_pad,
                        float* dqkv, float* dU, float* dkL, float* ws, void* stream) {
    if (!qkv || !kL || !U || !lse || !dO || !dqkv || !dU || !dkL || !ws || !ny_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(kL) || !ny_aligned(U) || !ny_aligned(lse) || !ny_aligned(dO) || !ny_aligned(dqkv) ||
        !ny_aligned(dU) || !ny_aligned(dkL) || !ny_aligned(ws))
        return MIL_EINVAL;
    const int nc = n_pad / TA_BC;
    hipLaunchKernelGGL(k_tok_bwd, dim3(nc, NY_H), dim3(512), 0, (hipStream_t)stream, qkv, kL, U, lse, dO, n_pad, dqkv, ws,
                       ws + (size_t)nc * NY_H * TA_PART);
    hipLaunchKernelGGL(k_ny_reduce<2>, dim3(NY_M / 32, NY_H, 2), dim3(256), 0, (hipStream_t)stream, ws, nc, dU, dkL,
                       TmPackedArg<false>{});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

size_t mil_tm_tok_attn_packed_ws_floats(int total_blocks, int nb, int backward) {
    if (!tm_packed_ok(&nb, nb, total_blocks) || !backward) return 0;
    return (size_t)2 * total_blocks * NY_H * TA_PART;
}

int mil_tm_tok_attn_fwd_packed(const float* qkv, const float* kL, const float* U, float* O, float* lse, float* ws,
                               const int32_t* blk_off, int nb, int total_blocks, void* stream) {
    (void)ws;                                   // as the single-bag forward: no workspace
    if (!qkv || !kL || !U || !O || !lse || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(kL) || !ny_aligned(U) || !ny_aligned(O) || !ny_aligned(lse)) return MIL_EINVAL;
    const int rows = total_blocks * TM_PACKED_BLK;
    hipLaunchKernelGGL(k_tok_fwd_packed, dim3(rows / TA_FR, NY_H), dim3(256), 0, (hipStream_t)stream, qkv, kL, U, rows, O, lse,
                       blk_off, nb, total_blocks);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int mil_tm_tok_attn_bwd_packed(const float* qkv, const float* kL, const float* U, const float* lse, const float* dO, float* dqkv,
                               float* dU, float* dkL, float* ws, const int32_t* blk_off, int nb, int total_blocks, void* stream) {
    if (!qkv || !kL || !U || !lse || !dO || !dqkv || !dU || !dkL || !ws || !tm_packed_ok(blk_off, nb, total_blocks))
        return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(kL) || !ny_aligned(U) || !ny_aligned(lse) || !ny_aligned(dO) || !ny_aligned(dqkv) ||
        !ny_aligned(dU) || !ny_aligned(dkL) || !ny_aligned(ws))
        return MIL_EINVAL;
    hipLaunchKernelGGL(k_tok_bwd_packed, dim3(total_blocks, NY_H), dim3(512), 0, (hipStream_t)stream, qkv, kL, U, lse, dO,
                       total_blocks * TM_PACKED_BLK, dqkv, ws, ws + (size_t)total_blocks * NY_H * TA_PART, blk_off, nb,
                       total_blocks);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ny_reduce<2, true>), dim3(NY_M / 32, NY_H, 2 * nb), dim3(256), 0, (hipStream_t)stream, ws,
                       TM_PACKED_BLK / TA_BC, dU, dkL, TmPackedArg<true>{blk_off, nb, total_blocks});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

}  // extern "C"
