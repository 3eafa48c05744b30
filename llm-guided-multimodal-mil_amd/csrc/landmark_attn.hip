// TransMIL: the landmark-query pass of the Nystrom core without its [8, 256, n_pad] softmax map (A3 of csrc/transmil.hip).
//
// Per head, Q = qL [256, 64] (the landmark queries, scale already applied), K and V the k and v columns of the merged
// [n_pad, 1536] to_qkv rows read in place: W = softmax(Q K^T) V and lse = logsumexp(Q K^T), over ALL n_pad keys (the zero
// front pad rows take part with score 0, as upstream's unmasked attention has it).  The keys are split into chunks across
// workgroups; nothing of size [256, n_pad] reaches memory, in either direction.
//
//  forward   k_lmk_fwd    workgroup = (256-key chunk, head, 64 query rows), 2 waves of 32 query rows each.  Per 32-key tile
//                         S^T = K Q^T (keys down the accumulator registers, the query on the lane), a running maximum and
//                         sum per query, P^T straight back in as the B operand of O^T += V^T P^T.  No LDS.  Writes one
//                         partial (m, l, O^T) per (chunk, head).
//            k_lmk_merge  combines the partials chunk 0, 1, 2 .. in that order: W and lse.
//  backward  k_lmk_delta  delta = rowsum(dW o W)
//            k_lmk_bwd    workgroup = (128-key chunk, head), 4 waves of 32 keys each, which own those keys' dK and dV rows
//                         (accumulated over the 8 query tiles in registers, written once, no atomics).  P = exp(S - lse) is
//                         recomputed with the key on the lane, so dV^T += dW^T P and dK^T += Q^T dS take it as the B
//                         operand; dQ sums over the keys (the lane index), so dS goes through a 32 x 33 LDS tile per wave,
//                         the four waves' dQ^T tiles are added in LDS in a fixed order and leave as one partial per chunk.
//            k_ny_reduce  (csrc/nystrom_tile.h) sums the partials chunk 0, 1, 2 .. in that order into dqL.
// All products on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate).  The 64-deep contractions pair d with d + 32 in one
// MFMA step (lane half h holds d = 32 h .. 32 h + 31 of its row, one contiguous 128-byte read): the order of a dot product's
// terms is free as long as both operands use the same one.  No atomics anywhere: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "nystrom_tile.h"
#include "tm_packed.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int LA_FC = 256;                          // keys per forward workgroup
constexpr int LA_FPART = NY_M * (NY_DH + 2);        // floats of one forward partial: m [256], l [256], O^T [64][256]
constexpr int LA_BC = 128;                          // keys per backward workgroup (4 waves x 32)
constexpr int LA_DQPART = NY_M * NY_DH;             // floats of one backward partial: [8 query tiles][64 d][32 queries]

// The bodies below serve two kernels each: the single-bag one (PACKED false: tab, nb, total_blocks are constants that fold
// away, and the kernel compiles to what it was before the bodies were shared) and the packed one (csrc/tm_packed.h), where
// the chunk index runs over all bags' rows and the small operands are taken at the chunk's bag.  The bodies' pointers carry no
// __restrict__: inlined, they ARE the kernel's restrict arguments, which is what keeps the single-bag code as it was.
template <bool PACKED>
__device__ __forceinline__ void lmk_fwd_body(const float* qkv, const float* qL, float* ws, const int32_t* tab, int nb,
                                             int total_blocks) {
    const int c = blockIdx.x, hd = blockIdx.y;
    if constexpr (PACKED) {                     // LA_FC = 256: a forward chunk is a block
        const int bag = tm_packed_bag(tab, nb, total_blocks, c);
        if (bag < 0) return;
        qL += (size_t)bag * NY_H * NY_M * NY_DH;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const int q0 = blockIdx.z * 64 + wave * 32;
    float qr[32];
    load32(qL + ((size_t)hd * NY_M + q0 + r) * NY_DH + 32 * hh, qr);
    f32x16 o0 = zero16(), o1 = zero16();
    float m = -INFINITY, l = 0.f;               // of query q0 + r; l over this lane half's keys until the end
    const float* kbase = qkv + (size_t)c * LA_FC * NY_QKV + NY_D + hd * NY_DH;
    const float* vbase = kbase + NY_D;
    for (int t = 0; t < LA_FC / 32; ++t) {
        float kr[32];
        load32(kbase + (size_t)(32 * t + r) * NY_QKV + 32 * hh, kr);
        f32x16 s = dot64_tile(kr, qr);          // S^T: key 32 t + mfma32_row(i, hh), query q0 + r
        online_softmax_step(s, m, l, o0, o1);
        // O^T [d][query] += V^T [d][key] P^T [key][query]
        acc_rows<NY_QKV>(vbase + (size_t)(32 * t + 4 * hh) * NY_QKV + r, s, o0, o1);
    }
    l += __shfl_xor(l, 32, 64);
    float* part = ws + ((size_t)c * NY_H + hd) * LA_FPART;
    if (hh == 0) {
        part[q0 + r] = m;
        part[NY_M + q0 + r] = l;
    }
    float* ot = part + 2 * NY_M + q0 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int d = mfma32_row(i, hh);
        ot[d * NY_M] = o0[i];
        ot[(d + 32) * NY_M] = o1[i];
    }
}

__global__ __launch_bounds__(128) void k_lmk_fwd(const float* __restrict__ qkv, const float* __restrict__ qL,
                                                 float* __restrict__ ws) {
    lmk_fwd_body<false>(qkv, qL, ws, nullptr, 0, 0);
}

__global__ __launch_bounds__(128) void k_lmk_fwd_packed(const float* __restrict__ qkv, const float* __restrict__ qL,
                                                        float* __restrict__ ws, const int32_t* __restrict__ tab, int nb,
                                                        int total_blocks) {
    lmk_fwd_body<true>(qkv, qL, ws, tab, nb, total_blocks);
}

// block = (32 queries, head): thread (q = tid & 31, dg = tid >> 5) owns d = dg + 8 j.  ws: the first partial, nc: how many
__device__ __forceinline__ void lmk_merge_body(const float* ws, int nc, float* W, float* lse) {
    const int hd = blockIdx.y, q = blockIdx.x * 32 + (threadIdx.x & 31), dg = threadIdx.x >> 5;
    const float* p0 = ws + (size_t)hd * LA_FPART;
    const size_t step = (size_t)NY_H * LA_FPART;
    float m = -INFINITY;
    for (int c = 0; c < nc; ++c) m = fmaxf(m, p0[c * step + q]);
    float L = 0.f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float* p = p0 + c * step;
        const float w = expf(p[q] - m);
        L += w * p[NY_M + q];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * p[2 * NY_M + (dg + 8 * j) * NY_M + q];
    }
    const float inv = 1.f / L;
#pragma unroll
    for (int j = 0; j < 8; ++j) W[((size_t)hd * NY_M + q) * NY_DH + dg + 8 * j] = acc[j] * inv;
    if (dg == 0) lse[hd * NY_M + q] = m + logf(L);
}

__global__ __launch_bounds__(256) void k_lmk_merge(const float* __restrict__ ws, int nc, float* __restrict__ W,
                                                   float* __restrict__ lse) {
    lmk_merge_body(ws, nc, W, lse);
}

// blockIdx.z = the bag: its chunks alone, in ascending order, into slice `bag` of W and lse
__global__ __launch_bounds__(256) void k_lmk_merge_packed(const float* __restrict__ ws, const int32_t* __restrict__ tab, int nb,
                                                          int total_blocks, float* __restrict__ W, float* __restrict__ lse) {
    const int bag = blockIdx.z;
    int c0, c1;
    if (bag >= nb || !tm_packed_range(tab, total_blocks, bag, c0, c1)) return;
    lmk_merge_body(ws + (size_t)c0 * NY_H * LA_FPART, c1 - c0, W + (size_t)bag * NY_H * NY_M * NY_DH,
                   lse + (size_t)bag * NY_H * NY_M);
}

__global__ __launch_bounds__(256) void k_lmk_delta(const float* __restrict__ W, const float* __restrict__ dW,
                                                   float* __restrict__ delta) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    const float4* a = reinterpret_cast<const float4*>(W + (size_t)row * NY_DH);
    const float4* b = reinterpret_cast<const float4*>(dW + (size_t)row * NY_DH);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NY_DH / 4; ++j) {
        const float4 x = a[j], y = b[j];
        s += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
    }
    delta[row] = s;
}

// This kernel sits at 256 + 91 registers, and its time hangs on the loads the compiler hoists with them.  Of nystrom_tile.h it
// takes load32, zero16 and rtile_sum4, which leave its code as it was; the other steps stay written out, each marked with the
// part it repeats and what that part did to the build (same 160 MFMAs, same bits; the timings are in docs/lab_notes.md)
template <bool PACKED>
__device__ __forceinline__ void lmk_bwd_body(const float* qkv, const float* qL, const float* lse, const float* dW,
                                             const float* delta, float* dqkv, float* wsdq, const int32_t* tab, int nb,
                                             int total_blocks) {
    __shared__ float T[4][32 * NY_TLD];           // per wave: dS [query][key] of the current tile
    __shared__ float R[4][NY_DH * 32];            // per wave: its dQ^T [d][query] of the current tile
    const int c = blockIdx.x, hd = blockIdx.y;
    if constexpr (PACKED) {                       // two 128-key chunks per block; uniform per workgroup, ahead of every barrier
        const int bag = tm_packed_bag(tab, nb, total_blocks, c / (TM_PACKED_BLK / LA_BC));
        if (bag < 0) return;
        const size_t small = (size_t)bag * NY_H * NY_M * NY_DH, row = (size_t)bag * NY_H * NY_M;
        qL += small;
        dW += small;
        lse += row;
        delta += row;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const size_t key0 = (size_t)c * LA_BC + wave * 32;
    const float* krow = qkv + key0 * NY_QKV + NY_D + hd * NY_DH;      // K[key0][0] of this head; V is NY_D further
    float kr[32], vr[32];
    load32(krow + (size_t)r * NY_QKV + 32 * hh, kr);
    load32(krow + NY_D + (size_t)r * NY_QKV + 32 * hh, vr);
    f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();   // dK^T, dV^T [d][key]: key key0 + r
    const float* Qh = qL + (size_t)hd * NY_M * NY_DH;
    const float* dWh = dW + (size_t)hd * NY_M * NY_DH;
    const float* lseh = lse + hd * NY_M;
    const float* delh = delta + hd * NY_M;
    for (int qt = 0; qt < NY_M / 32; ++qt) {
        const int q0 = qt * 32;
        float a[32];
        load32(Qh + (q0 + r) * NY_DH + 32 * hh, a);
        // dot64_tile written out: with it 220 + 96 registers
        f32x16 s = zero16();                      // S [query q0 + mfma32_row(i, hh)][key key0 + r]
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], kr[kk], s, 0, 0, 0);
        load32(dWh + (q0 + r) * NY_DH + 32 * hh, a);
        f32x16 dp = zero16();                     // dP = dW V^T, same layout
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], vr[kk], dp, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = q0 + mfma32_row(i, hh);
            const float p = expf(s[i] - lseh[q]);
            s[i] = p;
            dp[i] = p * (dp[i] - delh[q]);        // dS
        }
        // dV^T [d][key] += dW^T [d][query] P [query][key], dK^T += Q^T dS: step i sums register i's two queries.  acc_rows twice,
        // written out as one loop: with every part taken from the header 189 + 96 registers and 178 us, not 139
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = q0 + mfma32_row(i, hh);
            const float* wq = dWh + q * NY_DH + r;
            const float* qq = Qh + q * NY_DH + r;
            dv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[0], s[i], dv0, 0, 0, 0);
            dv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq[32], s[i], dv1, 0, 0, 0);
            dk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qq[0], dp[i], dk0, 0, 0, 0);
            dk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qq[32], dp[i], dk1, 0, 0, 0);
        }
#pragma unroll                                    // tile_put written out: with it 256 + 94 registers
        for (int i = 0; i < 16; ++i) T[wave][mfma32_row(i, hh) * NY_TLD + r] = dp[i];
        __syncthreads();
        // dQ^T [d][query] = K^T [d][key] dS^T [key][query] over this wave's 32 keys: step t takes keys t and t + 16.  acc_tile_t
        // and rtile_put written out: with either the registers stay 256 + 91 but the schedule changes, and no run has timed it
        f32x16 g0 = zero16(), g1 = zero16();
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int kl = t + 16 * hh;
            const float b = T[wave][r * NY_TLD + kl];
            const float* kp = krow + (size_t)kl * NY_QKV + r;
            g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[0], b, g0, 0, 0, 0);
            g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[32], b, g1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int d = mfma32_row(i, hh);
            R[wave][d * 32 + r] = g0[i];
            R[wave][(d + 32) * 32 + r] = g1[i];
        }
        __syncthreads();
        rtile_sum4<256>(R, wsdq + (((size_t)c * NY_H + hd) * (NY_M / 32) + qt) * (NY_DH * 32), tid);
    }
    float* dkp = dqkv + (key0 + r) * NY_QKV + NY_D + hd * NY_DH;
#pragma unroll                                        // store_row64 twice, written out: with it 256 + 92 registers
    for (int g = 0; g < 4; ++g) {
        const int d = 8 * g + 4 * hh;             // registers 4 g .. 4 g + 3 are four consecutive d
        *reinterpret_cast<float4*>(dkp + d) = make_float4(dk0[4 * g], dk0[4 * g + 1], dk0[4 * g + 2], dk0[4 * g + 3]);
        *reinterpret_cast<float4*>(dkp + d + 32) = make_float4(dk1[4 * g], dk1[4 * g + 1], dk1[4 * g + 2], dk1[4 * g + 3]);
        *reinterpret_cast<float4*>(dkp + NY_D + d) = make_float4(dv0[4 * g], dv0[4 * g + 1], dv0[4 * g + 2], dv0[4 * g + 3]);
        *reinterpret_cast<float4*>(dkp + NY_D + d + 32) = make_float4(dv1[4 * g], dv1[4 * g + 1], dv1[4 * g + 2], dv1[4 * g + 3]);
    }
}

__global__ __launch_bounds__(256) void k_lmk_bwd(const float* __restrict__ qkv, const float* __restrict__ qL,
                                                 const float* __restrict__ lse, const float* __restrict__ dW,
                                                 const float* __restrict__ delta, float* __restrict__ dqkv,
                                                 float* __restrict__ wsdq) {
    lmk_bwd_body<false>(qkv, qL, lse, dW, delta, dqkv, wsdq, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void k_lmk_bwd_packed(const float* __restrict__ qkv, const float* __restrict__ qL,
                                                        const float* __restrict__ lse, const float* __restrict__ dW,
                                                        const float* __restrict__ delta, float* __restrict__ dqkv,
                                                        float* __restrict__ wsdq, const int32_t* __restrict__ tab, int nb,
                                                        int total_blocks) {
    lmk_bwd_body<true>(qkv, qL, lse, dW, delta, dqkv, wsdq, tab, nb, total_blocks);
}

}  // namespace

extern "C" {

size_t mil_tm_lmk_attn_ws_floats(int n_pad, int backward) {
    if (!ny_shape_ok(n_pad)) return 0;
    if (backward) return (size_t)NY_H * NY_M + (size_t)(n_pad / LA_BC) * NY_H * LA_DQPART;
    return (size_t)(n_pad / LA_FC) * NY_H * LA_FPART;
}

int mil_tm_lmk_attn_fwd(const float* qkv, const float* qL, int n_pad, float* W, float* lse, float* ws, void* stream) {
    if (!qkv || !qL || !W || !lse || !ws || !ny_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL)) return MIL_EINVAL;
    const int nc = n_pad / LA_FC;
    hipLaunchKernelGGL(k_lmk_fwd, dim3(nc, NY_H, NY_M / 64), dim3(128), 0, (hipStream_t)stream, qkv, qL, ws);
    hipLaunchKernelGGL(k_lmk_merge, dim3(NY_M / 32, NY_H), dim3(256), 0, (hipStream_t)stream, ws, nc, W, lse);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int mil_tm_lmk_attn_bwd(const float* qkv, const float* qL, const float* W, const float* lse, const float* dW, int n_pad,
                        float* dqkv, float* dqL, float* ws, void* stream) {
    if (!qkv || !qL || !W || !lse || !dW || !dqkv || !dqL || !ws || !ny_shape_ok(n_pad)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL) || !ny_aligned(W) || !ny_aligned(dW) || !ny_aligned(dqkv)) return MIL_EINVAL;
    const int nc = n_pad / LA_BC;
    float* wsdq = ws + NY_H * NY_M;
    hipLaunchKernelGGL(k_lmk_delta, dim3(NY_H * NY_M / 256), dim3(256), 0, (hipStream_t)stream, W, dW, ws);
    hipLaunchKernelGGL(k_lmk_bwd, dim3(nc, NY_H), dim3(256), 0, (hipStream_t)stream, qkv, qL, lse, dW, ws, dqkv, wsdq);
    hipLaunchKernelGGL(k_ny_reduce<1>, dim3(NY_M / 32, NY_H), dim3(256), 0, (hipStream_t)stream, wsdq, nc, dqL,
                       (float*)nullptr, TmPackedArg<false>{});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

size_t mil_tm_lmk_attn_packed_ws_floats(int total_blocks, int nb, int backward) {
    if (!tm_packed_ok(&nb, nb, total_blocks)) return 0;
    if (backward)
        return (size_t)nb * NY_H * NY_M + (size_t)total_blocks * (TM_PACKED_BLK / LA_BC) * NY_H * LA_DQPART;
    return (size_t)total_blocks * NY_H * LA_FPART;
}

int mil_tm_lmk_attn_fwd_packed(const float* qkv, const float* qL, float* W, float* lse, float* ws, const int32_t* blk_off, int nb,
                               int total_blocks, void* stream) {
    if (!qkv || !qL || !W || !lse || !ws || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_lmk_fwd_packed, dim3(total_blocks, NY_H, NY_M / 64), dim3(128), 0, (hipStream_t)stream, qkv, qL, ws,
                       blk_off, nb, total_blocks);
    hipLaunchKernelGGL(k_lmk_merge_packed, dim3(NY_M / 32, NY_H, nb), dim3(256), 0, (hipStream_t)stream, ws, blk_off, nb,
                       total_blocks, W, lse);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int mil_tm_lmk_attn_bwd_packed(const float* qkv, const float* qL, const float* W, const float* lse, const float* dW, float* dqkv,
                               float* dqL, float* ws, const int32_t* blk_off, int nb, int total_blocks, void* stream) {
    if (!qkv || !qL || !W || !lse || !dW || !dqkv || !dqL || !ws || !tm_packed_ok(blk_off, nb, total_blocks)) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL) || !ny_aligned(W) || !ny_aligned(dW) || !ny_aligned(dqkv)) return MIL_EINVAL;
    constexpr int per = TM_PACKED_BLK / LA_BC;          // backward chunks per block
    float* wsdq = ws + (size_t)nb * NY_H * NY_M;
    hipLaunchKernelGGL(k_lmk_delta, dim3(nb * (NY_H * NY_M / 256)), dim3(256), 0, (hipStream_t)stream, W, dW, ws);
    hipLaunchKernelGGL(k_lmk_bwd_packed, dim3(total_blocks * per, NY_H), dim3(256), 0, (hipStream_t)stream, qkv, qL, lse, dW, ws,
                       dqkv, wsdq, blk_off, nb, total_blocks);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ny_reduce<1, true>), dim3(NY_M / 32, NY_H, nb), dim3(256), 0, (hipStream_t)stream, wsdq,
                       per, dqL, (float*)nullptr, TmPackedArg<true>{blk_off, nb, total_blocks});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

}  // extern "C"
