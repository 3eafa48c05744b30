// TransMIL: the cls token's per-patch attention straight from the operands of the two fused passes (csrc/landmark_attn.hip,
// csrc/token_attn.hip) - the cls row (padded row `pad`) of P = A1 Z A3 with neither A1 [8, n_pad, 256] nor A3 [8, 256, n_pad]
// in memory.  Per head h:
//     a1[m] = softmax_m(64^-0.5 q[pad] . kL[m])                       256 values
//     t     = a1 Z[h]                                                  256 values
//     r[j]  = sum_m t[m] exp(qL[m] . k[j] - lse3[m])                   j over the keys from column pad + 1 on
//     out[i] = r[pad + 1 + i] + (i < s^2 - N ? r[pad + 1 + N + i] : 0) for i < N, 0 for N <= i < s^2
// qL is the scaled landmark query (mil_tm_landmarks), kL is not scaled, lse3 is what mil_tm_lmk_attn_fwd returns, q and k are
// read in place from the merged [n_pad, 1536] rows.
//
//  k_clsf_t     workgroup = (64 columns of Z, head), as k_tm_cls_t of csrc/transmil.hip.  Each recomputes the head's 256 cls
//               scores (thread = landmark), softmaxes them in LDS and forms its 64 entries of t: the 16 KiB of kL that the
//               four workgroups of a head each re-read cost less than a launch of their own, and no lse1 is needed.
//  k_clsf_key   workgroup = (128-key chunk, head), 4 waves of 32 keys each.  A wave holds its 32 key rows in registers; per
//               32-landmark tile S = qL k^T on v_mfma_f32_32x32x2_f32 (the landmark down the accumulator registers, the key
//               on the lane - the orientation k_lmk_bwd has for P), then acc += t[m] expf(S - lse3[m]) on the VALU with the
//               head's t and lse3 staged in LDS once.  The tiles are summed 0 .. 7 and the registers 0 .. 15 in that order,
//               the two lane halves meet through one __shfl_xor(., 32): no atomics, two runs give the same bits.  The key
//               tiles that lie wholly in front of column pad + 1 are not launched.
//  k_clsf_fold  thread = (patch, head): the fold and the zeros from N on.  A launch of its own and not the key kernel's
//               epilogue: patch i's second key pad + 1 + N + i lies N keys further on, in general in another workgroup, so an
//               epilogue would need either atomics on out (which would cost the fixed order of the sum) or an order between
//               workgroups.  The launch reads 8 n_pad floats that are still in L2.
// N is the host `n`, or len_dev[bag] read on the device and clamped into the side's bucket exactly as k_tm_cls_row does; only
// the fold needs it.  Nothing is read on the host and nothing is allocated: the entry is capture-safe.
//
// mil_tm_cls_attn_packed: the same three kernels over ALL bags of a packed step (csrc/tm_packed.h) in one launch set.  The
// bag of a workgroup comes from the block table, its side and output offset from a second small table, its length from
// len_dev; t is [nb, 8, 256], r [8, 256 total_blocks] over the packed rows, out the bags' [8, s_b^2] one after another.  The
// grids follow from (nb, total_blocks) alone: t (4, 8, nb), key (2 total_blocks, 8), fold (total_blocks, 8).  A key's sum and
// a bag's t do not depend on the grid, so every bag's output has the bits of mil_tm_cls_attn_fused on its rows and slices.
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "nystrom_tile.h"
#include "tm_packed.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int CF_KC = 128;                          // keys per workgroup of k_clsf_key (4 waves x 32)
constexpr int CF_MAX_BAGS = 16;                     // as TM_MAX_BAGS of csrc/transmil.hip

// over the 64 lanes of a wave by a butterfly: every lane ends with the same value, formed in the same order in every run
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What a packed workgroup knows of its bag (csrc/tm_packed.h): the first block c0 and the block count l from the block table,
// the side s and the output offset off (in patches) from the cls table (ops.tm_cls_table: side [nb] | off [nb + 1]), and from
// these pad = 256 l - s^2 - 1.  false - the workgroup returns - for a block range outside [0, total_blocks], s < 1, pad outside
// [0, 256) or [off, off + s^2) outside the total_patches patches of out: whatever the tables hold, no address leaves the rows,
// the nb slices, the workspace or out.  Everything here is wave-uniform.
struct ClsfBag {
    int c0, l, s, S2, pad, off;
};
__device__ __forceinline__ bool clsf_bag(const int32_t* __restrict__ tab, const int32_t* __restrict__ ctab, int nb,
                                         int total_blocks, int total_patches, int bag, ClsfBag& g) {
    int c1;
    if (bag < 0 || bag >= nb || !tm_packed_range(tab, total_blocks, bag, g.c0, c1)) return false;
    g.l = c1 - g.c0;
    g.s = __builtin_amdgcn_readfirstlane(ctab[bag]);
    g.off = __builtin_amdgcn_readfirstlane(ctab[nb + bag]);
    if (g.s < 1 || g.s > 46340) return false;           // s^2 in an int
    g.S2 = g.s * g.s;
    const long pad = (long)TM_PACKED_BLK * g.l - g.S2 - 1;
    if (pad < 0 || pad >= TM_PACKED_BLK) return false;
    g.pad = (int)pad;
    return g.off >= 0 && g.off <= total_patches - g.S2;
}

// The table and the packed sizes as ONE trailing argument, empty in the single-bag kernels (as TmPackedArg)
template <bool PACKED>
struct ClsfArg {
    const int32_t *tab, *ctab;
    int nb, total_blocks, total_patches;
};
template <>
struct ClsfArg<false> {};

// The three kernels below are each one body with a single-bag and a packed instantiation: the packed one reads its bag's
// geometry off the tables and moves the pointers to the bag's rows and slices; every sum keeps its terms and their order.
// packed: blockIdx.z = the bag; t is [nb, 8, 256]
template <bool PACKED>
__global__ __launch_bounds__(256) void k_clsf_t(const float* __restrict__ qkv, const float* __restrict__ kL,
                                                const float* __restrict__ Z, int pad, float* __restrict__ t, ClsfArg<PACKED> pk) {
    __shared__ float q[NY_DH];
    __shared__ float a[NY_M];
    __shared__ float red[4][64];
    if constexpr (PACKED) {                         // uniform per workgroup, ahead of every barrier
        ClsfBag g;
        if (!clsf_bag(pk.tab, pk.ctab, pk.nb, pk.total_blocks, pk.total_patches, blockIdx.z, g)) return;
        pad = g.pad;
        qkv += (size_t)g.c0 * TM_PACKED_BLK * NY_QKV;
        kL += (size_t)blockIdx.z * NY_H * NY_M * NY_DH;
        Z += (size_t)blockIdx.z * NY_H * NY_M * NY_M;
        t += (size_t)blockIdx.z * NY_H * NY_M;
    }
    const int hd = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < NY_DH) q[tid] = qkv[(size_t)pad * NY_QKV + hd * NY_DH + tid] * NY_QSCALE;    // row pad holds the unscaled q
    __syncthreads();
    const float4* kr = reinterpret_cast<const float4*>(kL + ((size_t)hd * NY_M + tid) * NY_DH);
    float sc = 0.f;                                 // the score of landmark tid
#pragma unroll
    for (int j = 0; j < NY_DH / 4; ++j) {
        const float4 x = kr[j];
        sc += (q[4 * j] * x.x + q[4 * j + 1] * x.y) + (q[4 * j + 2] * x.z + q[4 * j + 3] * x.w);
    }
    const float wm = wave_max(sc);
    if (lane == 0) red[wv][0] = wm;
    __syncthreads();
    const float mx = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    const float e = expf(sc - mx);
    const float wsum = wave_sum(e);
    if (lane == 0) red[wv][1] = wsum;
    __syncthreads();
    a[tid] = e / ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1]));
    __syncthreads();
    // t[j] = sum_k a[k] Z[k][j]: wave wv sums k in [64 wv, 64 wv + 64), the four partial sums are added in a fixed order
    const int j = blockIdx.x * 64 + lane;
    const float* z = Z + ((size_t)hd * NY_M + 64 * wv) * NY_M + j;
    const float* aw = a + 64 * wv;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) s += aw[k] * z[k * NY_M];
    red[wv][lane] = s;
    __syncthreads();
    if (wv == 0) t[hd * NY_M + j] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// tile0: the first 32-key tile that holds a column from pad + 1 on; r [8, n_pad] gets the keys from 32 tile0 on.
// packed: blockIdx.x = a 128-key chunk of the packed rows - half a block, so inside one bag -, n_pad = all 256 total_blocks rows
// and r [8, n_pad] is indexed by the packed row.  A chunk that lies wholly in front of its bag's column pad + 1 returns ahead of
// the barrier; a wave whose tile does returns behind it, where the single-bag kernel drops its spare waves.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_clsf_key(const float* __restrict__ qkv, const float* __restrict__ qL,
                                                  const float* __restrict__ t, const float* __restrict__ lse3, int n_pad,
                                                  int tile0, float* __restrict__ r_ws, ClsfArg<PACKED> pk) {
    __shared__ float ts[NY_M], ls[NY_M];
    const int hd = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    int tile = tile0 + (CF_KC / 32) * blockIdx.x + wave;
    if constexpr (PACKED) {
        const int blk = blockIdx.x / (TM_PACKED_BLK / CF_KC);
        const int bag = tm_packed_bag(pk.tab, pk.nb, pk.total_blocks, blk);
        ClsfBag g;
        if (bag < 0 || !clsf_bag(pk.tab, pk.ctab, pk.nb, pk.total_blocks, pk.total_patches, bag, g)) return;
        if (blk < g.c0 || blk >= g.c0 + g.l) return;               // a table whose two halves disagree
        const int first = g.c0 * (TM_PACKED_BLK / 32) + (g.pad + 1) / 32;      // the bag's first tile with a column from pad + 1 on
        if ((CF_KC / 32) * (int)blockIdx.x + CF_KC / 32 <= first) return;
        tile = (CF_KC / 32) * blockIdx.x + wave;
        tile0 = first;
        qL += (size_t)bag * NY_H * NY_M * NY_DH;
        t += (size_t)bag * NY_H * NY_M;
        lse3 += (size_t)bag * NY_H * NY_M;
    }
    ts[tid] = t[hd * NY_M + tid];
    ls[tid] = lse3[hd * NY_M + tid];
    __syncthreads();
    if (tile >= n_pad / 32) return;                 // the last workgroup's spare waves; no barrier follows
    if constexpr (PACKED) {
        if (tile < tile0) return;
    }
    const size_t key0 = (size_t)tile * 32;
    float kr[32];
    load32(qkv + (key0 + r) * NY_QKV + NY_D + hd * NY_DH + 32 * hh, kr);
    const float* Qh = qL + (size_t)hd * NY_M * NY_DH;
    float acc = 0.f;                                // of key key0 + r, over this lane half's landmarks
    for (int qt = 0; qt < NY_M / 32; ++qt) {
        float a[32];
        load32(Qh + (32 * qt + r) * NY_DH + 32 * hh, a);
        const f32x16 s = dot64_tile(a, kr);         // S [landmark 32 qt + mfma32_row(i, hh)][key key0 + r]
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = 32 * qt + mfma32_row(i, hh);
            acc += ts[m] * expf(s[i] - ls[m]);
        }
    }
    acc += __shfl_xor(acc, 32, 64);
    if (hh == 0) r_ws[(size_t)hd * n_pad + key0 + r] = acc;
}

// packed: blockIdx.x = a 256-row block; block k of bag b folds the patches 256 (k - c0) + tid < s^2 of that bag, the length is
// len_dev[b], and the bag's [8, s^2] lies at float 8 off of out.  n_pad = all 256 total_blocks rows, as in k_clsf_key.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_clsf_fold(const float* __restrict__ r_ws, int n_pad, int pad, int s, int n_host,
                                                   const int32_t* __restrict__ len_dev, int bag, float* __restrict__ out,
                                                   ClsfArg<PACKED> pk) {
    int blk = blockIdx.x;
    if constexpr (PACKED) {
        bag = tm_packed_bag(pk.tab, pk.nb, pk.total_blocks, blk);
        ClsfBag g;
        if (bag < 0 || !clsf_bag(pk.tab, pk.ctab, pk.nb, pk.total_blocks, pk.total_patches, bag, g)) return;
        if (blk < g.c0 || blk >= g.c0 + g.l) return;               // a table whose two halves disagree
        blk -= g.c0;
        s = g.s;
        pad = g.pad;
        r_ws += (size_t)g.c0 * TM_PACKED_BLK;
        out += (size_t)NY_H * g.off;
    }
    const int S2 = s * s;
    const int N = len_dev != nullptr ? min(max(len_dev[bag], (s - 1) * (s - 1) + 1), S2) : n_host;
    const int add = S2 - N;
    const int hd = blockIdx.y, i = blk * 256 + threadIdx.x;
    if (i >= S2) return;
    const float* row = r_ws + (size_t)hd * n_pad + pad + 1;     // the S2 sequence keys: i < N and N + i < S2 stay inside
    float v = 0.f;
    if (i < N) {
        v = row[i];
        if (i < add) v += row[N + i];
    }
    out[(size_t)hd * S2 + i] = v;
}

}  // namespace

extern "C" {

size_t mil_tm_cls_attn_fused_ws_floats(int n_pad) {
    if (!ny_shape_ok(n_pad)) return 0;
    return (size_t)NY_H * NY_M + (size_t)NY_H * n_pad;          // t [8, 256] | r [8, n_pad]
}

int mil_tm_cls_attn_fused(const float* qkv, const float* qL, const float* kL, const float* Z, const float* lse3, int n_pad,
                          int pad, int s, int n, const int32_t* len_dev, int bag, float* ws, float* out, void* stream) {
    if (!qkv || !qL || !kL || !Z || !lse3 || !ws || !out || !ny_shape_ok(n_pad) || s < 1 || s > 4096) return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL) || !ny_aligned(kL)) return MIL_EINVAL;     // read as float4
    const long S2 = (long)s * s;
    if (pad < 0 || (long)pad + 1 + S2 != n_pad) return MIL_EINVAL;
    if (len_dev != nullptr ? (bag < 0 || bag >= CF_MAX_BAGS) : (n > S2 || n <= (long)(s - 1) * (s - 1))) return MIL_EINVAL;
    float* t = ws;
    float* r_ws = ws + NY_H * NY_M;
    const int tile0 = (pad + 1) / 32, tiles = n_pad / 32 - tile0;                     // pad + 1 < n_pad: tiles >= 1
    hipLaunchKernelGGL(k_clsf_t<false>, dim3(NY_M / 64, NY_H), dim3(256), 0, (hipStream_t)stream, qkv, kL, Z, pad, t,
                       ClsfArg<false>{});
    hipLaunchKernelGGL(k_clsf_key<false>, dim3((tiles + CF_KC / 32 - 1) / (CF_KC / 32), NY_H), dim3(256), 0, (hipStream_t)stream,
                       qkv, qL, t, lse3, n_pad, tile0, r_ws, ClsfArg<false>{});
    hipLaunchKernelGGL(k_clsf_fold<false>, dim3((unsigned)((S2 + 255) / 256), NY_H), dim3(256), 0, (hipStream_t)stream, r_ws, n_pad,
                       pad, s, n, len_dev, bag, out, ClsfArg<false>{});
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

size_t mil_tm_cls_attn_packed_ws_floats(int total_blocks, int nb) {
    if (!tm_packed_ok(&nb, nb, total_blocks)) return 0;
    return (size_t)nb * NY_H * NY_M + (size_t)NY_H * TM_PACKED_BLK * total_blocks;      // t [nb, 8, 256] | r [8, 256 total_blocks]
}

int mil_tm_cls_attn_packed(const float* qkv, const float* qL, const float* kL, const float* Z, const float* lse3,
                           const int32_t* cls_tab, int total_patches, const int32_t* len_dev, float* ws, float* out,
                           const int32_t* blk_off, int nb, int total_blocks, void* stream) {
    if (!qkv || !qL || !kL || !Z || !lse3 || !cls_tab || !len_dev || !ws || !out || !tm_packed_ok(blk_off, nb, total_blocks))
        return MIL_EINVAL;
    if (!ny_aligned(qkv) || !ny_aligned(qL) || !ny_aligned(kL)) return MIL_EINVAL;     // read as float4
    // every bag has 1 <= s^2 < 256 l: nb <= sum s^2 < 256 total_blocks
    if (total_patches < nb || total_patches >= (long)TM_PACKED_BLK * total_blocks) return MIL_EINVAL;
    float* t = ws;
    float* r_ws = ws + (size_t)nb * NY_H * NY_M;
    const int R = TM_PACKED_BLK * total_blocks;
    const ClsfArg<true> pk{blk_off, cls_tab, nb, total_blocks, total_patches};
    hipLaunchKernelGGL(k_clsf_t<true>, dim3(NY_M / 64, NY_H, nb), dim3(256), 0, (hipStream_t)stream, qkv, kL, Z, 0, t, pk);
    hipLaunchKernelGGL(k_clsf_key<true>, dim3(total_blocks * (TM_PACKED_BLK / CF_KC), NY_H), dim3(256), 0, (hipStream_t)stream,
                       qkv, qL, t, lse3, R, 0, r_ws, pk);
    hipLaunchKernelGGL(k_clsf_fold<true>, dim3(total_blocks, NY_H), dim3(256), 0, (hipStream_t)stream, r_ws, R, 0, 0, 0, len_dev,
                       0, out, pk);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

}  // extern "C"
