// TransMIL: the tile parts of the two fused passes of the Nystrom core (csrc/landmark_attn.hip, csrc/token_attn.hip), once.
// Everything here is per wave on v_mfma_f32_32x32x2_f32: lane = (r = lane & 31, hh = lane >> 5), an f32x16 accumulator holds
// row mfma32_row(i, hh) in register i and column r on the lane.  All of it sits in the including file's anonymous namespace
// and is inlined (the one kernel is a template that each file instantiates for its own launch): nothing is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "tm_packed.h"

namespace {

constexpr int NY_H = 8, NY_DH = 64, NY_D = 512, NY_QKV = 3 * NY_D, NY_M = 256;
constexpr float NY_QSCALE = 0.125f;                 // 64^-0.5 = 2^-3: where it is applied does not change a bit
constexpr int NY_TLD = 33;                          // row stride of a 32 x 32 LDS tile

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

// A B^T [row of a][row of b] over 64 d: lane (r, hh) holds d = 32 hh .. 32 hh + 31 of row r of either operand, so one MFMA
// step pairs d with d + 32 (the order of a dot product's terms is free as long as both operands use the same one)
__device__ __forceinline__ f32x16 dot64_tile(const float (&a)[32], const float (&b)[32]) {
    f32x16 s = zero16();
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], s, 0, 0, 0);
    return s;
}

// One 32-key tile of scores s (keys down the registers, the query on the lane) into the running maximum m and sum l of the
// lane's query (l over this lane half's keys); s leaves as exp(s - m), o0 / o1 are rescaled to the new maximum
__device__ __forceinline__ void online_softmax_step(f32x16& s, float& m, float& l, f32x16& o0, f32x16& o1) {
    float tm = s[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) tm = fmaxf(tm, s[i]);
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);
    const float sc = expf(m - mn);              // 0 on the first tile (m = -inf)
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
}

// o0 / o1 [d][lane] += A^T [d][row] b [row][lane] (d, d + 32) with b straight back in as the B operand: step i sums the two
// rows mfma32_row(i, 0 | 1) that register i holds in the lane halves.  ap = &A[row 4 hh][r], LD = A's row stride
template <int LD>
__device__ __forceinline__ void acc_rows(const float* __restrict__ ap, const f32x16& b, f32x16& o0, f32x16& o1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float* ar = ap + (size_t)((i & 3) + 8 * (i >> 2)) * LD;
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[0], b[i], o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[32], b[i], o1, 0, 0, 0);
    }
}

// The round trip for a product that sums over the lane index: x into a 32 x NY_TLD LDS tile as [register row][lane] ..
__device__ __forceinline__ void tile_put(float* T, const f32x16& x, int r, int hh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) T[mfma32_row(i, hh) * NY_TLD + r] = x[i];
}
// .. and g0 / g1 [d][tile row] += A^T [d][lane index] T^T over the tile's 32 columns: step t takes columns t and t + 16.
// ap = &A[0][r], ld = A's row stride
__device__ __forceinline__ void acc_tile_t(const float* T, const float* __restrict__ ap, int ld, int r, int hh, f32x16& g0,
                                           f32x16& g1) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int kl = t + 16 * hh;
        const float b = T[r * NY_TLD + kl];
        const float* a = ap + (size_t)kl * ld;
        g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b, g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[32], b, g1, 0, 0, 0);
    }
}

// g0 / g1 into (add: onto) a [64][32] LDS slot; four slots summed as a tree by NT threads - the same order in every run
__device__ __forceinline__ void rtile_put(float* R, const f32x16& g0, const f32x16& g1, int r, int hh, bool add) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int d = mfma32_row(i, hh);
        if (add) {
            R[d * 32 + r] += g0[i];
            R[(d + 32) * 32 + r] += g1[i];
        } else {
            R[d * 32 + r] = g0[i];
            R[(d + 32) * 32 + r] = g1[i];
        }
    }
}
template <int NT>
__device__ __forceinline__ void rtile_sum4(const float (&R)[4][NY_DH * 32], float* __restrict__ out, int tid) {
#pragma unroll
    for (int j = 0; j < NY_DH * 32 / NT; ++j) {
        const int e = tid + NT * j;
        out[e] = (R[0][e] + R[1][e]) + (R[2][e] + R[3][e]);
    }
}

// An accumulator pair as the 64 d of the lane's row: p = &row[4 hh], registers 4 g .. 4 g + 3 are four consecutive d
__device__ __forceinline__ void store_row64(float* __restrict__ p, const f32x16& a0, const f32x16& a1, float scale) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(p + 8 * g) =
            make_float4(a0[4 * g] * scale, a0[4 * g + 1] * scale, a0[4 * g + 2] * scale, a0[4 * g + 3] * scale);
        *reinterpret_cast<float4*>(p + 8 * g + 32) =
            make_float4(a1[4 * g] * scale, a1[4 * g + 1] * scale, a1[4 * g + 2] * scale, a1[4 * g + 3] * scale);
    }
}

// Sums the partials [nc][8 heads][8 tiles][64 d][32] chunk 0, 1, 2 .. in that order into [8, 256, 64]: block = (tile, head,
// which of the NZ = gridDim.z partial sets, out0 | out1), element e = d * 32 + row of the tile, thread tid owns e = tid + 256 j.
// NZ is a template parameter because with one set the index of the set, read from blockIdx.z, cost its launch 0.2 of 20.7 us
// PACKED (csrc/tm_packed.h): blockIdx.z = set * nb + bag, the partials of a set lie over all bags' chunks, nc = the chunks per
// 256-row block; bag b's are summed alone, in ascending order, into slice b of the stacked [nb, 8, 256, 64] output - the terms
// and the order of the single-bag sum on that bag.  The kernel is templated as a whole, not built on a shared body: moved
// into a function its loop comes out with another addressing and two more registers.
template <int NZ, bool PACKED = false>
__global__ __launch_bounds__(256) void k_ny_reduce(const float* __restrict__ ws, int nc, float* __restrict__ out0,
                                                   float* __restrict__ out1, TmPackedArg<PACKED> pk = {}) {
    const int lt = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
    const float* p;
    float* dst;
    if constexpr (PACKED) {
        const int z = blockIdx.z, which = NZ > 1 ? z / pk.nb : 0, bag = z - which * pk.nb;
        int c0, c1;
        if (which >= NZ || !tm_packed_range(pk.tab, pk.total_blocks, bag, c0, c1)) return;
        const size_t part = (size_t)NY_H * NY_M * NY_DH;
        p = ws + ((size_t)which * pk.total_blocks + c0) * nc * part + ((size_t)hd * (NY_M / 32) + lt) * (NY_DH * 32);
        dst = (which ? out1 : out0) + (size_t)bag * part;
        nc *= c1 - c0;
    } else {
        const size_t set = NZ > 1 ? (size_t)blockIdx.z * nc * NY_H * NY_M * NY_DH : 0;
        p = ws + set + ((size_t)hd * (NY_M / 32) + lt) * (NY_DH * 32);
        dst = NZ > 1 && blockIdx.z ? out1 : out0;
    }
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int c = 0; c < nc; ++c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += p[tid + 256 * j];
        p += (size_t)NY_H * NY_M * NY_DH;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = tid + 256 * j;
        dst[((size_t)hd * NY_M + lt * 32 + (e & 31)) * NY_DH + (e >> 5)] = acc[j];
    }
}

inline bool ny_shape_ok(int n_pad) { return n_pad > 0 && n_pad % NY_M == 0; }
inline bool ny_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
