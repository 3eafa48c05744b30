// K1b: the attention pool of the gated-attention MIL pooling (ABMIL) for gfx950 - scores -> softmax over the bag -> A.x, and
// ds in the backward.
//
// Reference arithmetic: model/dim1/ABMIL.py:57-59 (forward), torch autograd of the same ops (backward).  These stages
// stream x once: HBM-bound.  The gate GEMMs around them: gate_fwd.hip, gate_bwd_dw.hip,
// gate_bwd_dx.hip.
#include "mil_common.h"

// ================================================================================ K1b attention pool forward
// One workgroup (256 threads) per tile of <= 32 rows of one bag.  Wave w streams rows w, w+4, ...;
// lane l owns columns 4l + 256q (16-byte loads, 1 KiB per wave instruction).
// Output partial: acc[t][L] weighted row sum with weights exp(s_i - m_tile) in partials[0 .. T*L),
// then (m_tile, l_tile) pairs in partials[T*L + 2t ..].
// Optional by-product (Wf != NULL, C <= 4): h[row][c] = x_row . Wf[c], the head's projection of every patch.  The
// backward then needs no second pass over x: x_i . dM = sum_c dz[bag][c] h[i][c] because dM = dz Wf
// (k_pool_ds_from_h replaces the 64 MiB read of k_pool_bwd_ds).
// Train mode: xbits keeps (ABMIL.py:49: the DROPPED x is what gets pooled, :59) - lane l owns columns 4l + 256q, i.e. bits
// 4 (l & 7).. of word 8q + (l >> 3) of its row; the survivors' scale rides on the softmax weight.  mbits / mscale: the
// head's Dropout(.25) on the bag embedding (aggregator.py:129) folds into the head rows used for the by-product
// h[row][c] = x_row . (Wf[c] * keepM[bag] * mscale), so that x_i . dM = sum_c dz_c h[i][c] still holds in the backward.
// NT: x is larger than the Infinity Cache, so the pass is a pure HBM stream: nontemporal loads (tools/cu_load_bw.hip: a
// streaming read of 512 MB runs at 7.2 TB/s with the hint, 6.5 TB/s without).  Off when x fits the cache and the
// weight-gradient pass re-reads it from there.
template <int NQ, bool NT>
__global__ __launch_bounds__(256) void k_pool_partial(const float* __restrict__ x, const float* __restrict__ scores,
                                                      const int32_t* __restrict__ tile_map, float* __restrict__ partials,
                                                      int L, const float* __restrict__ Wf, int C,
                                                      float* __restrict__ hrow, const uint32_t* __restrict__ xbits,
                                                      float xscale, const uint32_t* __restrict__ mbits, float mscale) {
    __shared__ float p_lds[MIL_POOL_TILE];
    __shared__ float ml_lds[2];
    __shared__ __attribute__((aligned(16))) float red[3 * NQ * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x;
    const int row0 = tile_map[4 * t + 1], nrows = tile_map[4 * t + 2];

    f32x4 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = f32x4{0, 0, 0, 0};
    // Rows past the tile end are clamped to its last row and carry weight 0 (p_lds is 0 there): the
    // loop is branch-free, so all 8 x NQ 16-byte loads of a wave are in flight together - and they are issued BEFORE the
    // tile's softmax weights are formed (below), whose score load + two wave reductions then run under the x stream.
    f32x4 v[MIL_POOL_TILE / 4][NQ];
    unsigned mk[MIL_POOL_TILE / 4][NQ];
#pragma unroll
    for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
        const int rr = max(min(wave + 4 * i, nrows - 1), 0);      // nrows == 0: a padding tile of a device-built map
        const float* xr = x + (size_t)(row0 + rr) * L + 4 * lane;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            v[i][q] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + 256 * q)) : *reinterpret_cast<const f32x4*>(xr + 256 * q);
        if (xbits != nullptr) {
            const uint32_t* mr = xbits + (size_t)(row0 + rr) * (L >> 5) + (lane >> 3);
#pragma unroll
            for (int q = 0; q < NQ; ++q) mk[i][q] = mr[8 * q];
        }
    }
    if (wave == 0) {
        const float s = lane < nrows ? scores[row0 + lane] : -INFINITY;
        const float m = wave_allmax(s);
        const float p = lane < nrows ? expf(s - m) : 0.f;
        const float l = wave_allsum(p);
        if (lane < MIL_POOL_TILE) p_lds[lane] = p;
        if (lane == 0) { ml_lds[0] = m; ml_lds[1] = l; }
    }
    __syncthreads();
    if (xbits != nullptr) {
        const int sh = 4 * (lane & 7);
#pragma unroll
        for (int i = 0; i < MIL_POOL_TILE / 4; ++i)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const unsigned m = mk[i][q] >> sh;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[i][q][e] = keep_if(v[i][q][e], m, e);
            }
    } else {
        xscale = 1.0f;
    }
#pragma unroll
    for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
        const float p = p_lds[wave + 4 * i] * xscale;
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] += p * v[i][q];
    }
    // head rows as this tile's bag sees them: x scale and the head's dropout mask folded in
    const int bag_ = tile_map[4 * t];
    auto head_row = [&](int c, int q) {
        f32x4 w = *reinterpret_cast<const f32x4*>(Wf + (size_t)c * L + 256 * q + 4 * lane) * xscale;
        if (mbits != nullptr) {
            const unsigned m = mbits[(size_t)bag_ * (L >> 5) + 8 * q + (lane >> 3)] >> (4 * (lane & 7));
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = keep_if(w[e], m, e) * mscale;
        }
        return w;
    };
    if (Wf != nullptr && C == 2) {
        // two classes (the usual head): the tile's 8 x 2 dot products of this wave go through ONE 16-value reduction
        float d16[16];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            f32x4 wf[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) wf[q] = head_row(c, q);
#pragma unroll
            for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    d += v[i][q][0] * wf[q][0] + v[i][q][1] * wf[q][1] + v[i][q][2] * wf[q][2] + v[i][q][3] * wf[q][3];
                d16[2 * i + c] = d;
            }
        }
        const float tot = wave_reduce16(d16, lane);
        const int k = wave_reduce16_index(lane), rr = wave + 4 * (k >> 1);
        if ((lane & 3) == 0 && rr < nrows) hrow[(size_t)(row0 + rr) * 2 + (k & 1)] = tot;
    } else if (Wf != nullptr) {
        for (int c = 0; c < C; ++c) {
            f32x4 wf[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) wf[q] = head_row(c, q);
#pragma unroll
            for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    d += v[i][q][0] * wf[q][0] + v[i][q][1] * wf[q][1] + v[i][q][2] * wf[q][2] + v[i][q][3] * wf[q][3];
                d = wave_allsum(d);
                const int rr = wave + 4 * i;
                if (lane == 0 && rr < nrows) hrow[(size_t)(row0 + rr) * C + c] = d;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            *reinterpret_cast<f32x4*>(red + ((wave - 1) * NQ + q) * 256 + 4 * lane) = acc[q];
    }
    __syncthreads();
    if (wave == 0) {
        float* out = partials + (size_t)t * L;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x4 v = acc[q];
#pragma unroll
            for (int w = 0; w < 3; ++w) v += *reinterpret_cast<const f32x4*>(red + (w * NQ + q) * 256 + 4 * lane);
            *reinterpret_cast<f32x4*>(out + 256 * q + 4 * lane) = v;
        }
        if (lane == 0) {
            float* ml = partials + (size_t)gridDim.x * L + 2 * t;
            ml[0] = ml_lds[0];
            ml[1] = ml_lds[1];
        }
    }
}

// Merge the tile partials of one bag: M = sum_t e^{m_t - m} acc_t / sum_t e^{m_t - m} l_t.
// grid = (B, L / 128): workgroup (b, cb) owns 128 columns of bag b; thread (g, c4): float4 column c4 < 32,
// tile group g < 8, tile loads unrolled 4 deep (the kernel is latency-bound, so many loads in flight
// and 4x more workgroups than bags).
__global__ __launch_bounds__(256) void k_pool_merge(const float* __restrict__ partials,
                                                    const int32_t* __restrict__ bag_tile_off, float* __restrict__ M,
                                                    float* __restrict__ lse, int L, int T) {
    __shared__ float red[4];
    __shared__ float scale_lds[1024];
    __shared__ __attribute__((aligned(16))) float part_lds[8 * 128];
    const int b = blockIdx.x, cb = blockIdx.y, tid = threadIdx.x;
    const int t0 = bag_tile_off[b], t1 = bag_tile_off[b + 1], nt = t1 - t0;
    const float* ml = partials + (size_t)T * L;
    float m = -INFINITY;
    for (int t = t0 + tid; t < t1; t += 256) m = fmaxf(m, ml[2 * t]);
    m = wave_allmax(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float l = 0.f;
    for (int t = t0 + tid; t < t1; t += 256) l += ml[2 * t + 1] * expf(ml[2 * t] - m);
    l = wave_allsum(l);
    if ((tid & 63) == 0) red[tid >> 6] = l;
    __syncthreads();
    l = red[0] + red[1] + red[2] + red[3];
    const float inv = nt > 0 ? 1.0f / l : 0.f;

    const int c4 = tid & 31, g = tid >> 5;
    const float* base = partials + 128 * cb + 4 * c4;
    f32x4 acc = {0, 0, 0, 0};
    for (int tb = 0; tb < nt; tb += 1024) {
        __syncthreads();
        for (int k = tid; k < 1024; k += 256) scale_lds[k] = (tb + k < nt) ? expf(ml[2 * (t0 + tb + k)] - m) : 0.f;
        __syncthreads();
        const int cnt = min(1024, nt - tb);
        int k = g;
        for (; k + 24 < cnt; k += 32) {
            f32x4 v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const f32x4*>(base + (size_t)(t0 + tb + k + 8 * e) * L);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += scale_lds[k + 8 * e] * v[e];
        }
        for (; k < cnt; k += 8) acc += scale_lds[k] * *reinterpret_cast<const f32x4*>(base + (size_t)(t0 + tb + k) * L);
    }
    *reinterpret_cast<f32x4*>(part_lds + g * 128 + 4 * c4) = acc;
    __syncthreads();
    if (tid < 128) {
        float v = 0.f;
#pragma unroll
        for (int gg = 0; gg < 8; ++gg) v += part_lds[gg * 128 + tid];
        M[(size_t)b * L + 128 * cb + tid] = v * inv;
    }
    if (tid == 0 && cb == 0) lse[b] = nt > 0 ? m + logf(l) : -INFINITY;
}

// ================================================================================ K1 backward: ds (HBM-bound)
// ds_i = A_i (x_i . dM - cdot),  A_i = exp(s_i - lse).  Optionally dx_i = A_i dM (the pool term).
template <int NQ>
__global__ __launch_bounds__(256) void k_pool_bwd_ds(const float* __restrict__ x, const float* __restrict__ scores,
                                                     const float* __restrict__ lse, const float* __restrict__ dM,
                                                     const float* __restrict__ cdot,
                                                     const int32_t* __restrict__ tile_map, float* __restrict__ ds,
                                                     float* __restrict__ dx, int L, const uint32_t* __restrict__ xbits,
                                                     float xscale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x;
    const int bag = tile_map[4 * t], row0 = tile_map[4 * t + 1], nrows = tile_map[4 * t + 2];
    constexpr bool NT = false;
    if (xbits == nullptr) xscale = 1.0f;
    f32x4 g[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) g[q] = *reinterpret_cast<const f32x4*>(dM + (size_t)bag * L + 256 * q + 4 * lane);
    const float lse_b = lse[bag], c_b = cdot[bag];
    // branch-free loads (rows past the tile end clamp to its last row), guarded stores
    f32x4 v[MIL_POOL_TILE / 4][NQ];
    unsigned mk[MIL_POOL_TILE / 4][NQ];
    float sc[MIL_POOL_TILE / 4];
    const int sh = 4 * (lane & 7);
#pragma unroll
    for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
        const size_t row = (size_t)(row0 + max(min(wave + 4 * i, nrows - 1), 0));
        const float* xr = x + row * L + 4 * lane;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            v[i][q] = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + 256 * q)) : *reinterpret_cast<const f32x4*>(xr + 256 * q);
        if (xbits != nullptr) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) mk[i][q] = xbits[row * (L >> 5) + 8 * q + (lane >> 3)] >> sh;
        }
        sc[i] = scores[row];
    }
#pragma unroll
    for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
        const int rr = wave + 4 * i;
        float dot = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x4 xv = v[i][q];
            if (xbits != nullptr) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = keep_if(xv[e], mk[i][q], e);
            }
            dot += xv[0] * g[q][0] + xv[1] * g[q][1] + xv[2] * g[q][2] + xv[3] * g[q][3];
        }
        dot = wave_allsum(dot) * xscale;
        const float a = expf(sc[i] - lse_b);
        if (rr < nrows) {
            const size_t row = (size_t)(row0 + rr);
            if (lane == 0) ds[row] = a * (dot - c_b);
            if (dx != nullptr) {
                // the pool term of the gradient of the (dropped) rows; the dropout's own backward (mask, scale) is applied
                // once, by the last writer of dx (k_gate_bwd_dx)
                float* dr = dx + row * L + 4 * lane;
#pragma unroll
                for (int q = 0; q < NQ; ++q) *reinterpret_cast<f32x4*>(dr + 256 * q) = a * g[q];
            }
        }
    }
}

// ds_i = A_i (sum_c dz[bag][c] h[i][c] - cdot[bag]) from the forward's head projections: no pass over x.
// 8 tiles per workgroup, 32 threads per tile.
__global__ __launch_bounds__(256) void k_pool_ds_from_h(const float* __restrict__ scores, const float* __restrict__ lse,
                                                        const float* __restrict__ hrow, const float* __restrict__ dz,
                                                        const float* __restrict__ cdot,
                                                        const int32_t* __restrict__ tile_map, int T, int C,
                                                        float* __restrict__ ds) {
    const int t = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;
    if (t >= T) return;
    const int bag = tile_map[4 * t], row0 = tile_map[4 * t + 1], nrows = tile_map[4 * t + 2];
    if (l >= nrows) return;
    const size_t row = (size_t)(row0 + l);
    float g = 0.f;
    for (int c = 0; c < C; ++c) g += dz[bag * C + c] * hrow[row * C + c];
    ds[row] = expf(scores[row] - lse[bag]) * (g - cdot[bag]);
}

// ================================================================================ host side
static int launch_pool_partial(const float* x, const float* scores, const int32_t* tile_map, int T, int L,
                               float* partials, const float* Wf, int C, float* hrow, hipStream_t st,
                               const uint32_t* xbits = nullptr, float xscale = 1.0f, const uint32_t* mbits = nullptr,
                               float mscale = 1.0f) {
    if (T <= 0) return MIL_OK;
    const bool nt = (size_t)T * MIL_POOL_TILE * L * sizeof(float) > MIL_STREAM_BYTES;
#define POOL_LAUNCH(NQ_) do { \
        if (nt) hipLaunchKernelGGL((k_pool_partial<NQ_, true>), dim3(T), dim3(256), 0, st, x, scores, tile_map, partials, L, Wf, C, hrow, xbits, xscale, mbits, mscale); \
        else hipLaunchKernelGGL((k_pool_partial<NQ_, false>), dim3(T), dim3(256), 0, st, x, scores, tile_map, partials, L, Wf, C, hrow, xbits, xscale, mbits, mscale); } while (0)
    switch (L / 256) {
        case 1: POOL_LAUNCH(1); break;
        case 2: POOL_LAUNCH(2); break;
        case 3: POOL_LAUNCH(3); break;
        default: POOL_LAUNCH(4); break;
    }
#undef POOL_LAUNCH
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// Tile map on the device (ragged batches whose lengths change every step): one workgroup scans the B bag lengths and
// writes tile_map [T_cap][4], bag_tile_off [B + 1] and rows_out [1] = total rows.  Tiles beyond the last real one are
// padding: {0, 0, 0, 0} (the pool kernels emit a neutral partial for nrows == 0).  T_cap >= sum ceil(len / 32).
__global__ __launch_bounds__(256) void k_build_tile_map(const int32_t* __restrict__ bag_len, int B, int32_t* __restrict__ tile_map,
                                                        int32_t* __restrict__ bag_tile_off, int32_t* __restrict__ rows_out,
                                                        int T_cap) {
    build_tile_map_block(bag_len, B, tile_map, bag_tile_off, rows_out, T_cap);
}

extern "C" int mil_build_tile_map(const int32_t* bag_len, int B, int32_t* tile_map, int32_t* bag_tile_off, int32_t* rows_out,
                                  int T_cap, void* stream) {
    if (!bag_len || !tile_map || !bag_tile_off || !rows_out || B <= 0 || B > 1024 || T_cap < 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_build_tile_map, dim3(1), dim3(256), 0, (hipStream_t)stream, bag_len, B, tile_map, bag_tile_off, rows_out,
                       T_cap);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_attn_pool_partial_h(const float* x, const float* scores, const int32_t* tile_map, int T, int L,
                                       float* partials, const float* Wf, int C, float* hrow, const uint32_t* xbits,
                                       float xscale, const uint32_t* mbits, float mscale, void* stream) {
    if (!x || !scores || !tile_map || !partials || !Wf || !hrow) return MIL_EINVAL;
    if (L <= 0 || (L % 256) != 0 || L > 1024 || T < 0 || C <= 0 || C > 4) return MIL_EINVAL;
    return launch_pool_partial(x, scores, tile_map, T, L, partials, Wf, C, hrow, (hipStream_t)stream, xbits, xscale, mbits,
                               mscale);
}

extern "C" int mil_attn_pool_bwd_from_h(const float* scores, const float* lse, const float* hrow, const float* dz,
                                        const float* cdot, const int32_t* tile_map, int T, int C, float* ds, void* stream) {
    if (!scores || !lse || !hrow || !dz || !cdot || !tile_map || !ds || T < 0 || C <= 0 || C > 4) return MIL_EINVAL;
    if (T == 0) return MIL_OK;
    hipLaunchKernelGGL(k_pool_ds_from_h, dim3((T + 7) / 8), dim3(256), 0, (hipStream_t)stream, scores, lse, hrow, dz, cdot,
                       tile_map, T, C, ds);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_attn_pool_partial(const float* x, const float* scores, const int32_t* tile_map, int T, int L,
                                     float* partials, const uint32_t* xbits, float xscale, void* stream) {
    if (!x || !scores || !tile_map || !partials) return MIL_EINVAL;
    if (L <= 0 || (L % 256) != 0 || L > 1024 || T < 0) return MIL_EINVAL;
    return launch_pool_partial(x, scores, tile_map, T, L, partials, nullptr, 0, nullptr, (hipStream_t)stream, xbits, xscale);
}

extern "C" int mil_attn_pool_fwd(const float* x, const float* scores, const int32_t* tile_map,
                                 const int32_t* bag_tile_off, int T, int B, int L, float* partials, float* M,
                                 float* lse, const uint32_t* xbits, float xscale, void* stream) {
    if (!x || !scores || !tile_map || !bag_tile_off || !partials || !M || !lse) return MIL_EINVAL;
    if (L <= 0 || (L % 256) != 0 || L > 1024 || B < 0 || T < 0) return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_pool_partial(x, scores, tile_map, T, L, partials, nullptr, 0, nullptr, st, xbits, xscale);
    if (rc != MIL_OK) return rc;
    if (B > 0) {
        hipLaunchKernelGGL(k_pool_merge, dim3(B, L / 128), dim3(256), 0, st, partials, bag_tile_off, M, lse, L, T);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_attn_pool_bwd(const float* x, const float* scores, const float* lse, const float* dM,
                                 const float* cdot, const int32_t* tile_map, int T, int L, float* ds, float* dx,
                                 const uint32_t* xbits, float xscale, void* stream) {
    if (!x || !scores || !lse || !dM || !cdot || !tile_map || !ds) return MIL_EINVAL;
    if (L <= 0 || (L % 256) != 0 || L > 1024 || T < 0) return MIL_EINVAL;
    if (T == 0) return MIL_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (L / 256) {
        case 1: hipLaunchKernelGGL(k_pool_bwd_ds<1>, dim3(T), dim3(256), 0, st, x, scores, lse, dM, cdot, tile_map, ds, dx, L, xbits, xscale); break;
        case 2: hipLaunchKernelGGL(k_pool_bwd_ds<2>, dim3(T), dim3(256), 0, st, x, scores, lse, dM, cdot, tile_map, ds, dx, L, xbits, xscale); break;
        case 3: hipLaunchKernelGGL(k_pool_bwd_ds<3>, dim3(T), dim3(256), 0, st, x, scores, lse, dM, cdot, tile_map, ds, dx, L, xbits, xscale); break;
        default: hipLaunchKernelGGL(k_pool_bwd_ds<4>, dim3(T), dim3(256), 0, st, x, scores, lse, dM, cdot, tile_map, ds, dx, L, xbits, xscale); break;
    }
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// ================================================================================ softmax weights of a bag
// w[n] = exp(s_n - lse) over the rows [row_off[b], row_off[b + 1]) of bag b: the weights k_pool_partial folds into the pooled
// sum and never writes.  One workgroup per bag, two passes over its scores (a few KB, L2-resident): per-thread online
// (max, sum), merged over the wave and then over the four waves in wave order - a fixed order, the same bits every run -
// then the weights.  len_dev (nullable): the bag's true length on the device; the rows behind it inside the slot get zero.
__global__ __launch_bounds__(256) void k_bag_softmax(const float* __restrict__ scores, const int32_t* __restrict__ row_off,
                                                     const int32_t* __restrict__ len_dev, float* __restrict__ w) {
    __shared__ float m_lds[4], l_lds[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int r0 = row_off[b], cap = row_off[b + 1] - r0;
    const int n = len_dev != nullptr ? max(min(len_dev[b], cap), 0) : cap;
    float m = -INFINITY, l = 0.f;
    for (int i = tid; i < n; i += 256) {
        const float s = scores[r0 + i];
        if (s > m) { l = l * expf(m - s) + 1.0f; m = s; }
        else l += expf(s - m);
    }
    const float mw = wave_allmax(m);
    l = wave_allsum(m == -INFINITY ? 0.f : l * expf(m - mw));
    if ((tid & 63) == 0) { m_lds[tid >> 6] = mw; l_lds[tid >> 6] = l; }
    __syncthreads();
    const float mt = fmaxf(fmaxf(m_lds[0], m_lds[1]), fmaxf(m_lds[2], m_lds[3]));
    float lt = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) lt += m_lds[k] == -INFINITY ? 0.f : l_lds[k] * expf(m_lds[k] - mt);
    const float inv = 1.0f / lt;
    for (int i = tid; i < cap; i += 256) w[r0 + i] = i < n ? expf(scores[r0 + i] - mt) * inv : 0.f;
}

extern "C" int mil_bag_softmax(const float* scores, const int32_t* row_off, const int32_t* len_dev, int B, float* w,
                               void* stream) {
    if (!scores || !row_off || !w || B < 0) return MIL_EINVAL;
    if (B == 0) return MIL_OK;
    hipLaunchKernelGGL(k_bag_softmax, dim3(B), dim3(256), 0, (hipStream_t)stream, scores, row_off, len_dev, w);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// The same weights over a CAPACITY BUCKET (segments.FusionBucket): a bag's rows are scattered - its patch rows inside the
// `cap` block, one piece per tail segment behind it - and its length lives on the device, so the rows of bag b are named by
// its tiles [bag_tile_off[b], bag_tile_off[b + 1]) of the bucket's 32-row map {bag, row0, nrows, 0}.  Workgroup b < B walks
// those tiles twice (eight tiles per sweep, one row per thread): per-thread online (max, sum), merged over the wave and then
// over the four waves in wave order - the order is fixed by the map alone, the same bits every run -, then the weights.
// Workgroups >= B write the 0 of the rows no bag owns (row_bag < 0): no tile names them, so no row has two writers.
__global__ __launch_bounds__(256) void k_bag_softmax_rows(const float* __restrict__ scores, const int32_t* __restrict__ tile_map,
                                                          const int32_t* __restrict__ bag_tile_off, int T,
                                                          const int32_t* __restrict__ row_bag, int B, int R,
                                                          float* __restrict__ w) {
    __shared__ float m_lds[4], l_lds[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= B) {
        const int nz = gridDim.x - B;
        for (int r = ((int)blockIdx.x - B) * 256 + tid; r < R; r += nz * 256)
            if (row_bag[r] < 0) w[r] = 0.f;
        return;
    }
    const int b = blockIdx.x;
    const int t0 = max(bag_tile_off[b], 0), t1 = min(bag_tile_off[b + 1], T);
    const int sub = tid / MIL_POOL_TILE, lane = tid % MIL_POOL_TILE;
    constexpr int SWEEP = 256 / MIL_POOL_TILE;
    float m = -INFINITY, l = 0.f;
    for (int t = t0 + sub; t < t1; t += SWEEP) {
        const int4 tm = reinterpret_cast<const int4*>(tile_map)[t];
        const int row = tm.y + lane;
        if (lane < tm.z && row >= 0 && row < R) {
            const float s = scores[row];
            if (s > m) { l = l * expf(m - s) + 1.0f; m = s; }
            else l += expf(s - m);
        }
    }
    const float mw = wave_allmax(m);
    l = wave_allsum(m == -INFINITY ? 0.f : l * expf(m - mw));
    if ((tid & 63) == 0) { m_lds[tid >> 6] = mw; l_lds[tid >> 6] = l; }
    __syncthreads();
    const float mt = fmaxf(fmaxf(m_lds[0], m_lds[1]), fmaxf(m_lds[2], m_lds[3]));
    float lt = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) lt += m_lds[k] == -INFINITY ? 0.f : l_lds[k] * expf(m_lds[k] - mt);
    const float inv = 1.0f / lt;
    for (int t = t0 + sub; t < t1; t += SWEEP) {
        const int4 tm = reinterpret_cast<const int4*>(tile_map)[t];
        const int row = tm.y + lane;
        if (lane < tm.z && row >= 0 && row < R) w[row] = expf(scores[row] - mt) * inv;
    }
}

extern "C" int mil_bag_softmax_rows(const float* scores, const int32_t* tile_map, const int32_t* bag_tile_off, int T,
                                    const int32_t* row_bag, int B, int R, float* w, void* stream) {
    if (!scores || !tile_map || !bag_tile_off || !row_bag || !w || B < 0 || B > 1024 || T < 0 || R < 0) return MIL_EINVAL;
    if (B == 0 || R == 0) return MIL_OK;
    const int nz = min((R + 255) / 256, 64);
    hipLaunchKernelGGL(k_bag_softmax_rows, dim3(B + nz), dim3(256), 0, (hipStream_t)stream, scores, tile_map, bag_tile_off, T,
                       row_bag, B, R, w);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
