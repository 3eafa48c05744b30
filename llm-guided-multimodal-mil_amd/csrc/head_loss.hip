// K3b: per-bag classifier head, sigmoid, BCE loss and their backward; Adam step.
// Reference: model/aggregator.py:128-131,200 (fc = Dropout(.25) + Linear(512, C), sigmoid),
// train_ddp.py:99,323-324 (BCELoss), train_ddp.py:115-118 (Adam).  All tiny, latency-bound kernels.
#include "mil_internal.h"

template <int NT>
__device__ __forceinline__ float block_allsum_nt(float v, float* red) {
    const int tid = threadIdx.x;
    v = wave_allsum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ float block_allsum_256(float v, float* red) {
    const int tid = threadIdx.x;
    v = wave_allsum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// z[b][c] = M[b] . Wf[c] + bf[c];  p = sigmoid(z).   grid = B, 256 threads.
__global__ __launch_bounds__(256) void k_head_fwd(const float* __restrict__ M, const float* __restrict__ Wf,
                                                  const float* __restrict__ bf, float* __restrict__ z,
                                                  float* __restrict__ p, int L, int C) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        float v = 0.f;
        for (int j = tid; j < L; j += 256) v += M[(size_t)b * L + j] * Wf[(size_t)c * L + j];
        v = block_allsum_256(v, red);
        if (tid == 0) {
            const float zz = v + bf[c];
            z[b * C + c] = zz;
            p[b * C + c] = 1.0f / (1.0f + expf(-zz));
        }
    }
}

// BCE(mean) forward + gradient through the sigmoid.  One workgroup.
__global__ __launch_bounds__(256) void k_bce_fwd_bwd(const float* __restrict__ p, const float* __restrict__ y,
                                                     float* __restrict__ loss_sum, float* __restrict__ dz, int n,
                                                     float scale) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float pi = p[i], yi = y[i];
        const float lp = fmaxf(logf(pi), -100.0f);
        const float l1p = fmaxf(logf(1.0f - pi), -100.0f);
        acc += -(yi * lp + (1.0f - yi) * l1p);
        dz[i] = (pi - yi) * scale;
    }
    acc = block_allsum_256(acc, red);
    if (threadIdx.x == 0) atomicAdd(loss_sum, acc * scale);
}

// dM[b] = dz[b] Wf;  cdot[b] = M[b] . dM[b].   grid = B, 256 threads.
__global__ __launch_bounds__(256) void k_head_bwd_dm(const float* __restrict__ dz_or_dp, const float* __restrict__ p,
                                                     const float* __restrict__ M, const float* __restrict__ Wf,
                                                     float* __restrict__ dM, float* __restrict__ cdot, int L, int C) {
    __shared__ float red[4];
    __shared__ float dzs[32];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < C) {
        float g = dz_or_dp[b * C + tid];
        if (p != nullptr) { const float pp = p[b * C + tid]; g = g * pp * (1.0f - pp); }
        dzs[tid] = g;
    }
    __syncthreads();
    float dot = 0.f;
    for (int j = tid; j < L; j += 256) {
        float v = 0.f;
        for (int c = 0; c < C; ++c) v += dzs[c] * Wf[(size_t)c * L + j];
        dM[(size_t)b * L + j] = v;
        dot += v * M[(size_t)b * L + j];
    }
    dot = block_allsum_256(dot, red);
    if (tid == 0) cdot[b] = dot;
}

// dWf[c][j] = sum_b dz[b][c] M[b][j];  dbf[c] = sum_b dz[b][c];  loss_out[0] = sum_b loss_bag[b].
// grid = C * ceil(L / 64) + 1 workgroups of 256 threads = 64 columns x 4 bag lanes; the last workgroup does the
// bias gradient and the loss.  dz_or_dp / p as in mil_head_bwd.
__global__ __launch_bounds__(256) void k_head_bwd_params(const float* __restrict__ dz_or_dp, const float* __restrict__ p,
                                                         const float* __restrict__ M, float* __restrict__ dWf,
                                                         float* __restrict__ dbf, int B, int L, int C,
                                                         const float* __restrict__ loss_bag, float* __restrict__ loss_out,
                                                         int accumulate) {
    __shared__ float red[4][64];
    const int nlb = (L + 63) / 64;
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    if ((int)blockIdx.x < C * nlb) {
        const int c = blockIdx.x / nlb, j = (blockIdx.x % nlb) * 64 + lane;
        float v = 0.f;
        if (j < L)
            for (int b = g; b < B; b += 4) {
                float gz = dz_or_dp[b * C + c];
                if (p != nullptr) { const float pp = p[b * C + c]; gz = gz * pp * (1.0f - pp); }
                v += gz * M[(size_t)b * L + j];
            }
        red[g][lane] = v;
        __syncthreads();
        if (g == 0 && j < L) {
            const float t = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
            dWf[(size_t)c * L + j] = accumulate ? dWf[(size_t)c * L + j] + t : t;
        }
    } else {
        // bias gradients: thread t < C sums over the bags; the loss: wave 1 sums loss_bag
        if ((int)threadIdx.x < C) {
            const int c = threadIdx.x;
            float v = 0.f;
            for (int b = 0; b < B; ++b) {
                float gz = dz_or_dp[b * C + c];
                if (p != nullptr) { const float pp = p[b * C + c]; gz = gz * pp * (1.0f - pp); }
                v += gz;
            }
            dbf[c] = accumulate ? dbf[c] + v : v;
        }
        if (loss_bag != nullptr && g == 1) {
            float v = 0.f;
            for (int b = lane; b < B; b += 64) v += loss_bag[b];
            v = wave_allsum(v);
            if (lane == 0) loss_out[0] = accumulate ? loss_out[0] + v : v;
        }
    }
}

// torch.optim.Adam, weight decay folded into the gradient (L2), bias-corrected.  Four elements per thread; the
// bias corrections come from the host (step known there) or, for a step that is replayed from a hipGraph, from
// a device-side counter (step_dev holds the number of steps ALREADY taken).

template <int AD_U>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ param, const float* __restrict__ grad,
                                              float* __restrict__ m, float* __restrict__ v, size_t n, float lr, float b1,
                                              float b2, float eps, float wd, float gscale, float bc1, float bc2_sqrt,
                                              const int* __restrict__ step_dev, const float* __restrict__ lr_dev) {
    __shared__ float bc[2];
    if (step_dev != nullptr) {
        if (threadIdx.x == 0) {
            const double st = (double)(*step_dev + 1);
            bc[0] = (float)(1.0 - pow((double)b1, st));
            bc[1] = (float)sqrt(1.0 - pow((double)b2, st));
        }
        __syncthreads();
        bc1 = bc[0];
        bc2_sqrt = bc[1];
    }
    if (lr_dev != nullptr) lr = *lr_dev;            // a schedule writes it between two replays of one captured graph
    const float lr_bc1 = lr / bc1;
    // workgroup = 256 threads x AD_U float4 each; the AD_U x 4 loads of a thread are issued before any arithmetic
    // (a 4-stream pass with one float4 in flight per stream and thread left the HBM pipe half empty: 3.4 TB/s)
    const size_t base = (size_t)blockIdx.x * (256 * 4 * AD_U);
    if (base + 256 * 4 * AD_U <= n) {
        f32x4 p4[AD_U], g4[AD_U], m4[AD_U], v4[AD_U];
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const size_t i = base + ((size_t)u * 256 + threadIdx.x) * 4;
            p4[u] = *reinterpret_cast<const f32x4*>(param + i);
            g4[u] = *reinterpret_cast<const f32x4*>(grad + i);
            m4[u] = *reinterpret_cast<const f32x4*>(m + i);
            v4[u] = *reinterpret_cast<const f32x4*>(v + i);
        }
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const size_t i = base + ((size_t)u * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p4[u][e], me = m4[u][e], ve = v4[u][e];
                adam_one(pe, g4[u][e], me, ve, lr_bc1, b1, b2, eps, wd, gscale, bc2_sqrt);
                p4[u][e] = pe; m4[u][e] = me; v4[u][e] = ve;
            }
            *reinterpret_cast<f32x4*>(param + i) = p4[u];
            *reinterpret_cast<f32x4*>(m + i) = m4[u];
            *reinterpret_cast<f32x4*>(v + i) = v4[u];
        }
    } else {
        for (size_t j = base + threadIdx.x; j < n; j += 256) {
            float pe = param[j], me = m[j], ve = v[j];
            adam_one(pe, grad[j], me, ve, lr_bc1, b1, b2, eps, wd, gscale, bc2_sqrt);
            param[j] = pe; m[j] = me; v[j] = ve;
        }
    }
}
__global__ void k_step_inc(int* step_dev) { *step_dev += 1; }

// Adam over up to MIL_ADAM_MAX_SEGS contiguous ranges of one flat buffer AND the advance of the device step counter in ONE
// launch (optim.FlatAdam: parameters that received no gradient are skipped, as torch.optim.Adam skips them, so the live part
// of the buffer is a few ranges - three launches plus a one-thread increment per fusion step before).  Every workgroup reads
// the step number when it starts; the counter may only move once all of them have, so each workgroup signs off on `done`
// when it ends and the last one advances the step and clears `done` for the next launch (replay-safe: no host reset).
struct AdamSegs {
    int nseg;
    unsigned blk_end[MIL_ADAM_MAX_SEGS];      // exclusive prefix of workgroups per range
    unsigned long long begin[MIL_ADAM_MAX_SEGS], end[MIL_ADAM_MAX_SEGS];
};
__global__ __launch_bounds__(256) void k_adam_segs(float* __restrict__ param, const float* __restrict__ grad,
                                                   float* __restrict__ m, float* __restrict__ v, const AdamSegs sg, float b1,
                                                   float b2, float eps, float wd, float gscale, int* __restrict__ step_dev,
                                                   const float* __restrict__ lr_dev, int* __restrict__ done, int inc) {
    __shared__ float bc[2];
    if (threadIdx.x == 0) {
        const double st = (double)(__hip_atomic_load(step_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1);
        bc[0] = (float)(1.0 - pow((double)b1, st));
        bc[1] = (float)sqrt(1.0 - pow((double)b2, st));
    }
    __syncthreads();
    const float lr_bc1 = *lr_dev / bc[0], bc2_sqrt = bc[1];
    int sI = 0;
    while (sI + 1 < sg.nseg && blockIdx.x >= sg.blk_end[sI]) ++sI;
    const unsigned b0 = sI == 0 ? 0u : sg.blk_end[sI - 1];
    constexpr int AD_U = 4;
    const size_t base = (size_t)sg.begin[sI] + (size_t)(blockIdx.x - b0) * (256 * 4 * AD_U), n = (size_t)sg.end[sI];
    if (base + 256 * 4 * AD_U <= n) {
        f32x4 p4[AD_U], g4[AD_U], m4[AD_U], v4[AD_U];
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const size_t i = base + ((size_t)u * 256 + threadIdx.x) * 4;
            p4[u] = *reinterpret_cast<const f32x4*>(param + i);
            g4[u] = *reinterpret_cast<const f32x4*>(grad + i);
            m4[u] = *reinterpret_cast<const f32x4*>(m + i);
            v4[u] = *reinterpret_cast<const f32x4*>(v + i);
        }
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
            const size_t i = base + ((size_t)u * 256 + threadIdx.x) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p4[u][e], me = m4[u][e], ve = v4[u][e];
                adam_one(pe, g4[u][e], me, ve, lr_bc1, b1, b2, eps, wd, gscale, bc2_sqrt);
                p4[u][e] = pe; m4[u][e] = me; v4[u][e] = ve;
            }
            *reinterpret_cast<f32x4*>(param + i) = p4[u];
            *reinterpret_cast<f32x4*>(m + i) = m4[u];
            *reinterpret_cast<f32x4*>(v + i) = v4[u];
        }
    } else {
        for (size_t j = base + threadIdx.x; j < n; j += 256) {
            float pe = param[j], me = m[j], ve = v[j];
            adam_one(pe, grad[j], me, ve, lr_bc1, b1, b2, eps, wd, gscale, bc2_sqrt);
            param[j] = pe; m[j] = me; v[j] = ve;
        }
    }
    if (inc) {
        __syncthreads();                         // thread 0 read the step long ago; nothing else of this workgroup needs it
        if (threadIdx.x == 0) {
            const int prev = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == (int)gridDim.x - 1) {    // every workgroup has started (and read the step): advance it
                __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(step_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
__global__ void k_counter_add(int* ctr, int v) { *ctr += v; }
// Up to 8 int32 values handed over AS KERNEL ARGUMENTS (the per-step bag lengths of a capacity bucket: a 4-byte
// hipMemcpyAsync from pageable memory showed up as a 4.7 us blit kernel behind an 8.7 us gap in front of every replay).
struct SetI32Args { int32_t v[8]; };
__global__ void k_set_i32(int32_t* dst, int n, SetI32Args a) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = a.v[threadIdx.x];
}
extern "C" int mil_set_i32(int32_t* dst, const int32_t* values_host, int n, void* stream) {
    if (!dst || !values_host || n < 0 || n > 8) return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    SetI32Args a{};
    for (int i = 0; i < n; ++i) a.v[i] = values_host[i];
    hipLaunchKernelGGL(k_set_i32, dim3(1), dim3(64), 0, (hipStream_t)stream, dst, n, a);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
extern "C" int mil_counter_add(int32_t* counter, int v, void* stream) {
    if (!counter) return MIL_EINVAL;
    hipLaunchKernelGGL(k_counter_add, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, v);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// ---------------------------------------------------------------------------------------------
// Fused per-bag tail of the forward and head of the backward (one workgroup per bag):
//   merge the attention-pool tile partials -> M, lse        (ABMIL.py:57-59)
//   z = M Wf^T + bf, p = sigmoid(z)                         (aggregator.py:128-131,200)
//   if labels: loss_bag[b] = BCE(p_b, y_b) * scale, dz = (p - y) * scale, dM = dz Wf, cdot = M . dM
// Thread (g, c4): column float4 c4 < L/4, tile group g < 256/(L/4); tile loads are unrolled 8 deep
// so one workgroup keeps ~8 x 4 KiB in flight (the kernel is latency-bound: B workgroups only).
template <int NT>
__global__ __launch_bounds__(NT) void k_pool_merge_head(const float* __restrict__ partials,
                                                         const int32_t* __restrict__ bag_tile_off, int T, int L,
                                                         const float* __restrict__ Wf, const float* __restrict__ bf,
                                                         int C, const float* __restrict__ y, float scale,
                                                         float* __restrict__ M, float* __restrict__ lse,
                                                         float* __restrict__ z, float* __restrict__ p,
                                                         float* __restrict__ loss_sum, float* __restrict__ dz,
                                                         float* __restrict__ dM, float* __restrict__ cdot,
                                                         const int32_t* __restrict__ tile_map,
                                                         const float* __restrict__ scores, const float* __restrict__ hrow,
                                                         float* __restrict__ ds, const uint32_t* __restrict__ mbits,
                                                         float mscale, float* __restrict__ Mdrop, int loss_kind) {
    // mbits [B][L/32]: keep bits of the head's Dropout(.25) on the bag embedding (aggregator.py:129; train mode).  M stays
    // the un-dropped ABMIL output, Mdrop = M * keep * mscale feeds the head (and dWf); dM = d loss / d M carries the mask.
    // Latency-bound (one workgroup per bag, a chain of reductions): every load that does not depend on the chain - keep
    // words, the tile statistics, the head rows of the thread's columns, the rows of the ds pass - is issued before the
    // first barrier, and the C head dot products share one block reduction.
    constexpr int NW = NT / 64;
    constexpr int JP = 1024 / NT;                 // columns per thread (L <= 1024)
    constexpr int DSP = 4;                        // ds passes whose operands are loaded up front (NT / 32 tiles per pass)
    __shared__ float red[NW][4];
    __shared__ float scale_lds[1024];
    __shared__ __attribute__((aligned(16))) float m_lds[1024];
    __shared__ __attribute__((aligned(16))) float part_lds[4 * 1024];
    __shared__ float keep_lds[1024];
    __shared__ float dzs[32];
    __shared__ float ps[32];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t0 = bag_tile_off[b], t1 = bag_tile_off[b + 1], nt = t1 - t0;
    const float* ml = partials + (size_t)T * L;
    const bool fastC = C <= 4;
    // ---- loads that do not depend on the merge
    float mt = -INFINITY, lt = 0.f;
    if (tid < nt) { mt = ml[2 * (t0 + tid)]; lt = ml[2 * (t0 + tid) + 1]; }
    float keepv[JP], wf[JP][4];
#pragma unroll
    for (int q = 0; q < JP; ++q) {
        const int j = tid + q * NT;
        keepv[q] = 1.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) wf[q][c] = 0.f;
        if (j < L) {
            if (mbits != nullptr) keepv[q] = ((mbits[(size_t)b * (L >> 5) + (j >> 5)] >> (j & 31)) & 1u) ? mscale : 0.f;
            if (fastC)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) wf[q][c] = Wf[(size_t)c * L + j];
        }
    }
    int ds_row[DSP];
    float ds_sc[DSP], ds_h[DSP][4];
#pragma unroll
    for (int k = 0; k < DSP; ++k) {
        ds_row[k] = -1;
        ds_sc[k] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) ds_h[k][c] = 0.f;
    }
    if (ds != nullptr && y != nullptr && fastC) {
#pragma unroll
        for (int k = 0; k < DSP; ++k) {
            const int g8 = t0 + (tid >> 5) + k * (NT / 32);
            if (g8 < t1) {
                const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
                if (lr < nrows) ds_row[k] = row0 + lr;
            }
        }
#pragma unroll
        for (int k = 0; k < DSP; ++k)
            if (ds_row[k] >= 0) {
                ds_sc[k] = scores[ds_row[k]];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < C) ds_h[k][c] = hrow[(size_t)ds_row[k] * C + c];
            }
    }
#pragma unroll
    for (int q = 0; q < JP; ++q)
        if (tid + q * NT < L) keep_lds[tid + q * NT] = keepv[q];
    // ---- global max / normaliser over the bag's tiles
    float m = mt;
    for (int t = t0 + tid + NT; t < t1; t += NT) m = fmaxf(m, ml[2 * t]);
    m = wave_allmax(m);
    if (lane == 0) red[wv][0] = m;
    __syncthreads();
    m = red[0][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w][0]);
    const float sc0 = tid < nt ? expf(mt - m) : 0.f;
    float l = lt * sc0;
    for (int t = t0 + tid + NT; t < t1; t += NT) l += ml[2 * t + 1] * expf(ml[2 * t] - m);
    l = wave_allsum(l);
    __syncthreads();                               // red[.][0] of the max has been read by everyone
    if (lane == 0) red[wv][0] = l;
    scale_lds[tid] = sc0;                          // first chunk of tile weights: this thread's tile
    for (int k = tid + NT; k < 1024; k += NT) scale_lds[k] = (k < nt) ? expf(ml[2 * (t0 + k)] - m) : 0.f;
    __syncthreads();
    l = red[0][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) l += red[w][0];
    const float inv = nt > 0 ? 1.0f / l : 0.f;

    const int L4 = L >> 2, NG = NT / L4;          // NT = 256: L in {256, 512, 768, 1024} -> NG in {4, 2, 1, 1}; NT = 1024: 4x
    const int c4 = tid % L4, g = tid / L4;
    const bool worker = g < NG;                    // L = 768 leaves 64 threads without a column group
    f32x4 acc = {0, 0, 0, 0};
    for (int tb = 0; tb < nt; tb += 1024) {
        if (tb > 0) {
            __syncthreads();
            for (int k = tid; k < 1024; k += NT) scale_lds[k] = (tb + k < nt) ? expf(ml[2 * (t0 + tb + k)] - m) : 0.f;
            __syncthreads();
        }
        const int cnt = worker ? min(1024, nt - tb) : 0;
        int k = g;
        for (; k + 7 * NG < cnt; k += 8 * NG) {
            f32x4 v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                v[e] = *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + tb + k + e * NG) * L + 4 * c4);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += scale_lds[k + e * NG] * v[e];
        }
        for (; k < cnt; k += NG)
            acc += scale_lds[k] * *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + tb + k) * L + 4 * c4);
    }
    if (worker) *reinterpret_cast<f32x4*>(part_lds + g * L + 4 * c4) = acc;
    __syncthreads();
    float mv[JP];
    float hd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < JP; ++q) {
        const int j = tid + q * NT;
        mv[q] = 0.f;
        if (j < L) {
            float v = 0.f;
            for (int gg = 0; gg < NG; ++gg) v += part_lds[gg * L + j];
            v *= inv;
            mv[q] = v;
            m_lds[j] = v;
            M[(size_t)b * L + j] = v;
            if (Mdrop != nullptr) Mdrop[(size_t)b * L + j] = v * keepv[q];
#pragma unroll
            for (int c = 0; c < 4; ++c) hd[c] += v * keepv[q] * wf[q][c];
        }
    }
    if (tid == 0) lse[b] = nt > 0 ? m + logf(l) : -INFINITY;
    // ---- head: the C dot products through one block reduction (C <= 4), else one at a time
    if (fastC) {
#pragma unroll
        for (int c = 0; c < 4; ++c) hd[c] = wave_allsum(hd[c]);
        __syncthreads();                           // red[.][0] of the normaliser has been read by everyone
        if (lane == 0)
#pragma unroll
            for (int c = 0; c < 4; ++c) red[wv][c] = hd[c];
        __syncthreads();
        if (tid < C) {
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) v += red[w][tid];
            const float zz = v + bf[tid];
            const float pp = 1.0f / (1.0f + expf(-zz));
            z[b * C + tid] = zz;
            p[b * C + tid] = pp;
            ps[tid] = pp;
        }
    } else {
        __syncthreads();
        for (int c = 0; c < C; ++c) {
            float v = 0.f;
            for (int j = tid; j < L; j += NT) v += m_lds[j] * keep_lds[j] * Wf[(size_t)c * L + j];
            v = wave_allsum(v);
            __syncthreads();
            if (lane == 0) red[wv][0] = v;
            __syncthreads();
            if (tid == 0) {
                float t = 0.f;
                for (int w = 0; w < NW; ++w) t += red[w][0];
                const float zz = t + bf[c];
                const float pp = 1.0f / (1.0f + expf(-zz));
                z[b * C + c] = zz;
                p[b * C + c] = pp;
                ps[c] = pp;
            }
        }
    }
    if (y == nullptr) return;
    __syncthreads();
    if (tid == 0) {
        float lossacc = 0.f;
        if (loss_kind == 0) {
            // BCELoss on the sigmoid outputs vs one-hot float labels (train_ddp.py:98,323-324); log clamped at -100
            for (int c = 0; c < C; ++c) {
                const float pp = ps[c], yy = y[b * C + c];
                lossacc += -(yy * fmaxf(logf(pp), -100.0f) + (1.0f - yy) * fmaxf(logf(1.0f - pp), -100.0f));
                const float d = (pp - yy) * scale;
                dz[b * C + c] = d;
                dzs[c] = d;
            }
        } else {
            // num_classes > 2: the reference switches to CrossEntropyLoss and applies it to the module's SIGMOID outputs
            // with the float one-hot labels as class probabilities (train_ddp.py:95-96,323-324):
            //   loss_b = -sum_c y_c log softmax(p)_c;  d loss / d p_c = softmax(p)_c sum_k y_k - y_c;  dz = dp p (1 - p)
            float mx = -INFINITY, se = 0.f, sy = 0.f;
            for (int c = 0; c < C; ++c) mx = fmaxf(mx, ps[c]);
            for (int c = 0; c < C; ++c) se += expf(ps[c] - mx);
            const float lse_p = mx + logf(se);
            for (int c = 0; c < C; ++c) {
                const float yy = y[b * C + c];
                sy += yy;
                lossacc += -yy * (ps[c] - lse_p);
            }
            for (int c = 0; c < C; ++c) {
                const float pp = ps[c], q = expf(pp - lse_p);
                const float d = (q * sy - y[b * C + c]) * scale * pp * (1.0f - pp);
                dz[b * C + c] = d;
                dzs[c] = d;
            }
        }
        loss_sum[b] = lossacc * scale;              // per-bag loss; summed (fixed order) by k_head_bwd_params
    }
    __syncthreads();
    float dot = 0.f;
    if (fastC) {
        float dzr[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) dzr[c] = c < C ? dzs[c] : 0.f;
#pragma unroll
        for (int q = 0; q < JP; ++q) {
            const int j = tid + q * NT;
            if (j < L) {
                float v = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) v += dzr[c] * wf[q][c];
                v *= keepv[q];
                dM[(size_t)b * L + j] = v;
                dot += v * mv[q];
            }
        }
    } else {
        for (int j = tid; j < L; j += NT) {
            float v = 0.f;
            for (int c = 0; c < C; ++c) v += dzs[c] * Wf[(size_t)c * L + j];
            v *= keep_lds[j];
            dM[(size_t)b * L + j] = v;
            dot += v * m_lds[j];
        }
    }
    dot = wave_allsum(dot);
    if (lane == 0) red[wv][1] = dot;               // column 1: column 0 may still be read by a slow wave of the head stage
    __syncthreads();
    dot = red[0][1];
#pragma unroll
    for (int w = 1; w < NW; ++w) dot += red[w][1];
    if (tid == 0) cdot[b] = dot;
    if (ds != nullptr) {
        // the score gradient of this bag's rows from the forward's head projections (k_pool_ds_from_h, fused here: every
        // quantity it needs - lse, dz, M . dM - was just formed by this workgroup):  ds_i = A_i (sum_c dz_c h_i[c] - M . dM)
        const float lse_b = m + logf(l);
        int k0 = 0;
        if (fastC) {
#pragma unroll
            for (int k = 0; k < DSP; ++k)
                if (ds_row[k] >= 0) {
                    float gd = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) gd += dzs[c < C ? c : 0] * (c < C ? ds_h[k][c] : 0.f);
                    ds[ds_row[k]] = expf(ds_sc[k] - lse_b) * (gd - dot);
                }
            k0 = DSP;
        }
        for (int g8 = t0 + (tid >> 5) + k0 * (NT / 32); g8 < t1; g8 += NT / 32) {
            const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
            if (lr < nrows) {
                const size_t row = (size_t)(row0 + lr);
                float gd = 0.f;
                for (int c = 0; c < C; ++c) gd += dzs[c] * hrow[row * C + c];
                ds[row] = expf(scores[row] - lse_b) * (gd - dot);
            }
        }
    }
}

// The same per-bag tail split over TWO workgroups per bag that run side by side (round 3; C <= 4, labels, hrow and ds
// present - the training step).  k_pool_merge_head walks  tile statistics -> m -> l -> merge of the partials (64 KB per
// bag) -> M -> head dot products -> z -> loss -> dz -> M . dM -> ds  through nine barriers in one workgroup, but nothing the
// backward waits for needs M:
//     z_c - bf_c = sum_n a_n h_n[c]            (h_n[c] = x~_n . (Wf[c] keep_b mscale), the pool pass's by-product)
//     M . dM     = sum_c dz_c (z_c - bf_c)     (dM = dz Wf keep)
//     ds_n       = a_n (sum_c dz_c h_n[c] - M . dM)
// blockIdx.y = 0: row scores -> m -> {l, sum e_n h_n[c]} -> (per thread) z, p, loss, dz, cdot -> ds, dM: two block
// reductions over values the threads already hold.  blockIdx.y = 1: the merge of the partials -> M, Mdrop (what the
// head's weight gradient reads).  z is now the weighted sum of the rows' projections instead of the projection of the
// weighted sum: the same number up to summation order (1e-7); a first version that did both halves in ONE workgroup, chain
// first, was slower than k_pool_merge_head (13.3 vs 12.3 us in the step) - the next kernel waits for the launch, not for ds.
// AW (the deferred pool, gate_route_plan): launched with gridDim.y = 1, the chain half alone - nothing merges partials or
// writes M here - and it stores the row weights a_n = e_n / l to arow [R]: the weight-gradient launch forms M from them.
template <int NT, bool AW = false>
__global__ __launch_bounds__(NT) void k_pool_tail_h(const float* __restrict__ partials, const int32_t* __restrict__ bag_tile_off,
                                                     int T, int L, const float* __restrict__ Wf, const float* __restrict__ bf,
                                                     int C, const float* __restrict__ y, float scale, float* __restrict__ M,
                                                     float* __restrict__ lse, float* __restrict__ z, float* __restrict__ p,
                                                     float* __restrict__ loss_sum, float* __restrict__ dz,
                                                     float* __restrict__ dM, float* __restrict__ cdot,
                                                     const int32_t* __restrict__ tile_map, const float* __restrict__ scores,
                                                     const float* __restrict__ hrow, float* __restrict__ ds,
                                                     const uint32_t* __restrict__ mbits, float mscale,
                                                     float* __restrict__ Mdrop, int loss_kind,
                                                     float* __restrict__ arow = nullptr) {
    constexpr int NW = NT / 64;
    constexpr int JP = 1024 / NT;                 // columns per thread (L <= 1024)
    constexpr int DSP = 4;                        // row passes held in registers (NT / 32 tiles per pass)
    __shared__ float red[NW][8];
    __shared__ float scale_lds[1024];
    __shared__ __attribute__((aligned(16))) float part_lds[4 * 1024];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t0 = bag_tile_off[b], t1 = bag_tile_off[b + 1], nt = t1 - t0;
    const float* ml = partials + (size_t)T * L;
    if (!AW && blockIdx.y == 1) {
        // ------------------------------------------------------------------ merge of the partials -> M, Mdrop
        float mt = -INFINITY, lt = 0.f;
        if (tid < nt) { mt = ml[2 * (t0 + tid)]; lt = ml[2 * (t0 + tid) + 1]; }
        float keepv[JP];
#pragma unroll
        for (int q = 0; q < JP; ++q) {
            const int j = tid + q * NT;
            keepv[q] = 1.0f;
            if (j < L && mbits != nullptr) keepv[q] = ((mbits[(size_t)b * (L >> 5) + (j >> 5)] >> (j & 31)) & 1u) ? mscale : 0.f;
        }
        const int L4 = L >> 2, NG = NT / L4;      // NT = 256: L in {256, 512, 768, 1024} -> NG in {4, 2, 1, 1}; NT = 1024: 4x
        const int c4 = tid % L4, g = tid / L4;
        const bool worker = g < NG;                // L = 768 leaves 64 threads without a column group
        f32x4 pre[8];                              // the first eight partial rows of this thread: requested before the statistics
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            pre[e] = f32x4{0, 0, 0, 0};
            if (worker && g + e * NG < min(nt, 1024)) pre[e] = *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + g + e * NG) * L + 4 * c4);
        }
        float m = mt;
        for (int t = t0 + tid + NT; t < t1; t += NT) m = fmaxf(m, ml[2 * t]);
        m = wave_allmax(m);
        if (lane == 0) red[wv][0] = m;
        __syncthreads();
        m = red[0][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w][0]);
        const float sc0 = tid < nt ? expf(mt - m) : 0.f;
        float l = lt * sc0;
        for (int t = t0 + tid + NT; t < t1; t += NT) l += ml[2 * t + 1] * expf(ml[2 * t] - m);
        l = wave_allsum(l);
        if (lane == 0) red[wv][1] = l;
        scale_lds[tid] = sc0;
        for (int k = tid + NT; k < 1024; k += NT) scale_lds[k] = (k < nt) ? expf(ml[2 * (t0 + k)] - m) : 0.f;
        __syncthreads();
        l = red[0][1];
#pragma unroll
        for (int w = 1; w < NW; ++w) l += red[w][1];
        const float inv = nt > 0 ? 1.0f / l : 0.f;
        f32x4 acc = {0, 0, 0, 0};
        for (int tb = 0; tb < nt; tb += 1024) {
            if (tb > 0) {
                __syncthreads();
                for (int k = tid; k < 1024; k += NT) scale_lds[k] = (tb + k < nt) ? expf(ml[2 * (t0 + tb + k)] - m) : 0.f;
                __syncthreads();
            }
            const int cnt = worker ? min(1024, nt - tb) : 0;
            int k = g;
            if (tb == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k + e * NG < cnt) acc += scale_lds[k + e * NG] * pre[e];
                k += 8 * NG;
            }
            for (; k + 7 * NG < cnt; k += 8 * NG) {
                f32x4 v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    v[e] = *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + tb + k + e * NG) * L + 4 * c4);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += scale_lds[k + e * NG] * v[e];
            }
            for (; k < cnt; k += NG)
                acc += scale_lds[k] * *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + tb + k) * L + 4 * c4);
        }
        if (worker) *reinterpret_cast<f32x4*>(part_lds + g * L + 4 * c4) = acc;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < JP; ++q) {
            const int j = tid + q * NT;
            if (j < L) {
                float v = 0.f;
                for (int gg = 0; gg < NG; ++gg) v += part_lds[gg * L + j];
                v *= inv;
                M[(size_t)b * L + j] = v;
                if (Mdrop != nullptr) Mdrop[(size_t)b * L + j] = v * keepv[q];
            }
        }
        return;
    }
    // ---------------------------------------------------------------------- logits, loss, dz, ds from the rows
    int ds_row[DSP];
    float ds_sc[DSP], ds_h[DSP][4];
#pragma unroll
    for (int k = 0; k < DSP; ++k) {
        ds_row[k] = -1;
        ds_sc[k] = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) ds_h[k][c] = 0.f;
        const int g8 = t0 + (tid >> 5) + k * (NT / 32);
        if (g8 < t1) {
            const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
            if (lr < nrows) ds_row[k] = row0 + lr;
        }
    }
#pragma unroll
    for (int k = 0; k < DSP; ++k)
        if (ds_row[k] >= 0) {
            ds_sc[k] = scores[ds_row[k]];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) ds_h[k][c] = hrow[(size_t)ds_row[k] * C + c];
        }
    float keepv[JP], wf[JP][4];
#pragma unroll
    for (int q = 0; q < JP; ++q) {
        const int j = tid + q * NT;
        keepv[q] = 1.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) wf[q][c] = 0.f;
        if (j < L) {
            if (mbits != nullptr) keepv[q] = ((mbits[(size_t)b * (L >> 5) + (j >> 5)] >> (j & 31)) & 1u) ? mscale : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) wf[q][c] = Wf[(size_t)c * L + j];
        }
    }
    float bfr[4], yr[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bfr[c] = c < C ? bf[c] : 0.f;
        yr[c] = c < C ? y[b * C + c] : 0.f;
    }
    // ---- step 1: the bag's maximum over the row scores
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < DSP; ++k) m = fmaxf(m, ds_sc[k]);
    for (int g8 = t0 + (tid >> 5) + DSP * (NT / 32); g8 < t1; g8 += NT / 32) {        // bags of more than DSP * NT / 32 tiles
        const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
        if (lr < nrows) m = fmaxf(m, scores[row0 + lr]);
    }
    m = wave_allmax(m);
    if (lane == 0) red[wv][0] = m;
    __syncthreads();
    m = red[0][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w][0]);
    // ---- step 2: normaliser and the head's pre-activations from the rows
    float ek[DSP], sums[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < DSP; ++k) {
        ek[k] = ds_row[k] >= 0 ? expf(ds_sc[k] - m) : 0.f;
        sums[0] += ek[k];
#pragma unroll
        for (int c = 0; c < 4; ++c) sums[1 + c] += ek[k] * ds_h[k][c];
    }
    for (int g8 = t0 + (tid >> 5) + DSP * (NT / 32); g8 < t1; g8 += NT / 32) {
        const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
        if (lr < nrows) {
            const size_t row = (size_t)(row0 + lr);
            const float e = expf(scores[row] - m);
            sums[0] += e;
            for (int c = 0; c < C; ++c) sums[1 + c] += e * hrow[row * C + c];
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) sums[i] = wave_allsum(sums[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) red[wv][1 + i] = sums[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        float v = red[0][1 + i];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[w][1 + i];
        sums[i] = v;
    }
    const float l = sums[0];
    const float inv = nt > 0 ? 1.0f / l : 0.f;
    // ---- step 3 (every thread, no exchange): z, p, loss, dz, M . dM
    float zz[4], pp[4], dzr[4];
    float lossacc = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        zz[c] = sums[1 + c] * inv + bfr[c];
        pp[c] = 1.0f / (1.0f + expf(-zz[c]));
        dzr[c] = 0.f;
    }
    if (loss_kind == 0) {
        // BCELoss on the sigmoid outputs vs one-hot float labels (train_ddp.py:98,323-324); log clamped at -100
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) {
                lossacc += -(yr[c] * fmaxf(logf(pp[c]), -100.0f) + (1.0f - yr[c]) * fmaxf(logf(1.0f - pp[c]), -100.0f));
                dzr[c] = (pp[c] - yr[c]) * scale;
            }
    } else {
        // CrossEntropyLoss applied to the SIGMOID outputs with the one-hot labels as class probabilities (see k_pool_merge_head)
        float mx = -INFINITY, se = 0.f, sy = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < C) mx = fmaxf(mx, pp[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < C) se += expf(pp[c] - mx);
        const float lse_p = mx + logf(se);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) {
                sy += yr[c];
                lossacc += -yr[c] * (pp[c] - lse_p);
            }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) dzr[c] = (expf(pp[c] - lse_p) * sy - yr[c]) * scale * pp[c] * (1.0f - pp[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) dot += dzr[c] * (zz[c] - bfr[c]);
    // ---- step 4: the score gradient of the bag's rows
#pragma unroll
    for (int k = 0; k < DSP; ++k)
        if (ds_row[k] >= 0) {
            float gd = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) gd += dzr[c] * ds_h[k][c];
            ds[ds_row[k]] = ek[k] * inv * (gd - dot);
            if (AW) arow[ds_row[k]] = ek[k] * inv;
        }
    for (int g8 = t0 + (tid >> 5) + DSP * (NT / 32); g8 < t1; g8 += NT / 32) {
        const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
        if (lr < nrows) {
            const size_t row = (size_t)(row0 + lr);
            float gd = 0.f;
            for (int c = 0; c < C; ++c) gd += dzr[c] * hrow[row * C + c];
            const float an = expf(scores[row] - m) * inv;
            ds[row] = an * (gd - dot);
            if (AW) arow[row] = an;
        }
    }
    if (tid == 0) {
        lse[b] = nt > 0 ? m + logf(l) : -INFINITY;
        cdot[b] = dot;
        loss_sum[b] = lossacc * scale;              // per-bag loss; summed (fixed order) by k_head_bwd_params
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (tid == c && c < C) {
            z[b * C + c] = zz[c];
            p[b * C + c] = pp[c];
            dz[b * C + c] = dzr[c];
        }
#pragma unroll
    for (int q = 0; q < JP; ++q) {
        const int j = tid + q * NT;
        if (j < L) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) d += dzr[c] * wf[q][c];
            dM[(size_t)b * L + j] = d * keepv[q];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The per-bag tail for LONG bags (the authors' regime: ONE bag of 2 000 - 15 592 patches per GPU and step, run_train.sh:81;
// config 5's 4096-patch bags): one or two workgroups per bag walk hundreds of tiles one pass after the other (22 us for a
// 10 000-patch bag).  Two short launches spread the bag over many workgroups instead:
//   k_tail_stats  grid (B, S): workgroup (b, s) takes every S-th group of eight tiles of bag b: its rows' maximum m_w and,
//                 relative to it, l_w = sum e_n and z_w[c] = sum e_n h_n[c]  ->  ws[b][s][0..5]
//   k_tail_apply  grid (B, S + L / 64): every workgroup folds the S partial statistics of its bag (same order, same bits
//                 everywhere) into m, l, z -> p, loss, dz, M . dM (k_pool_tail_h's arithmetic); workgroups y < S write
//                 ds for the rows they took in the first launch, workgroup y = 0 also the bag's scalars and dM; workgroups
//                 y >= S merge the tile partials of one 64-column chunk -> M, Mdrop (tile weight exp(m_t - lse)).
// No atomics, no counters: the second launch is the barrier.
#define TAIL_S_MAX 16
template <int DSP>
__device__ __forceinline__ void tail_rows_load(const int32_t* __restrict__ tile_map, const float* __restrict__ scores,
                                               const float* __restrict__ hrow, int C, int t0, int t1, int s, int S, int tid,
                                               int (&row)[DSP], float (&sc)[DSP], float (&hh)[DSP][4]) {
#pragma unroll
    for (int k = 0; k < DSP; ++k) {
        row[k] = -1;
        sc[k] = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) hh[k][c] = 0.f;
        const int g8 = t0 + (k * S + s) * 8 + (tid >> 5);
        if (g8 < t1) {
            const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
            if (lr < nrows) row[k] = row0 + lr;
        }
    }
#pragma unroll
    for (int k = 0; k < DSP; ++k)
        if (row[k] >= 0) {
            sc[k] = scores[row[k]];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) hh[k][c] = hrow[(size_t)row[k] * C + c];
        }
}

__global__ __launch_bounds__(256) void k_tail_stats(const int32_t* __restrict__ bag_tile_off, const int32_t* __restrict__ tile_map,
                                                    const float* __restrict__ scores, const float* __restrict__ hrow, int C,
                                                    int S, float* __restrict__ ws) {
    constexpr int DSP = 4;
    __shared__ float red[4][8];
    const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t0 = bag_tile_off[b], t1 = bag_tile_off[b + 1];
    int row[DSP];
    float sc[DSP], hh[DSP][4];
    tail_rows_load<DSP>(tile_map, scores, hrow, C, t0, t1, s, S, tid, row, sc, hh);
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < DSP; ++k) m = fmaxf(m, sc[k]);
    for (int g8 = t0 + (DSP * S + s) * 8 + (tid >> 5); g8 < t1; g8 += 8 * S) {        // more than DSP passes: from memory
        const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
        if (lr < nrows) m = fmaxf(m, scores[row0 + lr]);
    }
    m = wave_allmax(m);
    if (lane == 0) red[wv][0] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    float sums[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (m > -INFINITY) {
#pragma unroll
        for (int k = 0; k < DSP; ++k) {
            const float e = row[k] >= 0 ? expf(sc[k] - m) : 0.f;
            sums[0] += e;
#pragma unroll
            for (int c = 0; c < 4; ++c) sums[1 + c] += e * hh[k][c];
        }
        for (int g8 = t0 + (DSP * S + s) * 8 + (tid >> 5); g8 < t1; g8 += 8 * S) {
            const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
            if (lr < nrows) {
                const size_t r_ = (size_t)(row0 + lr);
                const float e = expf(scores[r_] - m);
                sums[0] += e;
                for (int c = 0; c < C; ++c) sums[1 + c] += e * hrow[r_ * C + c];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) sums[i] = wave_allsum(sums[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 5; ++i) red[wv][1 + i] = sums[i];
    __syncthreads();
    if (tid < 6) {
        float* o = ws + ((size_t)b * TAIL_S_MAX + s) * 8;
        o[tid] = tid == 0 ? m : (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

__global__ __launch_bounds__(256) void k_tail_apply(const float* __restrict__ partials, const int32_t* __restrict__ bag_tile_off,
                                                    int T, int L, const float* __restrict__ Wf, const float* __restrict__ bf,
                                                    int C, const float* __restrict__ y, float scale, float* __restrict__ M,
                                                    float* __restrict__ lse, float* __restrict__ z, float* __restrict__ p,
                                                    float* __restrict__ loss_sum, float* __restrict__ dz,
                                                    float* __restrict__ dM, float* __restrict__ cdot,
                                                    const int32_t* __restrict__ tile_map, const float* __restrict__ scores,
                                                    const float* __restrict__ hrow, float* __restrict__ ds,
                                                    const uint32_t* __restrict__ mbits, float mscale,
                                                    float* __restrict__ Mdrop, int loss_kind, int S,
                                                    const float* __restrict__ ws) {
    constexpr int DSP = 4;
    __shared__ __attribute__((aligned(16))) float part_lds[16 * 64];
    const int b = blockIdx.x, yb = blockIdx.y, tid = threadIdx.x;
    const int t0 = bag_tile_off[b], t1 = bag_tile_off[b + 1], nt = t1 - t0;
    // the rows of a ds workgroup: requested before the statistics are folded
    int row[DSP];
    float sc[DSP], hh[DSP][4];
    if (yb < S) tail_rows_load<DSP>(tile_map, scores, hrow, C, t0, t1, yb, S, tid, row, sc, hh);
    // ---- fold the S partial statistics (every thread of every workgroup: the same operations in the same order)
    const float* wb = ws + (size_t)b * TAIL_S_MAX * 8;
    float m = -INFINITY;
    for (int i = 0; i < S; ++i) m = fmaxf(m, wb[8 * i]);
    float sums[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < S; ++i) {
        const float mw = wb[8 * i];
        const float f = mw > -INFINITY ? expf(mw - m) : 0.f;
#pragma unroll
        for (int q = 0; q < 5; ++q) sums[q] += f * wb[8 * i + 1 + q];
    }
    const float l = sums[0];
    const float inv = nt > 0 && l > 0.f ? 1.0f / l : 0.f;
    const float lse_b = nt > 0 ? m + logf(l) : -INFINITY;
    float bfr[4], yr[4], zz[4], pp[4], dzr[4];
    float lossacc = 0.f, dot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bfr[c] = c < C ? bf[c] : 0.f;
        yr[c] = c < C ? y[b * C + c] : 0.f;
        zz[c] = sums[1 + c] * inv + bfr[c];
        pp[c] = 1.0f / (1.0f + expf(-zz[c]));
        dzr[c] = 0.f;
    }
    if (loss_kind == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) {
                lossacc += -(yr[c] * fmaxf(logf(pp[c]), -100.0f) + (1.0f - yr[c]) * fmaxf(logf(1.0f - pp[c]), -100.0f));
                dzr[c] = (pp[c] - yr[c]) * scale;
            }
    } else {
        float mx = -INFINITY, se = 0.f, sy = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < C) mx = fmaxf(mx, pp[c]);
#pragma unroll
        for (int c = 0; c < 4; ++c) if (c < C) se += expf(pp[c] - mx);
        const float lse_p = mx + logf(se);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) {
                sy += yr[c];
                lossacc += -yr[c] * (pp[c] - lse_p);
            }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) dzr[c] = (expf(pp[c] - lse_p) * sy - yr[c]) * scale * pp[c] * (1.0f - pp[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) dot += dzr[c] * (zz[c] - bfr[c]);
    if (yb < S) {
        // ---- ds of this workgroup's rows
#pragma unroll
        for (int k = 0; k < DSP; ++k)
            if (row[k] >= 0) {
                float gd = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) gd += dzr[c] * hh[k][c];
                ds[row[k]] = expf(sc[k] - m) * inv * (gd - dot);
            }
        for (int g8 = t0 + (DSP * S + yb) * 8 + (tid >> 5); g8 < t1; g8 += 8 * S) {
            const int row0 = tile_map[4 * g8 + 1], nrows = tile_map[4 * g8 + 2], lr = tid & 31;
            if (lr < nrows) {
                const size_t r_ = (size_t)(row0 + lr);
                float gd = 0.f;
                for (int c = 0; c < C; ++c) gd += dzr[c] * hrow[r_ * C + c];
                ds[r_] = expf(scores[r_] - m) * inv * (gd - dot);
            }
        }
        if (yb == 0) {
            if (tid == 0) {
                lse[b] = lse_b;
                cdot[b] = dot;
                loss_sum[b] = lossacc * scale;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (tid == c && c < C) {
                    z[b * C + c] = zz[c];
                    p[b * C + c] = pp[c];
                    dz[b * C + c] = dzr[c];
                }
            for (int j = tid; j < L; j += 256) {
                float keep = 1.0f;
                if (mbits != nullptr) keep = ((mbits[(size_t)b * (L >> 5) + (j >> 5)] >> (j & 31)) & 1u) ? mscale : 0.f;
                float d = 0.f;
                for (int c = 0; c < C; ++c) d += dzr[c] * Wf[(size_t)c * L + j];
                dM[(size_t)b * L + j] = d * keep;
            }
        }
        return;
    }
    // ---- merge of the tile partials, columns [64 j, 64 j + 64): thread (tile group tg < 16, float4 column c4 < 16)
    const int j0 = 64 * (yb - S), c4 = tid & 15, tg = tid >> 4;
    const float* ml = partials + (size_t)T * L;
    f32x4 acc = {0, 0, 0, 0};
    int k = tg;
    for (; k + 48 < nt; k += 64) {                 // four tiles in flight per thread
        f32x4 v[4];
        float w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + k + 16 * e) * L + j0 + 4 * c4);
            w[e] = ml[2 * (t0 + k + 16 * e)];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += expf(w[e] - lse_b) * v[e];
    }
    for (; k < nt; k += 16)
        acc += expf(ml[2 * (t0 + k)] - lse_b) * *reinterpret_cast<const f32x4*>(partials + (size_t)(t0 + k) * L + j0 + 4 * c4);
    *reinterpret_cast<f32x4*>(part_lds + tg * 64 + 4 * c4) = acc;
    __syncthreads();
    if (tid < 64) {
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) v += part_lds[q * 64 + tid];
        const int j = j0 + tid;
        M[(size_t)b * L + j] = v;
        if (Mdrop != nullptr) {
            float keep = 1.0f;
            if (mbits != nullptr) keep = ((mbits[(size_t)b * (L >> 5) + (j >> 5)] >> (j & 31)) & 1u) ? mscale : 0.f;
            Mdrop[(size_t)b * L + j] = v * keep;
        }
    }
}

extern "C" size_t mil_pool_tail_workspace_floats(int B) { return (size_t)(B > 0 ? B : 0) * TAIL_S_MAX * 8; }

extern "C" int mil_pool_merge_head_ws(const float* partials, const int32_t* bag_tile_off, int T, int B, int L,
                                      const float* Wf, const float* bf, int C, const float* y, float scale, float* M,
                                      float* lse, float* z, float* p, float* loss_sum, float* dz, float* dM, float* cdot,
                                      const int32_t* tile_map, const float* scores, const float* hrow, float* ds,
                                      const uint32_t* mbits, float mscale, float* Mdrop, int loss_kind, float* tail_ws,
                                      void* stream) {
    if (!partials || !bag_tile_off || !Wf || !bf || !M || !lse || !z || !p) return MIL_EINVAL;
    if (loss_kind != MIL_LOSS_BCE && loss_kind != MIL_LOSS_CE_ON_SIGMOID) return MIL_EINVAL;
    if (y && (!loss_sum || !dz || !dM || !cdot)) return MIL_EINVAL;
    if (ds && (!y || !tile_map || !scores || !hrow)) return MIL_EINVAL;
    if (!(L == 256 || L == 512 || L == 768 || L == 1024) || C <= 0 || C > 32 || B < 0) return MIL_EINVAL;
    if (B == 0) return MIL_OK;
    // one workgroup per bag; bags of many tiles (>= 48 on average: 1536 rows) get 1024 threads - four times the tile
    // groups walking the partials and the rows of the ds pass (config 5, 128 tiles per bag: 21 -> see DESIGN.md)
    const char* tail_env = getenv("MIL_TAIL_H");                     // "0": the long-chain form (A/B runs, equivalence test)
    const bool short_chain = C <= 4 && y && ds && hrow && !(tail_env != nullptr && tail_env[0] == '0');
    if (short_chain && tail_ws != nullptr && T >= 64 * B && B <= 8 && (tail_env == nullptr || tail_env[0] != '1')) {
        // a FEW long bags (>= 64 tiles = 2048 rows on average): two short launches over many workgroups per bag ("1": never).
        // With many bags the bags themselves are the parallelism: config 5 (32 x 128 tiles) 13.9 us in one launch, 15.4 - 16.5 so.
        int S = (T / B + 31) / 32;
        if (S > TAIL_S_MAX) S = TAIL_S_MAX;
        hipLaunchKernelGGL(k_tail_stats, dim3(B, S), dim3(256), 0, (hipStream_t)stream, bag_tile_off, tile_map, scores, hrow, C, S,
                           tail_ws);
        MIL_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_tail_apply, dim3(B, S + L / 64), dim3(256), 0, (hipStream_t)stream, partials, bag_tile_off, T, L, Wf, bf,
                           C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map, scores, hrow, ds, mbits, mscale, Mdrop,
                           loss_kind, S, (const float*)tail_ws);
        MIL_CHECK_LAUNCH();
        return MIL_OK;
    }
    if (short_chain) {
        if (T >= 48 * B)
            hipLaunchKernelGGL(k_pool_tail_h<1024>, dim3(B, 2), dim3(1024), 0, (hipStream_t)stream, partials, bag_tile_off, T, L, Wf, bf,
                               C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map, scores, hrow, ds, mbits, mscale, Mdrop,
                               loss_kind);
        else
            hipLaunchKernelGGL(k_pool_tail_h<256>, dim3(B, 2), dim3(256), 0, (hipStream_t)stream, partials, bag_tile_off, T, L, Wf, bf,
                               C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map, scores, hrow, ds, mbits, mscale, Mdrop,
                               loss_kind);
        MIL_CHECK_LAUNCH();
        return MIL_OK;
    }
    if (T >= 48 * B)
        hipLaunchKernelGGL(k_pool_merge_head<1024>, dim3(B), dim3(1024), 0, (hipStream_t)stream, partials, bag_tile_off, T, L, Wf,
                           bf, C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map, scores, hrow, ds, mbits, mscale,
                           Mdrop, loss_kind);
    else
        hipLaunchKernelGGL(k_pool_merge_head<256>, dim3(B), dim3(256), 0, (hipStream_t)stream, partials, bag_tile_off, T, L, Wf,
                           bf, C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map, scores, hrow, ds, mbits, mscale,
                           Mdrop, loss_kind);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

int pool_tail_rows(const int32_t* bag_tile_off, int T, int B, int L, const float* Wf, const float* bf, int C, const float* y,
                   float scale, float* lse, float* z, float* p, float* loss_sum, float* dz, float* dM, float* cdot,
                   const int32_t* tile_map, const float* scores, const float* hrow, float* ds, const uint32_t* mbits, float mscale,
                   int loss_kind, float* arow, void* stream) {
    if (!bag_tile_off || !Wf || !bf || !y || !lse || !z || !p || !loss_sum || !dz || !dM || !cdot) return MIL_EINVAL;
    if (!tile_map || !scores || !hrow || !ds || !arow) return MIL_EINVAL;
    if (loss_kind != MIL_LOSS_BCE && loss_kind != MIL_LOSS_CE_ON_SIGMOID) return MIL_EINVAL;
    if (!(L == 256 || L == 512 || L == 768 || L == 1024) || C <= 0 || C > 4 || B < 0) return MIL_EINVAL;
    if (B == 0) return MIL_OK;
    // the thread counts of mil_pool_merge_head_ws's short chain
    if (T >= 48 * B)
        hipLaunchKernelGGL((k_pool_tail_h<1024, true>), dim3(B, 1), dim3(1024), 0, (hipStream_t)stream, (const float*)nullptr,
                           bag_tile_off, T, L, Wf, bf, C, y, scale, (float*)nullptr, lse, z, p, loss_sum, dz, dM, cdot, tile_map,
                           scores, hrow, ds, mbits, mscale, (float*)nullptr, loss_kind, arow);
    else
        hipLaunchKernelGGL((k_pool_tail_h<256, true>), dim3(B, 1), dim3(256), 0, (hipStream_t)stream, (const float*)nullptr,
                           bag_tile_off, T, L, Wf, bf, C, y, scale, (float*)nullptr, lse, z, p, loss_sum, dz, dM, cdot, tile_map,
                           scores, hrow, ds, mbits, mscale, (float*)nullptr, loss_kind, arow);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_pool_merge_head(const float* partials, const int32_t* bag_tile_off, int T, int B, int L,
                                   const float* Wf, const float* bf, int C, const float* y, float scale, float* M,
                                   float* lse, float* z, float* p, float* loss_sum, float* dz, float* dM, float* cdot,
                                   const int32_t* tile_map, const float* scores, const float* hrow, float* ds,
                                   const uint32_t* mbits, float mscale, float* Mdrop, int loss_kind, void* stream) {
    return mil_pool_merge_head_ws(partials, bag_tile_off, T, B, L, Wf, bf, C, y, scale, M, lse, z, p, loss_sum, dz, dM, cdot, tile_map,
                                  scores, hrow, ds, mbits, mscale, Mdrop, loss_kind, nullptr, stream);
}

extern "C" int mil_head_fwd(const float* M, const float* Wf, const float* bf, float* z, float* p, int B, int L, int C,
                            void* stream) {
    if (!M || !Wf || !bf || !z || !p) return MIL_EINVAL;
    if (B < 0 || L <= 0 || C <= 0 || C > 32) return MIL_EINVAL;
    if (B == 0) return MIL_OK;
    hipLaunchKernelGGL(k_head_fwd, dim3(B), dim3(256), 0, (hipStream_t)stream, M, Wf, bf, z, p, L, C);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_bce_fwd_bwd(const float* p, const float* y, float* loss_sum, float* dz, int B, int C, float scale,
                               void* stream) {
    if (!p || !y || !loss_sum || !dz) return MIL_EINVAL;
    if (B <= 0 || C <= 0) return MIL_EINVAL;
    hipLaunchKernelGGL(k_bce_fwd_bwd, dim3(1), dim3(256), 0, (hipStream_t)stream, p, y, loss_sum, dz, B * C, scale);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_head_bwd(const float* dz_or_dp, const float* p, const float* M, const float* Wf, float* dM,
                            float* dWf, float* dbf, float* cdot, int B, int L, int C, void* stream) {
    if (!dz_or_dp || !M || !Wf || !dM || !dWf || !dbf || !cdot) return MIL_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || C > 32) return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_head_bwd_dm, dim3(B), dim3(256), 0, st, dz_or_dp, p, M, Wf, dM, cdot, L, C);
    MIL_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_bwd_params, dim3(C * ((L + 63) / 64) + 1), dim3(256), 0, st, dz_or_dp, p, M, dWf, dbf, B, L,
                       C, (const float*)nullptr, (float*)nullptr, 0);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_head_bwd_params_acc(const float* dz, const float* M, float* dWf, float* dbf, int B, int L, int C,
                                       const float* loss_bag, float* loss_out, int accumulate, void* stream) {
    if (!dz || !M || !dWf || !dbf) return MIL_EINVAL;
    if (B <= 0 || L <= 0 || C <= 0 || C > 32 || (loss_bag && !loss_out)) return MIL_EINVAL;
    hipLaunchKernelGGL(k_head_bwd_params, dim3(C * ((L + 63) / 64) + 1), dim3(256), 0, (hipStream_t)stream, dz,
                       (const float*)nullptr, M, dWf, dbf, B, L, C, loss_bag, loss_out, accumulate);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
extern "C" int mil_head_bwd_params(const float* dz, const float* M, float* dWf, float* dbf, int B, int L, int C,
                                   const float* loss_bag, float* loss_out, void* stream) {
    return mil_head_bwd_params_acc(dz, M, dWf, dbf, B, L, C, loss_bag, loss_out, 0, stream);
}

// small buffers (the image-only step: 0.2 M parameters) want many workgroups, large ones (fusion: 9.8 M) loads in flight
static void launch_adam(float* param, const float* grad, float* m, float* v, size_t n, float lr, float b1, float b2,
                        float eps, float wd, float gscale, float bc1, float bc2_sqrt, const int* step_dev, hipStream_t st,
                        const float* lr_dev = nullptr) {
    if (n >= ((size_t)1 << 21))
        hipLaunchKernelGGL(k_adam<4>, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, st, param, grad, m, v, n, lr, b1, b2, eps,
                           wd, gscale, bc1, bc2_sqrt, step_dev, lr_dev);
    else
        hipLaunchKernelGGL(k_adam<1>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, param, grad, m, v, n, lr, b1, b2, eps,
                           wd, gscale, bc1, bc2_sqrt, step_dev, lr_dev);
}

extern "C" int mil_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, int step,
                             float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                             void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1) return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_scale, (float)bc1,
                (float)sqrt(bc2), (const int*)nullptr, (hipStream_t)stream);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// The Adam launch of mil_adam_step_counted WITHOUT the counter increment: a flat buffer updated in several contiguous
// segments (optim.FlatAdam skips parameters that received no gradient, as torch.optim.Adam does) reads the same step
// number in every segment; the caller advances the counter once (mil_counter_add).
extern "C" int mil_adam_step_counted_noinc(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                           const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                           float weight_decay, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_counter) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_scale, 1.f, 1.f,
                (const int*)step_counter, (hipStream_t)stream);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
extern "C" int mil_adam_step_counted(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                     int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, float grad_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_counter) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n > 0) {
        launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, grad_scale, 1.f, 1.f,
                    (const int*)step_counter, st);
        MIL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st, step_counter);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// mil_adam_step_counted with the learning rate in device memory as well (lr_dev [1]): a captured step follows a learning-rate
// schedule (utils.py:232-241 adjust_learning_rate) without re-capture.  inc != 0: advance the counter after the update.
extern "C" int mil_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                 int32_t* step_counter, const float* lr_dev, float beta1, float beta2, float eps,
                                 float weight_decay, float grad_scale, int inc, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_counter || !lr_dev) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n > 0) {
        launch_adam(param, grad, exp_avg, exp_avg_sq, n, 0.f, beta1, beta2, eps, weight_decay, grad_scale, 1.f, 1.f,
                    (const int*)step_counter, st, lr_dev);
        MIL_CHECK_LAUNCH();
    }
    if (inc) {
        hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, st, step_counter);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_adam_step_dev_segs(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const size_t* seg_begin,
                                      const size_t* seg_end, int nseg, int32_t* step_counter, const float* lr_dev,
                                      int32_t* done_counter, float beta1, float beta2, float eps, float weight_decay,
                                      float grad_scale, int inc, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_counter || !lr_dev || !done_counter || !seg_begin || !seg_end)
        return MIL_EINVAL;
    if (nseg < 1 || nseg > MIL_ADAM_MAX_SEGS) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
        return MIL_EINVAL;
    AdamSegs sg;
    sg.nseg = nseg;
    unsigned blocks = 0;
    for (int i = 0; i < MIL_ADAM_MAX_SEGS; ++i) { sg.blk_end[i] = 0; sg.begin[i] = sg.end[i] = 0; }
    for (int i = 0; i < nseg; ++i) {
        if (seg_end[i] < seg_begin[i] || (seg_begin[i] & 3)) return MIL_EINVAL;
        blocks += (unsigned)((seg_end[i] - seg_begin[i] + 4095) / 4096);
        sg.blk_end[i] = blocks;
        sg.begin[i] = seg_begin[i];
        sg.end[i] = seg_end[i];
    }
    if (blocks == 0) {
        if (inc) { hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, (hipStream_t)stream, step_counter); MIL_CHECK_LAUNCH(); }
        return MIL_OK;
    }
    hipLaunchKernelGGL(k_adam_segs, dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, sg, beta1,
                       beta2, eps, weight_decay, grad_scale, step_counter, lr_dev, done_counter, inc);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// torch.optim.SGD without momentum (train_ddp.py:103-108, the learnable-prompt runs): g = grad_scale * grad + wd * p;
// p -= lr * g.  One float4 per thread.
__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ param, const float* __restrict__ grad, size_t n, float lr,
                                             float wd, float gscale) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        f32x4 p4 = *reinterpret_cast<const f32x4*>(param + i);
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(grad + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) p4[e] = p4[e] - lr * (g4[e] * gscale + wd * p4[e]);
        *reinterpret_cast<f32x4*>(param + i) = p4;
    } else {
        for (size_t j = i; j < n; ++j) param[j] = param[j] - lr * (grad[j] * gscale + wd * param[j]);
    }
}

extern "C" int mil_sgd_step(float* param, const float* grad, size_t n, float lr, float weight_decay, float grad_scale,
                            void* stream) {
    if (!param || !grad) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad)) & 15) return MIL_EINVAL;
    if (n == 0) return MIL_OK;
    hipLaunchKernelGGL(k_sgd, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, param, grad, n, lr,
                       weight_decay, grad_scale);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// torch.nn.CosineEmbeddingLoss()(x1, x2, target) with target = +1 for every row and the default mean reduction - the
// 'textCosSim' term between the two text-aligned tokens x_CT2CI and x_Pth2CI (reference train_ddp.py:102,266,325-329).
// ATen's arithmetic (cosine_embedding_loss): cos = (x1 . x2) / sqrt((|x1|^2 + 1e-12) (|x2|^2 + 1e-12)), row loss 1 - cos.
// Forward and backward in one launch of ONE workgroup (B is the per-GPU batch: a handful of rows): wave w takes rows w,
// w + 16, ...;  d(1 - cos)/dx1 = -(x2 / den - cos x1 / m1), same for x2; `scale` (1 / B for the mean, times whatever weight
// the caller gives the term) is folded into the gradients and the loss.  The row losses are summed in row order.
__global__ __launch_bounds__(1024) void k_cosine_embedding_loss(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                int B, int E, float scale, float* __restrict__ loss,
                                                                float* __restrict__ dx1, float* __restrict__ dx2) {
    __shared__ float rowloss[1024];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int b0 = 0; b0 < B; b0 += 16) {
        const int b = b0 + w;
        if (b < B) {
            const float* a = x1 + (size_t)b * E;
            const float* c = x2 + (size_t)b * E;
            float dot = 0.f, m1 = 0.f, m2 = 0.f;
            for (int j = lane; j < E; j += 64) { const float u = a[j], v = c[j]; dot += u * v; m1 += u * u; m2 += v * v; }
            dot = wave_allsum(dot);
            m1 = wave_allsum(m1) + 1e-12f;
            m2 = wave_allsum(m2) + 1e-12f;
            const float den = sqrtf(m1 * m2), cs = dot / den;
            if (dx1 != nullptr)
                for (int j = lane; j < E; j += 64) {
                    const float u = a[j], v = c[j];
                    dx1[(size_t)b * E + j] = -scale * (v / den - cs * u / m1);
                    dx2[(size_t)b * E + j] = -scale * (u / den - cs * v / m2);
                }
            if (lane == 0) rowloss[b] = 1.0f - cs;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = 0.f;
        for (int b = 0; b < B; ++b) v += rowloss[b];
        loss[0] = v * scale;
    }
}

extern "C" int mil_cosine_embedding_loss(const float* x1, const float* x2, int B, int E, float scale, float* loss,
                                         float* dx1, float* dx2, void* stream) {
    if (!x1 || !x2 || !loss || B <= 0 || B > 1024 || E <= 0 || ((dx1 == nullptr) != (dx2 == nullptr))) return MIL_EINVAL;
    hipLaunchKernelGGL(k_cosine_embedding_loss, dim3(1), dim3(1024), 0, (hipStream_t)stream, x1, x2, B, E, scale, loss, dx1, dx2);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// out[b] = a[b] . c[b]   (row-wise dot of two [B, L] matrices; cdot for the pool backward).
__global__ __launch_bounds__(256) void k_rowdot(const float* __restrict__ a, const float* __restrict__ c,
                                                float* __restrict__ out, int L) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    float v = 0.f;
    for (int j = threadIdx.x; j < L; j += 256) v += a[(size_t)b * L + j] * c[(size_t)b * L + j];
    v = block_allsum_256(v, red);
    if (threadIdx.x == 0) out[b] = v;
}

extern "C" int mil_rowdot(const float* a, const float* c, float* out, int B, int L, void* stream) {
    if (!a || !c || !out || B < 0 || L <= 0) return MIL_EINVAL;
    if (B == 0) return MIL_OK;
    hipLaunchKernelGGL(k_rowdot, dim3(B), dim3(256), 0, (hipStream_t)stream, a, c, out, L);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// ---------------------------------------------------------------------------------------------
// CLIP-as-loss of the image-only variant (reference utils.py:247-284 CLIPloss_v1): for each clinical feature f,
// logits_f[i][j] = out[i] . feat[j][f]  (bag embedding i vs the CLIP text feature of sample j's prompt f), target =
// identity, CrossEntropyLoss over dim 1 (softmax over the bags i for every text j), mean over F * b.
//   loss = -(1 / (F b)) sum_f sum_j log softmax_i(logits_f[:, j])[j];  d_out[i] = sum_f sum_j (p_f[i][j] - [i==j]) feat[j][f] / (F b)
// One workgroup (256 threads) per feature; b <= 64.  part_dout [F][b][E] is folded over F by mil_colsum.
__global__ __launch_bounds__(256) void k_clip_contrastive(const float* __restrict__ out, const float* __restrict__ feat,
                                                          int b, int F, int E, float* __restrict__ loss_f,
                                                          float* __restrict__ part_dout) {
    __shared__ float lg[64 * 64];       // logits -> d_logits, [i][j]
    __shared__ float red[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int idx = tid; idx < b * b; idx += 256) {
        const int i = idx / b, j = idx % b;
        const float* o = out + (size_t)i * E;
        const float* t = feat + ((size_t)j * F + f) * E;
        float v = 0.f;
        for (int e = 0; e < E; e += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(o + e), c = *reinterpret_cast<const f32x4*>(t + e);
            v += a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3];
        }
        lg[i * 64 + j] = v;
    }
    __syncthreads();
    float lacc = 0.f;
    const float inv = 1.0f / (float)(F * b);
    if (tid < b) {                       // column j = tid: softmax over the bags i
        const int j = tid;
        float m = -INFINITY;
        for (int i = 0; i < b; ++i) m = fmaxf(m, lg[i * 64 + j]);
        float s = 0.f;
        for (int i = 0; i < b; ++i) s += expf(lg[i * 64 + j] - m);
        const float lse = m + logf(s);
        lacc = -(lg[j * 64 + j] - lse);
        for (int i = 0; i < b; ++i) lg[i * 64 + j] = (expf(lg[i * 64 + j] - lse) - (i == j ? 1.f : 0.f)) * inv;
    }
    lacc = block_allsum_256(lacc, red);
    if (tid == 0) loss_f[f] = lacc * inv;
    __syncthreads();
    for (int idx = tid; idx < b * E; idx += 256) {
        const int i = idx / E, e = idx % E;
        float v = 0.f;
        for (int j = 0; j < b; ++j) v += lg[i * 64 + j] * feat[((size_t)j * F + f) * E + e];
        part_dout[((size_t)f * b + i) * E + e] = v;
    }
}

extern "C" int mil_clip_contrastive_loss(const float* out, const float* feat, int b, int F, int E, float* loss,
                                         float* d_out, float* workspace, void* stream) {
    if (!out || !feat || !loss || !d_out || !workspace) return MIL_EINVAL;
    if (b <= 0 || b > 64 || F <= 0 || E <= 0 || (E & 3)) return MIL_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* loss_f = workspace;                      // [F]
    float* part = workspace + ((F + 3) & ~3);       // [F][b][E]
    hipLaunchKernelGGL(k_clip_contrastive, dim3(F), dim3(256), 0, st, out, feat, b, F, E, loss_f, part);
    MIL_CHECK_LAUNCH();
    int rc = mil_colsum(part, b * E, F, b * E, d_out, 0, nullptr, stream);
    if (rc) return rc;
    return mil_colsum(loss_f, 1, F, 1, loss, 0, nullptr, stream);
}
