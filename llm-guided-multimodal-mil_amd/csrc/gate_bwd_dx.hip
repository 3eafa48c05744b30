// K1 backward: the gate input gradient of the gated-attention MIL pooling (ABMIL) for gfx950.
//
// Reference arithmetic: torch autograd of model/dim1/ABMIL.py:47-59.  Forward and route plan: gate_fwd.hip.
#include "mil_internal.h"

// ================================================================================ K1 backward: gate dx (MFMA)
// dx[row][j] += sum_d dPreV[row][d] Wv[d][j] + dPreU[row][d] Wu[d][j]     (M = R, N = L, K = 384).
// K-slices of 32 = 16 d's x {V, U} so one (V, U) load pair yields both dPre terms.
// Workgroup 256 threads, tile 128 rows x 128 cols, wave (wi, wj) owns 64 x 64.
#define GX_KS 36       // k-contiguous A image row stride (words), as in k_gemm
// Same pipeline as k_gemm (csrc/linear.hip): 128 x 128 x 32 tiles, 2 x 2 waves of 64 x 64, the A image k-contiguous
// ([128][36], ds_read_b128 fragments: lane (r, h) takes k = 8t + 4h + jj), the weights k-major ([32][128]); registers
// carry the slice after next and the staging is issued in pieces between MFMA groups.  A slice of 32 k's is 16 gate units:
// local k 0..15 = dPreV_d, 16..31 = dPreU_d (d = 16 kk + k), built from (V, U, ds, w) when the slice is written to LDS.
// Pool term: with (scores, lse, row_bag, dM) given the kernel does not read dx at all - the attention pool's own input
// gradient, a_row dM[bag(row)] with a_row = exp(score_row - lse[bag]) (ABMIL.py:57-59), is formed in the epilogue from the
// [B, L] table dM and dx is written once (no pool-backward pass over [R, L], no read-modify-write here).
__global__ __launch_bounds__(256) void k_gate_bwd_dx(const float* __restrict__ gates, const float* __restrict__ ds,
                                                     const float* __restrict__ wvec, const float* __restrict__ Wv,
                                                     const float* __restrict__ Wu, float* __restrict__ dx, int R, int L,
                                                     const uint32_t* __restrict__ xbits, float xscale,
                                                     const float* __restrict__ scores, const float* __restrict__ lse,
                                                     const int32_t* __restrict__ row_bag, const float* __restrict__ dM) {
    constexpr int ASZ = 128 * GX_KS, BSZ = 32 * 128;
    __shared__ __attribute__((aligned(16))) float smem[2 * (ASZ + BSZ)];
    float* as = smem;
    float* bs = smem + 2 * ASZ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int NJ = L / 128;
    // XCD-aware order (as the weight-gradient kernels): the NJ column tiles of a row tile read the same 128 x 384 gates; with
    // the hardware's round-robin of workgroup ids over the 8 XCDs they sat on NJ different L2s (PMC: 200 MiB fetched for 48 MiB
    // of gates).  logical = (id % 8) * share + id / 8 puts them on consecutive slots of ONE XCD.
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const int jt = bid % NJ, rt = bid / NJ;
    const int row0 = rt * 128, j0 = jt * 128;

    // A producer: thread -> unit quad dq = tid & 3 (d = 16 kk + 4 dq ..+3), rows (tid >> 2) + 64 i (i < 2)
    const int dq = tid & 3, arow = tid >> 2;
    const float* gsrc[2];
    float dsr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int gr = row0 + arow + 64 * i;
        gsrc[i] = gates + (size_t)min(gr, R - 1) * GF_NG + 4 * dq;
        dsr[i] = gr < R ? ds[gr] : 0.f;                       // rows past the end contribute zeros
    }
    // B: k row (tid >> 5) + 8 i (i < 2: Wv rows, i >= 2: Wu rows), 16-byte chunk tid & 31
    const int bk = tid >> 5, bc4 = tid & 31;
    const float* bsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bsrc[i] = ((i < 2) ? Wv : Wu) + (size_t)(bk + 8 * (i & 1)) * L + j0 + 4 * bc4;
    f32x4 rv[2], ru[2], rw[2], rb[4];
    auto a_load = [&](int i, int kk) {
        rv[i] = *reinterpret_cast<const f32x4*>(gsrc[i] + 16 * kk);
        ru[i] = *reinterpret_cast<const f32x4*>(gsrc[i] + 192 + 16 * kk);
        rw[i] = *reinterpret_cast<const f32x4*>(wvec + 16 * kk + 4 * dq);
    };
    auto a_store = [&](int i, float* dst) {
        const f32x4 v = rv[i], u = ru[i];
        const f32x4 dsw = dsr[i] * rw[i];
        float* ad = dst + (arow + 64 * i) * GX_KS + 4 * dq;
        *reinterpret_cast<f32x4*>(ad) = dsw * u * (1.0f - v * v);            // dPreV
        *reinterpret_cast<f32x4*>(ad + 16) = dsw * v * u * (1.0f - u);       // dPreU
    };
    auto b_load = [&](int i, int kk) { rb[i] = *reinterpret_cast<const f32x4*>(bsrc[i] + (size_t)(16 * kk) * L); };
    auto b_store = [&](int i, float* dst) { *reinterpret_cast<f32x4*>(dst + (bk + 8 * i) * 128 + 4 * bc4) = rb[i]; };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    constexpr int nslice = MIL_GATE_D / 16;   // 12
#pragma unroll
    for (int i = 0; i < 2; ++i) a_load(i, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) b_load(i, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) a_store(i, as);
#pragma unroll
    for (int i = 0; i < 4; ++i) b_store(i, bs);
#pragma unroll
    for (int i = 0; i < 2; ++i) a_load(i, 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) b_load(i, 1);
    __syncthreads();
    for (int s = 0; s < nslice; ++s) {
        const int buf = s & 1;
        const int k2 = min(s + 2, nslice - 1);
        const float* ab = as + buf * ASZ;
        const float* bb = bs + buf * BSZ;
        float* an = as + (buf ^ 1) * ASZ;
        float* bn = bs + (buf ^ 1) * BSZ;
        f32x4 fa[2][2], fb[2][2];     // [register set][tile]
        auto frag_a = [&](int t, int q, int a) {
            fa[q][a] = *reinterpret_cast<const f32x4*>(ab + (64 * wi + 32 * a + r) * GX_KS + 8 * t + 4 * h);
        };
        auto frag_b = [&](int t, int q, int b) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) fb[q][b][jj] = bb[(8 * t + 4 * h + jj) * 128 + 64 * wj + 32 * b + r];
        };
        frag_a(0, 0, 0); frag_a(0, 0, 1); frag_b(0, 0, 0); frag_b(0, 0, 1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = t & 1;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int g = 4 * t + jj;
                // staging pieces between MFMA groups: the next slice into LDS, registers reloaded with the slice after
                if (g == 2 || g == 4) { const int i = (g - 2) >> 1; a_store(i, an); a_load(i, k2); }
                if (g >= 6 && g < 10) { const int i = g - 6; b_store(i, bn); b_load(i, k2); }
                if (t < 3) {
                    if (jj == 0) frag_a(t + 1, q ^ 1, 0);
                    if (jj == 1) frag_a(t + 1, q ^ 1, 1);
                    if (jj == 2) frag_b(t + 1, q ^ 1, 0);
                    if (jj == 3) frag_b(t + 1, q ^ 1, 1);
                }
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0][jj], fb[q][0][jj], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0][jj], fb[q][1][jj], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1][jj], fb[q][0][jj], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1][jj], fb[q][1][jj], acc[1][1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
    // pool term: a_row and the bag of each of the tile's 128 rows, once per workgroup (the staging area is free: the loop's
    // last barrier has passed)
    float* s_arow = smem;
    int* s_bag = reinterpret_cast<int*>(smem + 128);
    if (dM != nullptr) {
        if (tid < 128) {
            const int gr = min(row0 + tid, R - 1);
            const int bg = row_bag[gr];                  // < 0: a padding row of a capacity bucket - no pool weight
            s_bag[tid] = max(bg, 0);
            s_arow[tid] = bg < 0 ? 0.f : expf(scores[gr] - lse[bg]);
        }
        __syncthreads();
    }
    // dx += tile: the 16 old values of a tile column are loaded as one batch before the adds
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float* o = dx + j0 + 64 * wj + 32 * b + r;
            const int rbase = row0 + 64 * wi + 32 * a;
            float cv[16];
            if (dM != nullptr) {
                const int col = j0 + 64 * wj + 32 * b + r;
                const int lr0 = 64 * wi + 32 * a;
#pragma unroll
                for (int i = 0; i < 16; ++i) cv[i] = dM[(size_t)s_bag[lr0 + mfma32_row(i, h)] * L + col];
#pragma unroll
                for (int i = 0; i < 16; ++i) cv[i] *= s_arow[lr0 + mfma32_row(i, h)];
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) cv[i] = o[(size_t)min(rbase + mfma32_row(i, h), R - 1) * L];
            }
            if (xbits != nullptr) {
                // this launch is the last writer of dx: the backward of the patch dropout (ABMIL.py:49) is applied here,
                // dx = keep ? (pool term + gate term) / (1 - p) : 0
                const int col = j0 + 64 * wj + 32 * b + r;
                unsigned mw[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) mw[i] = xbits[(size_t)min(rbase + mfma32_row(i, h), R - 1) * (L >> 5) + (col >> 5)];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int gr = rbase + mfma32_row(i, h);
                    if (gr < R) o[(size_t)gr * L] = ((mw[i] >> (col & 31)) & 1u) ? (cv[i] + acc[a][b][i]) * xscale : 0.f;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int gr = rbase + mfma32_row(i, h);
                    if (gr < R) o[(size_t)gr * L] = cv[i] + acc[a][b][i];
                }
            }
        }
}

// The same tile quantisation for dx (two 128 x 128 workgroups per CU): the rows beyond whole rounds, one workgroup
// per row, thread = four columns, d looped (W is L2-resident).
// One 16 x 16 output tile per workgroup (rows = tail rows, columns of L), the 8 waves split the 384 gate units, operands
// straight from global memory (16x16x4 MFMA, all loads of a wave issued before its first MFMA), partial tiles folded
// through LDS: every workgroup reads 24 KB of the weights.  (One workgroup per ROW streamed all 768 KB of Wv, Wu through a
// single CU: 21-23 us for 32 rows.)
__global__ __launch_bounds__(512) void k_gate_bwd_dx_tail(const float* __restrict__ gates, const float* __restrict__ ds,
                                                          const float* __restrict__ wvec, const float* __restrict__ Wv,
                                                          const float* __restrict__ Wu, float* __restrict__ dx, int L, int rows,
                                                          const uint32_t* __restrict__ xbits, float xscale,
                                                          const float* __restrict__ scores, const float* __restrict__ lse,
                                                          const int32_t* __restrict__ row_bag, const float* __restrict__ dM) {
    __shared__ float red[8][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
    const int mrow = min(m0 + r, rows - 1);
    const int jc = j0 + r;                                   // L % 16 == 0: always a valid column
    const float dsr = ds[mrow];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // wave w: gate units [24 w, 24 w + 24) of V and of U = 12 k-chunks of 4 units; A = dPre[row][unit], B = W[unit][column]
    f32x4 fa[12];
    float fb[12][4];
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int isu = u >= 6;
        const int d = 24 * wave + 4 * (u % 6);                    // first gate unit of the chunk (chunks 0-5: V half, 6-11: U half)
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(gates + (size_t)mrow * GF_NG + d);
        const f32x4 u4 = *reinterpret_cast<const f32x4*>(gates + (size_t)mrow * GF_NG + 192 + d);
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + d);
        const f32x4 dsw = dsr * w4;
        fa[u] = isu ? dsw * v4 * u4 * (1.0f - u4) : dsw * u4 * (1.0f - v4 * v4);
        const float* Wp = (isu ? Wu : Wv) + (size_t)d * L + jc;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) fb[u][jj] = Wp[(size_t)jj * L];
    }
    __builtin_amdgcn_sched_barrier(0);
    // 16x16x4: lane (r, kq) supplies A[m = r][k = kq] and B[k = kq][n = r]; the chunk's 4 units are its 4 k values, so the
    // A value of lane kq is component kq of the chunk's dPre vector and the B value is row kq of the chunk's weight rows
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const float av = kq == 0 ? fa[u][0] : kq == 1 ? fa[u][1] : kq == 2 ? fa[u][2] : fa[u][3];
        const float bv_ = kq == 0 ? fb[u][0] : kq == 1 ? fb[u][1] : kq == 2 ? fb[u][2] : fb[u][3];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv_, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    if (tid < 256) {
        const int i = tid >> 6, l = tid & 63;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += red[w][i][l];
        const int row = m0 + 4 * (l >> 4) + i, col = j0 + (l & 15);
        if (row < rows) {
            float* o = dx + (size_t)row * L + col;
            float t;
            if (dM != nullptr) {
                const int bg = row_bag[row];
                t = bg < 0 ? v : expf(scores[row] - lse[bg]) * dM[(size_t)bg * L + col] + v;
            } else {
                t = *o + v;
            }
            if (xbits != nullptr) t = ((xbits[(size_t)row * (L >> 5) + (col >> 5)] >> (col & 31)) & 1u) ? t * xscale : 0.f;
            *o = t;
        }
    }
}

static int gate_bwd_input_impl(const float* gates, const float* ds, const float* w, const float* Wv, const float* Wu,
                               int R, int L, int D, float* dx, const uint32_t* xbits, float xscale, const float* scores,
                               const float* lse, const int32_t* row_bag, const float* dM, void* stream) {
    if (!gates || !ds || !w || !Wv || !Wu || !dx) return MIL_EINVAL;
    if (D != MIL_GATE_D || L <= 0 || (L % 128) != 0 || R < 0) return MIL_EINVAL;
    if (R == 0) return MIL_OK;
    hipStream_t st = (hipStream_t)stream;
    const int per_round = 2 * MIL_NUM_CU / (L / 128);          // row tiles per round of the grid
    const int tail = per_round > 0 ? gate_tail_rows(R, per_round) : 0;
    const int Rm = R - tail;
    const int grid = ((Rm + 127) / 128) * (L / 128);
    hipLaunchKernelGGL(k_gate_bwd_dx, dim3(grid), dim3(256), 0, st, gates, ds, w, Wv, Wu, dx, Rm, L, xbits, xscale, scores, lse,
                       row_bag, dM);
    MIL_CHECK_LAUNCH();
    if (tail > 0) {
        hipLaunchKernelGGL(k_gate_bwd_dx_tail, dim3(L / 16, (tail + 15) / 16), dim3(512), 0, st, gates + (size_t)Rm * GF_NG, ds + Rm, w,
                           Wv, Wu, dx + (size_t)Rm * L, L, tail, xbits ? xbits + (size_t)Rm * (L >> 5) : nullptr, xscale,
                           scores ? scores + Rm : nullptr, lse, row_bag ? row_bag + Rm : nullptr, dM);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_gate_bwd_input(const float* gates, const float* ds, const float* w, const float* Wv, const float* Wu,
                                  int R, int L, int D, float* dx, const uint32_t* xbits, float xscale, void* stream) {
    return gate_bwd_input_impl(gates, ds, w, Wv, Wu, R, L, D, dx, xbits, xscale, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int mil_gate_bwd_input_pool(const float* gates, const float* ds, const float* w, const float* Wv,
                                       const float* Wu, int R, int L, int D, float* dx, const uint32_t* xbits, float xscale,
                                       const float* scores, const float* lse, const int32_t* row_bag, const float* dM,
                                       void* stream) {
    if (!scores || !lse || !row_bag || !dM) return MIL_EINVAL;
    return gate_bwd_input_impl(gates, ds, w, Wv, Wu, R, L, D, dx, xbits, xscale, scores, lse, row_bag, dM, stream);
}
