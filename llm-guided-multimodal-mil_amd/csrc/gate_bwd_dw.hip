// K1 backward: the gate weight gradient of the gated-attention MIL pooling (ABMIL) for gfx950.
//
// Reference arithmetic: torch autograd of model/dim1/ABMIL.py:47-56.  The transpose-product dPre^T . x is a dense
// contraction over the rows: v_mfma_f32_32x32x2_f32 (k_gate_bwd_dw, k_gate_bwd_dw2) or the split-bf16 loop
// (k_gate_bwd_dw2_pieces); the split-K fold is k_gate_bwd_reduce (gate_reduce.h).  Forward and route plan: gate_fwd.hip.
#include "mil_internal.h"
#include "gate_reduce.h"
#include <type_traits>

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// ================================================================================ K1 backward: gate dW (MFMA)
// dW[gi][j] = sum_rows dPre[row][gi] x[row][j], gi = permuted gate index: block m (0..2) holds
// d in [64m, 64m+64): local 0..63 -> dPreV_d, 64..127 -> dPreU_d, so one (V, U) load pair yields both.
// Workgroup 256 threads = 4 waves, output tile 128 (gi) x 128 (j), wave (wi, wj) owns 64 x 64.
// Split-K over row chunks of KC rows; partials [S][384][L] are summed by k_gate_bwd_reduce.
// Both operands are "k-major" in LDS ([row][i] and [row][j]): lane (i = l & 31, k = l >> 5) reads
// word row*128 + i: consecutive lanes -> consecutive banks, no conflicts, no padding.
#define GB_BKR 32
typedef unsigned short gb_u16x8 __attribute__((ext_vector_type(8)));

// XB16: x is stored as bf16 and widened to fp32 while it is staged (config-5 path; the product stays fp32 MFMA).
// KG: K groups per workgroup.  KG = 2 (tall inputs): 512 threads, the two halves of the workgroup run the same pipeline
// on the two halves of the row chunk (own LDS stages, common barriers) and fold their accumulators through LDS before the
// store, so a launch needs half as many row chunks for the same number of resident waves - half the partial tiles to
// write here and to read in k_gate_bwd_reduce.
template <bool XB16, int KG, bool DROP>
__global__ __launch_bounds__(256 * KG) void k_gate_bwd_dw(const void* __restrict__ xv, const float* __restrict__ gates,
                                                     const float* __restrict__ ds, const float* __restrict__ wvec,
                                                     float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                     int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                     const int32_t* __restrict__ rows_dev) {
    __shared__ __attribute__((aligned(16))) float smem_all[KG * 2 * 2 * GB_BKR * 128];
    if (rows_dev != nullptr) R = min(R, rows_dev[0]);      // bucketed batches: the true row count lives on the device
    const int grp = KG == 1 ? 0 : (int)(threadIdx.x >> 8);
    float* smem = smem_all + grp * (2 * 2 * GB_BKR * 128);      // this K group's stages
    float* ab = smem;                         // [2][32][128] dPre
    float* xb = smem + 2 * GB_BKR * 128;      // [2][32][128] x
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    // XCD-aware order: hardware deals workgroup ids round-robin over the 8 XCDs (id % 8 shares an L2).
    // The 3*NJ workgroups of one row chunk re-read the same x / gate rows, so give them consecutive
    // slots of ONE XCD: logical = (id % 8) * ceil-share + id / 8 (bijective form for any grid size).
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    }
    const int jt = bid % NJ, m = (bid / NJ) % 3, s = bid / (3 * NJ);
    const int j0 = jt * 128;
    // row chunk of the workgroup, then this K group's part of it (whole slices to group 0 first); the slice loop runs
    // nloop times for everybody (common barriers): iterations past a group's own slices multiply dead copies (ds = 0)
    const int cbeg = min(s * KC, R), cend = min(R, cbeg + KC);
    const int half = KG == 1 ? cend - cbeg : ((cend - cbeg + 2 * GB_BKR - 1) / (2 * GB_BKR)) * GB_BKR;
    const int rbeg = min(cend, cbeg + grp * half), rend = KG == 1 ? cend : min(cend, rbeg + half);
    const int nslice = (rend - rbeg + GB_BKR - 1) / GB_BKR;
    const int nloop = (min(half, cend - cbeg) + GB_BKR - 1) / GB_BKR;

    const float* x = static_cast<const float*>(xv);
    const unsigned short* xh = static_cast<const unsigned short*>(xv);
    // staging maps
    const int xrow = tid >> 5, xc4 = tid & 31;    // x: rows xrow + 8i (i < 4), 16-byte chunk xc4
    const int hrow = tid >> 4, hc8 = tid & 15;    // bf16 x: rows hrow + 16i (i < 2), 16-byte chunk (8 columns) hc8
    gb_u16x8 rh[2];
    const int arow = tid >> 4, ad4 = tid & 15;    // gates: rows arow + 16i (i < 2), d = 64m + 4*ad4
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * m + 4 * ad4);
    f32x4 rx[4], rv[2], ru[2];
    unsigned rm[4] = {0, 0, 0, 0};   // train mode: keep bits of the staged x chunks (the forward's mask, csrc/dropout.hip)
    float rds[2], rmask[2];      // raw ds value and its validity mask (applied at use, never at load)
    f32x4 acc_bv = {0, 0, 0, 0}, acc_bu = {0, 0, 0, 0}, acc_w = {0, 0, 0, 0};
    float acc_ds = 0.f;

    // Branch-free staging pieces (rows past the chunk end are clamped to its last row and get ds = 0, so they
    // add nothing): the loop body is one basic block and every piece sits between two MFMA groups.
    const int LW = L >> 5;
    auto xload = [&](int i, int rs) {
        if (XB16) {
            if (i < 2) {
                const int gr = max(min(rs + hrow + 16 * i, rend - 1), 0);
                rh[i] = *reinterpret_cast<const gb_u16x8*>(xh + (size_t)gr * L + j0 + 8 * hc8);
                if (DROP) rm[i] = xbits[(size_t)gr * LW + ((j0 + 8 * hc8) >> 5)];
            }
        } else {
            const int gr = max(min(rs + xrow + 8 * i, rend - 1), 0);
            rx[i] = *reinterpret_cast<const f32x4*>(x + (size_t)gr * L + j0 + 4 * xc4);
            if (DROP) rm[i] = xbits[(size_t)gr * LW + ((j0 + 4 * xc4) >> 5)];
        }
    };
    auto xwrite = [&](int i, int buf) {
        if (XB16) {
            if (i < 2) {
                float* dst = xb + (buf * GB_BKR + hrow + 16 * i) * 128 + 8 * hc8;
                f32x4 lo, hi;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lo[e] = __uint_as_float(((unsigned)rh[i][e]) << 16);
                    hi[e] = __uint_as_float(((unsigned)rh[i][4 + e]) << 16);
                }
                if (DROP) {
                    const unsigned mm = rm[i] >> (8 * (hc8 & 3));
#pragma unroll
                    for (int e = 0; e < 4; ++e) { lo[e] = keep_if(lo[e], mm, e); hi[e] = keep_if(hi[e], mm, 4 + e); }
                }
                *reinterpret_cast<f32x4*>(dst) = lo;
                *reinterpret_cast<f32x4*>(dst + 4) = hi;
            }
        } else {
            f32x4 v = rx[i];
            if (DROP) {
                const unsigned mm = rm[i] >> (4 * (xc4 & 7));
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = keep_if(v[e], mm, e);
            }
            *reinterpret_cast<f32x4*>(xb + (buf * GB_BKR + xrow + 8 * i) * 128 + 4 * xc4) = v;
        }
    };
    auto aload = [&](int i, int rs, bool live) {
        const int gr = rs + arow + 16 * i;
        const int gc = max(min(gr, rend - 1), 0);
        const float* gp = gates + (size_t)gc * GF_NG + 64 * m + 4 * ad4;
        rv[i] = *reinterpret_cast<const f32x4*>(gp);
        ru[i] = *reinterpret_cast<const f32x4*>(gp + 192);
        rds[i] = ds[gc];                                  // unconditional load: keeps the body branch-free
        rmask[i] = (live && gr < rend) ? 1.f : 0.f;
    };
    // dPreV = ds w U (1 - V^2) = a - (a V) V and dPreU = ds w V U (1 - U) = t - t U with a = ds w U, t = a V: four VALU
    // per (V, U) pair instead of seven.  (The bias / w / b sums stay unconditional: a wave-uniform `jt == 0` branch around
    // them splits the k-step into basic blocks and costs more than the six VALU it saves.)
    f32x4 rt[2];
    auto awrite_v = [&](int i, int buf) {
        const f32x4 v = rv[i];
        const f32x4 a = ((rds[i] * rmask[i]) * w4) * ru[i];
        const f32x4 t = a * v;
        const f32x4 pv = a - t * v;
        rt[i] = t;
        *reinterpret_cast<f32x4*>(ab + (buf * GB_BKR + arow + 16 * i) * 128 + 4 * ad4) = pv;
        acc_bv += pv;
    };
    auto awrite_u = [&](int i, int buf) {
        const f32x4 t = rt[i], u = ru[i];
        const f32x4 pu = t - t * u;
        *reinterpret_cast<f32x4*>(ab + (buf * GB_BKR + arow + 16 * i) * 128 + 64 + 4 * ad4) = pu;
        const float dsv = rds[i] * rmask[i];
        acc_bu += pu;
        acc_w += (dsv * rv[i]) * u;
        if (ad4 == 0) acc_ds += dsv;
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    {
#pragma unroll
        for (int i = 0; i < 4; ++i) xload(i, rbeg);
#pragma unroll
        for (int i = 0; i < 2; ++i) aload(i, rbeg, nslice > 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) xwrite(i, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) { awrite_v(i, 0); awrite_u(i, 0); }
        const int rs1 = rbeg + max(min(1, nslice - 1), 0) * GB_BKR;
#pragma unroll
        for (int i = 0; i < 4; ++i) xload(i, rs1);
#pragma unroll
        for (int i = 0; i < 2; ++i) aload(i, rs1, nslice > 1);   // a single-slice chunk must not count slice 0 twice
    }
    __syncthreads();
    // Issue order inside a k-step.  The two waves of a SIMD (w and w + 4) share its matrix pipe and the older one wins every
    // arbitration: measured with in-kernel cycle stamps (docs/lab_notes.md), waves 0-3 spent 29 % of the loop parked at the
    // slice barrier while waves 4-7, starved until then, finished the slice ALONE.  A wave on its own only keeps the pipe
    // busy if its non-matrix instructions sit in the shadow of its own MFMAs, so the k-step is laid out as
    //     MFMA . fragment reads . MFMA . staging part a . MFMA . staging part b . MFMA . staging part c
    // (one v_mfma_f32_32x32x2_f32 occupies the pipe for 64 cycles; a part is a handful of VALU / one LDS write / one or
    // two global loads), each boundary pinned with sched_barrier: hipcc otherwise gathers the staging in front of a
    // block of four MFMAs, behind which the wave sits blocked for 3 x 64 cycles with nothing else to issue.
    auto slice_body = [&](int sl) {
        const int buf = sl & 1;
        // registers hold slice sl+1 (or, past this group's last slice, a dead copy with ds forced to 0)
        const bool live2 = sl + 2 < nslice;
        const int rs2 = rbeg + max(min(sl + 2, nslice - 1), 0) * GB_BKR;
        const float* ap = ab + buf * GB_BKR * 128 + h * 128 + 64 * wi + r;
        const float* bp = xb + buf * GB_BKR * 128 + h * 128 + 64 * wj + r;
        float fa[2][2], fb[2][2];
        fa[0][0] = ap[0]; fa[0][1] = ap[32]; fb[0][0] = bp[0]; fb[0][1] = bp[32];
        // staging parts of k-step ks (p = 0, 1, 2): LDS image of slice sl+1 from the registers, registers reloaded with sl+2
        auto part = [&](int ks, int p) {
            if (ks >= 1 && ks <= 4) {
                if (p == 0) xwrite(ks - 1, buf ^ 1);
                if (p == 1) xload(ks - 1, rs2);
            }
            if (ks == 5 && p == 0) awrite_v(0, buf ^ 1);
            if (ks == 6 && p == 0) awrite_u(0, buf ^ 1);
            if (ks == 6 && p == 1) aload(0, rs2, live2);
            if (ks == 7 && p == 0) awrite_v(1, buf ^ 1);
            if (ks == 8 && p == 0) awrite_u(1, buf ^ 1);
            if (ks == 8 && p == 1) aload(1, rs2, live2);
        };
#pragma unroll
        for (int ks = 0; ks < GB_BKR / 2; ++ks) {
            const int q = ks & 1;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][0], acc[0][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < GB_BKR / 2) {
                fa[q ^ 1][0] = ap[(ks + 1) * 256]; fa[q ^ 1][1] = ap[(ks + 1) * 256 + 32];
                fb[q ^ 1][0] = bp[(ks + 1) * 256]; fb[q ^ 1][1] = bp[(ks + 1) * 256 + 32];
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][1], acc[0][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            part(ks, 0);
            __builtin_amdgcn_sched_barrier(0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][0], acc[1][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            part(ks, 1);
            __builtin_amdgcn_sched_barrier(0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][1], acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            part(ks, 2);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int sl = 0; sl < nloop; ++sl) {
        slice_body(sl);
        __syncthreads();
    }

    // partial tile -> part[s][128m + 64wi + row][j0 + 64wj + col].  The accumulators hold a column per lane (16 rows
    // each); going through LDS turns 64 four-byte stores per lane into sixteen-byte ones: every wave writes its 64 x 64
    // tile row-major into its own 16 KB of its group's (now dead) staging area (stride 64 is conflict-free both ways).
    // KG = 2: both K groups do that, then the two waves that own the same tile (one per group) each fold and store HALF
    // of its rows - one LDS round trip and all eight waves storing, instead of fold -> transpose -> store by four.
    {
        __syncthreads();                                  // the staging buffers are dead from here on
        float* tw = smem + wave * (64 * 64);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) tw[(32 * a + mfma32_row(i, h)) * 64 + 32 * b + r] = acc[a][b][i];
        if (KG == 2) __syncthreads();                     // KG = 1: same-wave write -> read, ordered by lgkmcnt
        float* pt = part + ((size_t)s * GF_NG + 128 * m + 64 * wi) * L + j0 + 64 * wj;
        const int c4 = lane & 15, rr = lane >> 4;         // 16 float4 columns x 4 rows per pass
        const float* t0 = smem_all + wave * (64 * 64);
        const float* t1 = smem_all + (2 * 2 * GB_BKR * 128) + wave * (64 * 64);
        constexpr int NP = 16 / KG;
#pragma unroll
        for (int pass = 0; pass < NP; ++pass) {
            const int row = 4 * (pass + NP * grp) + rr;
            f32x4 v = *reinterpret_cast<const f32x4*>(t0 + row * 64 + 4 * c4);
            if (KG == 2) v += *reinterpret_cast<const f32x4*>(t1 + row * 64 + 4 * c4);
            *reinterpret_cast<f32x4*>(pt + (size_t)row * L + 4 * c4) = v;
        }
    }

    // bias / w partials (only the j-tile-0 workgroups publish them); both K groups contribute their row groups
    if (jt == 0) {
        float* redf = smem_all;   // [16 KG row groups][3][64]
        const int arow_all = arow + 16 * grp;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            redf[(arow_all * 3 + 0) * 64 + 4 * ad4 + e] = acc_bv[e];
            redf[(arow_all * 3 + 1) * 64 + 4 * ad4 + e] = acc_bu[e];
            redf[(arow_all * 3 + 2) * 64 + 4 * ad4 + e] = acc_w[e];
        }
        __syncthreads();
        if (grp == 0 && tid < 192) {
            const int which = tid / 64, d = tid % 64;
            float v = 0.f;
#pragma unroll
            for (int g = 0; g < 16 * KG; ++g) v += redf[(g * 3 + which) * 64 + d];
            pbias[((size_t)s * 4 + which) * 192 + 64 * m + d] = v;
        }
        if (m == 0) {
            __syncthreads();
            redf[threadIdx.x] = acc_ds;
            __syncthreads();
            if (threadIdx.x == 0) {
                float v = 0.f;
                for (int g = 0; g < 256 * KG; g += 16) v += redf[g];
                pbias[((size_t)s * 4 + 3) * 192] = v;
            }
        }
    }
}


// The epilogue shared by k_gate_bwd_dw2 and k_gate_bwd_dw2_pieces (512 threads: two K groups x four waves, wave (wi, wj) of
// either group holding a partial 64 x 64 tile of the same output; smem_all = the 128 KiB staging area, dead by now).
// partial tile -> part[s][128m + 64wi + row][j0 + 64wj + col]: every wave writes its 64 x 64 tile row-major into its own
// 16 KB of its group's half; the two waves that own the same tile (one per K group) each fold and store half of its rows
// with 16-byte stores.
__device__ __forceinline__ void dw2_store_tile(float* smem_all, const f32x16 (&acc)[2][2], float* __restrict__ part, int s, int m,
                                               int L, int j0, int grp, int wave, int lane) {
    const int wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    float* tw = smem_all + grp * (2 * 2 * GB_BKR * 128) + wave * (64 * 64);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) tw[(32 * a + mfma32_row(i, h)) * 64 + 32 * b + r] = acc[a][b][i];
    __syncthreads();
    float* pt = part + ((size_t)s * GF_NG + 128 * m + 64 * wi) * L + j0 + 64 * wj;
    const int c4 = lane & 15, rr = lane >> 4;
    const float* t0 = smem_all + wave * (64 * 64);
    const float* t1 = smem_all + (2 * 2 * GB_BKR * 128) + wave * (64 * 64);
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int row = 4 * (pass + 8 * grp) + rr;
        const f32x4 v = *reinterpret_cast<const f32x4*>(t0 + row * 64 + 4 * c4) +
                        *reinterpret_cast<const f32x4*>(t1 + row * 64 + 4 * c4);
        *reinterpret_cast<f32x4*>(pt + (size_t)row * L + 4 * c4) = v;
    }
}
// bias / w / b partials: every (s, jt) workgroup publishes the sums of its share of the slices -> pbias[s][jt][4][192].
// arow_all (0..31), ad4: the thread's row group and float4 column of the dPre staging map.
__device__ __forceinline__ void dw2_publish_sums(float* smem_all, float* __restrict__ pbias, int s, int NJ, int jt, int m,
                                                 int arow_all, int ad4, const f32x4 acc_bv, const f32x4 acc_bu,
                                                 const f32x4 acc_w, float acc_ds) {
    float* redf = smem_all;   // [32 row groups][3][64]
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        redf[(arow_all * 3 + 0) * 64 + 4 * ad4 + e] = acc_bv[e];
        redf[(arow_all * 3 + 1) * 64 + 4 * ad4 + e] = acc_bu[e];
        redf[(arow_all * 3 + 2) * 64 + 4 * ad4 + e] = acc_w[e];
    }
    __syncthreads();
    float* pb = pbias + ((size_t)s * NJ + jt) * 4 * 192;
    if (threadIdx.x < 192) {
        const int which = threadIdx.x / 64, d = threadIdx.x % 64;
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 32; ++g) v += redf[(g * 3 + which) * 64 + d];
        pb[which * 192 + 64 * m + d] = v;
    }
    if (m == 0) {
        __syncthreads();
        redf[threadIdx.x] = acc_ds;
        __syncthreads();
        if (threadIdx.x == 0) {
            float v = 0.f;
            for (int g = 0; g < 512; g += 16) v += redf[g];
            pb[3 * 192] = v;
        }
    }
}

// ================================================================================ K1 backward: gate dW, "VALU diet" form
// Same product, tiling, split-K layout, k order and outputs (bit for bit) as k_gate_bwd_dw<false, 2, *>; what changes is
// how little VECTOR-ALU work the main loop carries.  Measured on MI355X (tools/mfma_valu_mix.hip): unlike the bf16 MFMAs,
// v_mfma_f32_32x32x2_f32 does NOT hide VALU instructions issued around it - it runs at the f32 VALU rate and every
// v_fma / v_and between two of them costs 3-5 cycles of matrix time, at one or two waves per SIMD alike (4 fillers per
// MFMA: 64 -> 84 cycles; LDS reads, scalar ALU and s_nop fillers are free).  The first kernel spent ~230 VALU
// instructions per wave and 32-row slice (64 MFMAs) on 64-bit address arithmetic, row clamps, LDS addresses, masks:
// 27 % of the loop.  Here
//   * global operands come through buffer resources whose base / size live in SGPRs and advance by scalar ALU: the
//     per-lane offset is a loop invariant, rows beyond the K group's end read as ZERO by the hardware range check (no
//     clamps, no validity masks - a zero ds row contributes nothing);
//   * both LDS images store their four 32-column blocks in the order {0, 2, 1, 3}, so the two operand values a lane
//     needs per k-step are 64 dwords apart and ONE ds_read2st64_b32 with immediate offsets fetches them (no address
//     VALU; the buffer index is a compile-time constant: the slice loop is unrolled by two);
//   * the bias / w / b sums are spread over the NJ column-tile workgroups of a row chunk (slice sl is summed by the
//     workgroup with jt == sl % NJ, scalar branch) instead of being summed by all of them and published by one.
// What is left is the arithmetic itself: dPre (20 VALU per (V, U) float4 pair) and, in train mode, the keep mask of x.

template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_bwd_dw2(const float* __restrict__ x, const float* __restrict__ gates,
                                                      const float* __restrict__ ds, const float* __restrict__ wvec,
                                                      float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                      int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                      const int32_t* __restrict__ rows_dev) {
    __shared__ __attribute__((aligned(16))) float smem_all[2 * 2 * 2 * GB_BKR * 128];
    if (rows_dev != nullptr) R = min(R, __builtin_amdgcn_readfirstlane(rows_dev[0]));      // bucketed batches: true row count on the device
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    float* smem = smem_all + grp * (2 * 2 * GB_BKR * 128);      // this K group's stages: [2][32][128] dPre, [2][32][128] x
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    }
    const int jt = bid % NJ, m = (bid / NJ) % 3, s = bid / (3 * NJ);
    const int j0 = jt * 128;
    const int cbeg = min(s * KC, R), cend = min(R, cbeg + KC);
    const int half = ((cend - cbeg + 2 * GB_BKR - 1) / (2 * GB_BKR)) * GB_BKR;
    const int rbeg = min(cend, cbeg + grp * half), rend = min(cend, rbeg + half);
    const int nloop = (min(half, cend - cbeg) + GB_BKR - 1) / GB_BKR;      // common to both groups (shared barriers)

    // per-lane byte offsets inside a slice (loop invariants)
    const int xrow = tid >> 5, xc4 = tid & 31;    // x: rows xrow + 8i (i < 4), 16-byte chunk xc4 of the 128-column tile
    const int arow = tid >> 4, ad4 = tid & 15;    // gates: rows arow + 16i (i < 2), d = 64m + 4 ad4
    const int LW = L >> 5;
    int vx[4], vm[4], vg[2], vd[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        vx[i] = ((xrow + 8 * i) * L + j0 + 4 * xc4) * 4;
        vm[i] = ((xrow + 8 * i) * LW + ((j0 + 4 * xc4) >> 5)) * 4;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        vg[i] = ((arow + 16 * i) * GF_NG + 64 * m + 4 * ad4) * 4;
        vd[i] = (arow + 16 * i) * 4;
    }
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * m + 4 * ad4);
    // LDS positions: 32-column blocks stored in the order {0, 2, 1, 3}
    auto blkpos = [](int c) { return (c & 31) | ((c & 32) << 1) | ((c & 64) >> 1); };
    float* const ab = smem;                       // [2][32][128]
    float* const xb = smem + 2 * GB_BKR * 128;    // [2][32][128]
    float* const xw = xb + xrow * 128 + blkpos(4 * xc4);              // + (buf * 32 + 8 i) * 128
    float* const aw = ab + arow * 128 + blkpos(4 * ad4);              // V block; U block: blkpos(64 + 4 ad4) = + 32
    const float* const ap = ab + h * 128 + 32 * wi + r;               // + buf * 4096 + ks * 256 (+ 64)
    const float* const bp = xb + h * 128 + 32 * wj + r;

    u32x4_t rx[4], rv[2], ru[2];
    unsigned rm[4] = {0, 0, 0, 0};
    float rds[2];
    f32x4 rt[2];
    f32x4 acc_bv = {0, 0, 0, 0}, acc_bu = {0, 0, 0, 0}, acc_w = {0, 0, 0, 0};
    float acc_ds = 0.f;

    // scalar: resources of slice `row0`.  Rows >= rend are out of range -> the loads return zeros.
    auto x_srd = [&](int row0) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)row0 * L), 0, max(rend - row0, 0) * L * 4, MIL_SRD_FLAGS);
    };
    auto g_srd = [&](int row0) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(gates + (size_t)row0 * GF_NG), 0, max(rend - row0, 0) * GF_NG * 4,
                                                 MIL_SRD_FLAGS);
    };
    auto d_srd = [&](int row0) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(ds + row0), 0, max(rend - row0, 0) * 4, MIL_SRD_FLAGS);
    };
    auto m_srd = [&](int row0) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(xbits + (size_t)row0 * LW), 0, max(rend - row0, 0) * LW * 4,
                                                 MIL_SRD_FLAGS);
    };
    auto xload = [&](int i, int row0) {
        rx[i] = __builtin_amdgcn_raw_buffer_load_b128(x_srd(row0), vx[i], 0, 0);
        if (DROP) rm[i] = __builtin_amdgcn_raw_buffer_load_b32(m_srd(row0), vm[i], 0, 0);
    };
    auto aload = [&](int i, int row0) {
        const __amdgpu_buffer_rsrc_t g = g_srd(row0);
        rv[i] = __builtin_amdgcn_raw_buffer_load_b128(g, vg[i], 0, 0);
        ru[i] = __builtin_amdgcn_raw_buffer_load_b128(g, vg[i] + 192 * 4, 0, 0);
        rds[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(d_srd(row0), vd[i], 0, 0));
    };
    auto xwrite = [&](int i, int buf) {
        f32x4 v = __builtin_bit_cast(f32x4, rx[i]);
        if (DROP) {
            const unsigned mm = rm[i] >> (4 * (xc4 & 7));
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = keep_if(v[e], mm, e);
        }
        *reinterpret_cast<f32x4*>(xw + (buf * GB_BKR + 8 * i) * 128) = v;
    };
    auto awrite_v = [&](int i, int buf) {           // dPreV = a - (a V) V,  a = ds w U
        const f32x4 v = __builtin_bit_cast(f32x4, rv[i]);
        const f32x4 a = (rds[i] * w4) * __builtin_bit_cast(f32x4, ru[i]);
        const f32x4 t = a * v;
        rt[i] = t;
        *reinterpret_cast<f32x4*>(aw + (buf * GB_BKR + 16 * i) * 128) = a - t * v;
    };
    auto awrite_u = [&](int i, int buf, bool pub) { // dPreU = t - t U,  t = ds w U V
        const f32x4 t = rt[i], u = __builtin_bit_cast(f32x4, ru[i]);
        const f32x4 pu = t - t * u;
        *reinterpret_cast<f32x4*>(aw + (buf * GB_BKR + 16 * i) * 128 + 32) = pu;
        if (pub) {                                    // scalar branch: this slice's sums belong to this workgroup
            const f32x4 v = __builtin_bit_cast(f32x4, rv[i]);
            acc_bv += (rds[i] * w4) * u - t * v;      // = dPreV again (3 VALU per element, only every NJ-th slice)
            acc_bu += pu;
            acc_w += (rds[i] * v) * u;
            if (ad4 == 0) acc_ds += rds[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    // prologue: slice 0 -> LDS buffer 0, slice 1 -> registers
#pragma unroll
    for (int i = 0; i < 4; ++i) xload(i, rbeg);
#pragma unroll
    for (int i = 0; i < 2; ++i) aload(i, rbeg);
#pragma unroll
    for (int i = 0; i < 4; ++i) xwrite(i, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) { awrite_v(i, 0); awrite_u(i, 0, jt == 0); }
#pragma unroll
    for (int i = 0; i < 4; ++i) xload(i, rbeg + GB_BKR);
#pragma unroll
    for (int i = 0; i < 2; ++i) aload(i, rbeg + GB_BKR);
    __syncthreads();

    // one slice: 16 k-steps x 4 MFMAs; between the MFMAs the parts that stage slice sl + 1 and reload slice sl + 2
    auto slice = [&](int sl, auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        const int row2 = rbeg + (sl + 2) * GB_BKR;
        const bool pub = ((sl + 1) % NJ) == jt;                     // the slice being written now is sl + 1
        const float* apb = ap + buf * GB_BKR * 128;
        const float* bpb = bp + buf * GB_BKR * 128;
        float fa[2][2], fb[2][2];
        fa[0][0] = apb[0]; fa[0][1] = apb[64]; fb[0][0] = bpb[0]; fb[0][1] = bpb[64];
#pragma unroll
        for (int ks = 0; ks < GB_BKR / 2; ++ks) {
            const int q = ks & 1;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][0], acc[0][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < GB_BKR / 2) {
                fa[q ^ 1][0] = apb[(ks + 1) * 256]; fa[q ^ 1][1] = apb[(ks + 1) * 256 + 64];
                fb[q ^ 1][0] = bpb[(ks + 1) * 256]; fb[q ^ 1][1] = bpb[(ks + 1) * 256 + 64];
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][1], acc[0][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks >= 1 && ks <= 4) xwrite(ks - 1, buf ^ 1);
            if (ks == 5) awrite_v(0, buf ^ 1);
            if (ks == 6) awrite_u(0, buf ^ 1, pub);
            if (ks == 7) awrite_v(1, buf ^ 1);
            if (ks == 8) awrite_u(1, buf ^ 1, pub);
            __builtin_amdgcn_sched_barrier(0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][0], acc[1][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (ks >= 1 && ks <= 4) xload(ks - 1, row2);
            if (ks == 6) aload(0, row2);
            if (ks == 8) aload(1, row2);
            __builtin_amdgcn_sched_barrier(0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][1], acc[1][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    int sl = 0;
    for (; sl + 1 < nloop; sl += 2) {
        slice(sl, std::integral_constant<int, 0>{});
        __syncthreads();
        slice(sl + 1, std::integral_constant<int, 1>{});
        __syncthreads();
    }
    if (sl < nloop) {
        slice(sl, std::integral_constant<int, 0>{});
        __syncthreads();
    }

    dw2_store_tile(smem_all, acc, part, s, m, L, j0, grp, wave, lane);
    dw2_publish_sums(smem_all, pbias, s, NJ, jt, m, arow + 16 * grp, ad4, acc_bv, acc_bu, acc_w, acc_ds);
}

// ================================================================================ K1 backward: gate dW, split-bf16 K loop
// The product of k_gate_bwd_dw2 with its K loop on v_mfma_f32_32x32x16_bf16, as the forward's PW loop: every staged fp32
// value - dPreV / dPreU built from gates, ds, w and the keep-masked x - is split ONCE, while it is staged, into three exact
// bf16 pieces (gp_split3: a dropped element is zeroed first, a row beyond the chunk reads as zero, a zero splits to three
// zeros, a non-finite value keeps p0 = the inf / NaN and p1 = p2 = 0), and the contraction keeps the six cross terms (p, q)
// with p + q <= 2, smallest first: 192 matrix cycles per 16 k and tile where the f32 MFMA takes 512.  Grid, split-K chunks,
// XCD order, rows_dev clamp, part / pbias layout and the spreading of the bias / w / b sums (fp32 VALU on the unsplit
// values) are those of k_gate_bwd_dw2; MIL_DW_PIECES=0 keeps that kernel.
// LDS image: three pieces take 6 B per element, so two K groups with 32-row slices of their own (the f32 kernel's 128 KiB)
// would need 192 KiB.  Here ONE stage pair serves all eight waves: a stage is a 32-row slice of both operands, 3 pieces x
// [32][WB_S = 160] bf16 each (k-major as in memory; fragments come transposed from ds_read_b64_tr_b16, tr_frag) = 60 KiB,
// two stages 120 KiB.  The "K groups" are the two 16-row halves of every slice: waves 0-3 multiply rows 0-15, waves 4-7 rows
// 16-31, each wave on a 64 x 64 tile (12 fragments, 24 MFMAs per slice), and the epilogue folds the two halves as before.
// Every element is staged (and split) once per workgroup, by 512 threads instead of 256.
// Pipeline: one barrier per slice, in the MIDDLE of its 24 MFMAs.  Before it the wave lays the staging of slice sl + 1
// (split + LDS writes, then the global loads of slice sl + 2) between the twelve MFMAs of the small terms; after it the
// fragments of slice sl + 1 are read into the other register set under the twelve MFMAs of the large terms (the bf16 MFMA
// hides VALU and LDS issue, tools/mfma_valu_mix.hip).
#define GQ_PSZ (GB_BKR * WB_S)          /* one piece of one operand: [32][160] bf16 (10 KiB) */
#define GQ_BUF (6 * GQ_PSZ)             /* one stage: dPre pieces 0..2, x pieces 0..2 (60 KiB) */
template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_bwd_dw2_pieces(const float* __restrict__ x, const float* __restrict__ gates,
                                                             const float* __restrict__ ds, const float* __restrict__ wvec,
                                                             float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                             int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                             const int32_t* __restrict__ rows_dev) {
    // 128 KiB: the two stages take 120 KiB, the epilogue's eight 64 x 64 fp32 tiles all of it
    __shared__ __attribute__((aligned(16))) float smem_all[2 * 2 * 2 * GB_BKR * 128];
    static_assert(2 * GQ_BUF * 2 <= (int)sizeof(smem_all), "stages exceed the LDS image");
    unsigned short* const img = reinterpret_cast<unsigned short*>(smem_all);
    if (rows_dev != nullptr) R = min(R, __builtin_amdgcn_readfirstlane(rows_dev[0]));      // bucketed batches: true row count on the device
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));               // which 16 rows of every slice
    const int T = threadIdx.x, tid = T & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int h = lane >> 5;
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;                  // transpose-read address roles
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
        bid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    }
    const int jt = bid % NJ, m = (bid / NJ) % 3, s = bid / (3 * NJ);
    const int j0 = jt * 128;
    const int rbeg = min(s * KC, R), rend = min(R, rbeg + KC);
    const int nloop = (rend - rbeg + GB_BKR - 1) / GB_BKR;

    // per-lane byte offsets inside a slice (loop invariants)
    const int xrow = T >> 5, xc4 = T & 31;        // x: rows xrow + 16i (i < 2), 16-byte chunk xc4 of the 128-column tile
    const int arow = T >> 4, ad4 = T & 15;        // gates: row arow, d = 64m + 4 ad4
    const int LW = L >> 5;
    int vx[2], vm[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        vx[i] = ((xrow + 16 * i) * L + j0 + 4 * xc4) * 4;
        vm[i] = ((xrow + 16 * i) * LW + ((j0 + 4 * xc4) >> 5)) * 4;
    }
    const int vg = (arow * GF_NG + 64 * m + 4 * ad4) * 4, vd = arow * 4;
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * m + 4 * ad4);
    unsigned short* const xw = img + 3 * GQ_PSZ + xrow * WB_S + 4 * xc4;     // + buf * GQ_BUF + 16 i * WB_S; piece q: + q * GQ_PSZ
    unsigned short* const aw = img + arow * WB_S + 4 * ad4;                  // V columns 0..63; U: + 64
    const int frow = 16 * grp + 8 * h + tq;
    const int acol = 64 * wi + 16 * tg + 4 * tp;                             // + 32 a
    const int bcol = 64 * wj + 16 * tg + 4 * tp;                             // + 32 b

    u32x4_t rx[2], rv, ru;
    unsigned rm[2] = {0, 0};
    float rds;
    f32x4 rt;
    f32x4 acc_bv = {0, 0, 0, 0}, acc_bu = {0, 0, 0, 0}, acc_w = {0, 0, 0, 0};
    float acc_ds = 0.f;

    // resources of slice `row0`: rows >= rend are out of range -> the loads return zeros
    auto xload = [&](int i, int row0) {
        const int left = max(rend - row0, 0);
        rx[i] = __builtin_amdgcn_raw_buffer_load_b128(
            __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)row0 * L), 0, left * L * 4, MIL_SRD_FLAGS), vx[i], 0, 0);
        if (DROP)
            rm[i] = __builtin_amdgcn_raw_buffer_load_b32(
                __builtin_amdgcn_make_buffer_rsrc((void*)(xbits + (size_t)row0 * LW), 0, left * LW * 4, MIL_SRD_FLAGS), vm[i], 0, 0);
    };
    auto aload = [&](int row0) {
        const int left = max(rend - row0, 0);
        const __amdgpu_buffer_rsrc_t g =
            __builtin_amdgcn_make_buffer_rsrc((void*)(gates + (size_t)row0 * GF_NG), 0, left * GF_NG * 4, MIL_SRD_FLAGS);
        rv = __builtin_amdgcn_raw_buffer_load_b128(g, vg, 0, 0);
        ru = __builtin_amdgcn_raw_buffer_load_b128(g, vg + 192 * 4, 0, 0);
        rds = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            __builtin_amdgcn_make_buffer_rsrc((void*)(ds + row0), 0, left * 4, MIL_SRD_FLAGS), vd, 0, 0));
    };
    auto put3 = [&](unsigned short* dst, const f32x4 v) {          // four columns of one row: one 8-byte store per piece
        ushort4 o[3];
        gp_split3(v[0], o[0].x, o[1].x, o[2].x);
        gp_split3(v[1], o[0].y, o[1].y, o[2].y);
        gp_split3(v[2], o[0].z, o[1].z, o[2].z);
        gp_split3(v[3], o[0].w, o[1].w, o[2].w);
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<ushort4*>(dst + q * GQ_PSZ) = o[q];
    };
    auto xwrite = [&](int i, int buf) {
        f32x4 v = __builtin_bit_cast(f32x4, rx[i]);
        if (DROP) {
            const unsigned mm = rm[i] >> (4 * (xc4 & 7));
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = keep_if(v[e], mm, e);
        }
        put3(xw + buf * GQ_BUF + 16 * i * WB_S, v);
    };
    auto awrite_v = [&](int buf) {                  // dPreV = a - (a V) V,  a = ds w U
        const f32x4 v = __builtin_bit_cast(f32x4, rv);
        const f32x4 a = (rds * w4) * __builtin_bit_cast(f32x4, ru);
        const f32x4 t = a * v;
        rt = t;
        put3(aw + buf * GQ_BUF, a - t * v);
    };
    auto awrite_u = [&](int buf, bool pub) {        // dPreU = t - t U,  t = ds w U V
        const f32x4 t = rt, u = __builtin_bit_cast(f32x4, ru);
        const f32x4 pu = t - t * u;
        put3(aw + buf * GQ_BUF + 64, pu);
        if (pub) {                                    // scalar branch: this slice's sums belong to this workgroup
            const f32x4 v = __builtin_bit_cast(f32x4, rv);
            acc_bv += (rds * w4) * u - t * v;
            acc_bu += pu;
            acc_w += (rds * v) * u;
            if (ad4 == 0) acc_ds += rds;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    gp_u16x8 fa[2][3][2], fb[2][3][2];              // [register set][piece][tile]
    auto frags = [&](auto set_c, int buf) {         // smallest piece first: the small terms are multiplied first
        constexpr int set = decltype(set_c)::value;
        const unsigned short* ai = img + buf * GQ_BUF;
#pragma unroll
        for (int p = 2; p >= 0; --p) {
#pragma unroll
            for (int a = 0; a < 2; ++a) fa[set][p][a] = tr_frag(ai + p * GQ_PSZ, frow, acol + 32 * a);
#pragma unroll
            for (int b = 0; b < 2; ++b) fb[set][p][b] = tr_frag(ai + (3 + p) * GQ_PSZ, frow, bcol + 32 * b);
        }
    };

    // prologue: slice 0 -> stage 0 -> fragment set 0, slice 1 -> registers
    xload(0, rbeg); xload(1, rbeg); aload(rbeg);
    xwrite(0, 0); xwrite(1, 0); awrite_v(0); awrite_u(0, jt == 0);
    xload(0, rbeg + GB_BKR); xload(1, rbeg + GB_BKR); aload(rbeg + GB_BKR);
    __syncthreads();
    frags(std::integral_constant<int, 0>{}, 0);

    // cross terms (p, q) of dPre piece p and x piece q, p + q <= 2, smallest first (the forward's order)
    auto slice = [&](int sl, auto set_c) {
        constexpr int set = decltype(set_c)::value;      // fragment set = stage of slice sl
        constexpr int TP[6] = {0, 1, 2, 0, 1, 0}, TQ[6] = {2, 1, 0, 1, 0, 0};
        const int row2 = rbeg + (sl + 2) * GB_BKR;
        const bool pub = ((sl + 1) % NJ) == jt;          // the slice being staged now is sl + 1
        auto mfma = [&](int t, int g) {
            const int a = g >> 1, b = g & 1;
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gp_bf16x8, fa[set][TP[t]][a]),
                                                                __builtin_bit_cast(gp_bf16x8, fb[set][TQ[t]][b]), acc[a][b], 0, 0, 0);
        };
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                mfma(t, g);
                __builtin_amdgcn_sched_barrier(0);
                switch (4 * t + g) {                     // seven staging parts behind the first MFMAs
                    case 0: xwrite(0, set ^ 1); break;
                    case 1: xload(0, row2); break;
                    case 2: xwrite(1, set ^ 1); break;
                    case 3: xload(1, row2); break;
                    case 4: awrite_v(set ^ 1); break;
                    case 5: awrite_u(set ^ 1, pub); break;
                    case 6: aload(row2); break;
                    default: break;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();                                 // stage set ^ 1 holds slice sl + 1; every wave has read stage `set`
        if (sl + 1 < nloop) frags(std::integral_constant<int, set ^ 1>{}, set ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 3; t < 6; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) mfma(t, g);
    };
    int sl = 0;
    for (; sl + 1 < nloop; sl += 2) {
        slice(sl, std::integral_constant<int, 0>{});
        slice(sl + 1, std::integral_constant<int, 1>{});
    }
    if (sl < nloop) slice(sl, std::integral_constant<int, 0>{});
    __syncthreads();                                     // the stages are dead from here on

    dw2_store_tile(smem_all, acc, part, s, m, L, j0, grp, wave, lane);
    dw2_publish_sums(smem_all, pbias, s, NJ, jt, m, arow, ad4, acc_bv, acc_bu, acc_w, acc_ds);
}

// ================================================================================ host side
// The weight-gradient part of the route plan (gate_route_plan, gate_fwd.hip): it depends on the shape alone (L % 128 == 0).
// KG = 2 (two K groups per 512-thread workgroup, one workgroup per CU) once a row chunk is at least 512 rows deep; with fp32
// x and offsets within 32 bits that is the low-VALU kernel (k_gate_bwd_dw2; bf16 x stays on k_gate_bwd_dw<true, 2>)
GateDwPlan gate_dw_plan(int R, int L, int ncu) {
    const int NJ = L / 128;
    GateDwPlan d{};
    int kg = 1;
    if (ncu / (3 * NJ) >= 1 && R / (ncu / (3 * NJ)) >= 512) kg = 2;
    d.dw = kg == 2 ? MIL_ROUTE_DW_KG2 : MIL_ROUTE_DW_KG1;
    if (kg == 2 && (long long)R * L < (1ll << 29)) d.dw = MIL_ROUTE_DW2;
    int smax = (2 * ncu / kg) / (3 * NJ);
    if (smax < 1) smax = 1;
    d.kc = ((R + smax - 1) / smax + GB_BKR - 1) / GB_BKR * GB_BKR;
    if (d.kc < GB_BKR) d.kc = GB_BKR;
    d.S = (R + d.kc - 1) / d.kc;
    return d;
}

template <bool XB16>
static void launch_gate_bwd_dw(const void* x, const float* gates, const float* ds, const float* w, float* part, float* pbias,
                               int R, int L, int kc, int NJ, int S, int kg, const uint32_t* xbits, hipStream_t st,
                               const int32_t* rows_dev = nullptr) {
    const dim3 grid(S * 3 * NJ);
    if (kg == 2) {
        if (xbits) hipLaunchKernelGGL((k_gate_bwd_dw<XB16, 2, true>), grid, dim3(512), 0, st, x, gates, ds, w, part, pbias, R, L, kc, NJ, xbits, rows_dev);
        else hipLaunchKernelGGL((k_gate_bwd_dw<XB16, 2, false>), grid, dim3(512), 0, st, x, gates, ds, w, part, pbias, R, L, kc, NJ, xbits, rows_dev);
    } else {
        if (xbits) hipLaunchKernelGGL((k_gate_bwd_dw<XB16, 1, true>), grid, dim3(256), 0, st, x, gates, ds, w, part, pbias, R, L, kc, NJ, xbits, rows_dev);
        else hipLaunchKernelGGL((k_gate_bwd_dw<XB16, 1, false>), grid, dim3(256), 0, st, x, gates, ds, w, part, pbias, R, L, kc, NJ, xbits, rows_dev);
    }
}

static inline size_t gate_bwd_ws_floats(int S, int L) { return (size_t)S * GF_NG * L + (size_t)S * (L / 128) * 4 * 192; }

extern "C" size_t mil_gate_bwd_workspace_floats(int R, int L) {
    if (R <= 0 || L <= 0 || (L % 128) != 0) return 0;
    return gate_bwd_ws_floats(gate_dw_plan(R, L, MIL_NUM_CU).S, L);
}

// The K loop of the dw2 route: the split-bf16 kernel (k_gate_bwd_dw2_pieces) unless MIL_DW_PIECES=0 asks for the f32-MFMA
// one.  Read per call (under a hipGraph: at capture), so A/B runs and tests toggle it inside one process; the route plan,
// the workspace and the fold are the same for both.
static inline bool dw_pieces_on() {
    const char* e = getenv("MIL_DW_PIECES");
    return e == nullptr || atoi(e) != 0;
}

// The two launches of mil_gate_bwd_params as separate entry points (bench.py times the MFMA kernel alone).
static int gate_bwd_partials_impl(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                  int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                  const int32_t* rows_dev, void* stream) {
    if (!x || !gates || !ds || !w || !workspace) return MIL_EINVAL;
    if (D != MIL_GATE_D || L <= 0 || (L % 128) != 0 || R <= 0) return MIL_EINVAL;
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);
    const int S = p.S, kc = p.kc, NJ = L / 128;
    if (workspace_floats < gate_bwd_ws_floats(S, L)) return MIL_ENOSPC;
    float* pb = workspace + (size_t)S * GF_NG * L;
    if (p.dw == MIL_ROUTE_DW2 && dw_pieces_on()) {
        if (xbits)
            hipLaunchKernelGGL(k_gate_bwd_dw2_pieces<true>, dim3(S * 3 * NJ), dim3(512), 0, (hipStream_t)stream, x, gates, ds, w, workspace, pb,
                               R, L, kc, NJ, xbits, rows_dev);
        else
            hipLaunchKernelGGL(k_gate_bwd_dw2_pieces<false>, dim3(S * 3 * NJ), dim3(512), 0, (hipStream_t)stream, x, gates, ds, w, workspace, pb,
                               R, L, kc, NJ, xbits, rows_dev);
        MIL_CHECK_LAUNCH();
        return MIL_OK;
    }
    if (p.dw == MIL_ROUTE_DW2) {
        if (xbits)
            hipLaunchKernelGGL(k_gate_bwd_dw2<true>, dim3(S * 3 * NJ), dim3(512), 0, (hipStream_t)stream, x, gates, ds, w, workspace, pb,
                               R, L, kc, NJ, xbits, rows_dev);
        else
            hipLaunchKernelGGL(k_gate_bwd_dw2<false>, dim3(S * 3 * NJ), dim3(512), 0, (hipStream_t)stream, x, gates, ds, w, workspace, pb,
                               R, L, kc, NJ, xbits, rows_dev);
        MIL_CHECK_LAUNCH();
        return MIL_OK;
    }
    launch_gate_bwd_dw<false>((const void*)x, gates, ds, w, workspace, pb, R, L, kc, NJ, S, p.dw == MIL_ROUTE_DW_KG2 ? 2 : 1, xbits,
                              (hipStream_t)stream, rows_dev);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_gate_bwd_partials(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                     int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                     void* stream) {
    return gate_bwd_partials_impl(x, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, nullptr, stream);
}
// rows_dev: device int32 holding the TRUE number of rows (<= R).  R then is the bucket the launch is sized for (grid,
// split-K plan, workspace); rows beyond the true count contribute nothing.  One launch configuration - one captured
// graph - serves every batch of the bucket.
extern "C" int mil_gate_bwd_partials_rows(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                          int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                          const int32_t* rows_dev, void* stream) {
    return gate_bwd_partials_impl(x, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, rows_dev, stream);
}

// The fold of the workspace gate_bwd_partials_impl filled for (R, L): the same plan gives its layout
static int gate_bwd_fold(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu, float* dw, float* db,
                         int accumulate, float wscale, void* stream, const HeadBwdArgs* head = nullptr,
                         const AdamFuse* ad = nullptr, uint16_t* Wp = nullptr) {
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);
    return launch_gate_bwd_reduce(workspace, workspace + (size_t)p.S * GF_NG * L, p.S, p.dw == MIL_ROUTE_DW2 ? p.S * (L / 128) : p.S,
                                  L, dWv, dbv, dWu, dbu, dw, db, accumulate, wscale, (hipStream_t)stream, head, ad, nullptr,
                                  nullptr, Wp);
}

extern "C" int mil_gate_bwd_reduce(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu,
                                   float* dw, float* db, int accumulate, float xscale, void* stream) {
    if (!workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0) return MIL_EINVAL;
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, stream);
}

extern "C" int mil_gate_bwd_params_head(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                        int D, float* workspace, size_t workspace_floats, float* dWv, float* dbv,
                                        float* dWu, float* dbu, float* dw, float* db, int accumulate, const float* dz,
                                        const float* M, float* dWf, float* dbf, int B, int C, const float* loss_bag,
                                        float* loss_out, const uint32_t* xbits, float xscale, void* stream) {
    if (!dWv || !dbv || !dWu || !dbu || !dw || !db || !dz || !M || !dWf || !dbf) return MIL_EINVAL;
    if (B <= 0 || C <= 0 || C > 32 || (loss_bag && !loss_out)) return MIL_EINVAL;
    const int rc = mil_gate_bwd_partials(x, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, stream);
    if (rc != MIL_OK) return rc;
    const HeadBwdArgs head{dz, M, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate};
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xbits ? xscale : 1.0f, stream, &head);
}

// The reduce launch of mil_gate_bwd_params_head alone (split-K fold + the head's parameter gradients as appended
// workgroups), for a caller that issued mil_gate_bwd_partials itself (csrc/step.hip).
extern "C" int mil_gate_bwd_reduce_head(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu,
                                        float* dw, float* db, int accumulate, float xscale, const float* dz, const float* M,
                                        float* dWf, float* dbf, int B, int C, const float* loss_bag, float* loss_out,
                                        void* stream) {
    if (!workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db || !dz || !M || !dWf || !dbf) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0 || B <= 0 || C <= 0 || C > 32 || (loss_bag && !loss_out)) return MIL_EINVAL;
    const HeadBwdArgs head{dz, M, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate};
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, stream, &head);
}

// mil_gate_bwd_reduce_head with Adam applied by the threads that produce the final gradients (world size 1: nothing sits
// between the gradient and the update): param_flat / exp_avg / exp_avg_sq are indexed like grad_flat, in which dWv .. dbf all
// lie; `step` >= 1 is the update's number (bias corrections on the host).  Saves the Adam launch of the image-only step.
extern "C" int mil_gate_bwd_reduce_head_adam(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu,
                                             float* dbu, float* dw, float* db, int accumulate, float xscale, const float* dz,
                                             const float* M, float* dWf, float* dbf, int B, int C, const float* loss_bag,
                                             float* loss_out, float* param_flat, const float* grad_flat, size_t n_param,
                                             float* exp_avg, float* exp_avg_sq, int step, float lr, float beta1, float beta2,
                                             float eps, float weight_decay, float grad_scale, void* stream) {
    return gate_bwd_reduce_head_adam_impl(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, dz, M, dWf, dbf, B, C,
                                          loss_bag, loss_out, param_flat, grad_flat, n_param, exp_avg, exp_avg_sq, step, nullptr,
                                          lr, nullptr, beta1, beta2, eps, weight_decay, grad_scale, stream);
}

int gate_bwd_reduce_head_adam_impl(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu,
                                   float* dw, float* db, int accumulate, float xscale, const float* dz, const float* M,
                                   float* dWf, float* dbf, int B, int C, const float* loss_bag, float* loss_out,
                                   float* param_flat, const float* grad_flat, size_t n_param, float* exp_avg,
                                   float* exp_avg_sq, int step, const int* step_dev, float lr, const float* lr_dev, float beta1,
                                   float beta2, float eps, float weight_decay, float grad_scale, void* stream, int* done,
                                   uint16_t* Wp) {
    if (!workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db || !dz || !M || !dWf || !dbf) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0 || B <= 0 || C <= 0 || C > 32 || (loss_bag && !loss_out)) return MIL_EINVAL;
    const HeadBwdArgs head{dz, M, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate};
    AdamFuse ad{};
    const int rc = gate_adam_fuse(dWv, dbv, dWu, dbu, dw, db, head, param_flat, grad_flat, n_param, exp_avg, exp_avg_sq, step, step_dev,
                                  lr, lr_dev, beta1, beta2, eps, weight_decay, grad_scale, done, &ad);
    if (rc != MIL_OK) return rc;
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, stream, &head, &ad, Wp);
}

extern "C" int mil_gate_bwd_params(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                   int D, float* workspace, size_t workspace_floats, float* dWv, float* dbv,
                                   float* dWu, float* dbu, float* dw, float* db, int accumulate, const uint32_t* xbits,
                                   float xscale, void* stream) {
    if (!dWv || !dbv || !dWu || !dbu || !dw || !db) return MIL_EINVAL;
    const int rc = mil_gate_bwd_partials(x, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, stream);
    if (rc != MIL_OK) return rc;
    return mil_gate_bwd_reduce(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xbits ? xscale : 1.0f, stream);
}

extern "C" int mil_gate_bwd_params_x16(const uint16_t* x, const float* gates, const float* ds, const float* w, int R,
                                       int L, int D, float* workspace, size_t workspace_floats, float* dWv, float* dbv,
                                       float* dWu, float* dbu, float* dw, float* db, int accumulate, const uint32_t* xbits,
                                       float xscale, void* stream) {
    if (!x || !gates || !ds || !w || !workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db) return MIL_EINVAL;
    if (D != MIL_GATE_D || L <= 0 || (L % 128) != 0 || R <= 0) return MIL_EINVAL;
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);          // bf16 x: k_gate_bwd_dw<true, KG> where fp32 x would take k_gate_bwd_dw2
    const int S = p.S;
    if (workspace_floats < gate_bwd_ws_floats(S, L)) return MIL_ENOSPC;
    float* part = workspace;
    float* pbias = workspace + (size_t)S * GF_NG * L;
    hipStream_t st = (hipStream_t)stream;
    launch_gate_bwd_dw<true>((const void*)x, gates, ds, w, part, pbias, R, L, p.kc, L / 128, S, p.dw == MIL_ROUTE_DW_KG1 ? 1 : 2, xbits,
                             st);
    MIL_CHECK_LAUNCH();
    return launch_gate_bwd_reduce(part, pbias, S, S, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xbits ? xscale : 1.0f, st);
}
