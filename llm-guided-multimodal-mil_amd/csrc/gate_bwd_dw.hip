// K1 backward: the gate weight gradient of the gated-attention MIL pooling (ABMIL) for gfx950.
//
// Reference arithmetic: torch autograd of model/dim1/ABMIL.py:47-56.  The transpose-product dPre^T . x is a dense
// contraction over the rows: v_mfma_f32_32x32x2_f32 (k_gate_bwd_dw, k_gate_bwd_dw2) or the split-bf16 loop
// (k_gate_bwd_dw2_pieces); the split-K fold is k_gate_bwd_reduce (gate_reduce.h).  Forward and route plan: gate_fwd.hip.
// The three kernels are built from one set of parts (below): workgroup coordinates and K-group rows (dw_coord, dw_rows),
// the keep mask of a staged x chunk (dw_keep4), the dPre formula and the bias / w / b sums (DwPre, DwSums), the buffer-resource
// loaders of the dw2 kernels (DwSrdSource), the pinned f32 k-steps of a slice (dw_slice_f32) and the epilogue (dw_store_tile,
// dw_publish_sums).  The host side names every instantiation in two tables (DW_KERNELS, DW2_KERNELS; gate_dw_launch picks).
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
#define DW_GRP_FLOATS (2 * 2 * GB_BKR * 128)      /* the f32 stages of one K group: [2][32][128] dPre, [2][32][128] x (64 KiB) */
typedef unsigned short gb_u16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- parts
// Output tile of the workgroup: column tile jt (j0 = 128 jt), gate block m, row chunk s.  The 3*NJ workgroups of one row
// chunk re-read the same x / gate rows, so they take consecutive slots of ONE XCD (xcd_order).  Handed to the parts by value.
struct DwCoord {
    int jt, m, s, j0;
};
__device__ __forceinline__ DwCoord dw_coord(int NJ) {
    const int bid = xcd_order(blockIdx.x, gridDim.x);
    const int jt = bid % NJ;
    return {jt, (bid / NJ) % 3, bid / (3 * NJ), jt * 128};
}

// Bucketed batches: R is the bucket the launch is sized for, the true row count lives on the device (rows_dev, or NULL)
__device__ __forceinline__ int dw_true_rows(int R, const int32_t* __restrict__ rows_dev) {
    return rows_dev != nullptr ? min(R, __builtin_amdgcn_readfirstlane(rows_dev[0])) : R;
}

// Row chunk s of the workgroup, then K group grp's part of it (whole slices to group 0 first).  The slice loop runs nloop times
// for every group (common barriers); nslice counts the group's own slices (the clamped loaders of k_gate_bwd_dw need it).
struct DwRows {
    int rbeg, rend, nloop, nslice;
};
template <int KG>
__device__ __forceinline__ DwRows dw_rows(int s, int KC, int R, int grp) {
    const int cbeg = min(s * KC, R), cend = min(R, cbeg + KC);
    const int half = KG == 1 ? cend - cbeg : ((cend - cbeg + 2 * GB_BKR - 1) / (2 * GB_BKR)) * GB_BKR;
    const int rbeg = min(cend, cbeg + grp * half), rend = KG == 1 ? cend : min(cend, rbeg + half);
    return {rbeg, rend, (min(half, cend - cbeg) + GB_BKR - 1) / GB_BKR, (rend - rbeg + GB_BKR - 1) / GB_BKR};
}

// Train mode: the keep bits (the forward's mask, csrc/dropout.hip) of four staged x columns.  word = the 32 keep bits the
// columns lie in, chunk = their 16-byte chunk index within the row.
__device__ __forceinline__ f32x4 dw_keep4(f32x4 v, unsigned word, int chunk) {
    const unsigned mm = word >> (4 * (chunk & 7));
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = keep_if(v[e], mm, e);
    return v;
}

// dPreV = ds w U (1 - V^2) = a - (a V) V and dPreU = ds w V U (1 - U) = t - t U with a = ds w U, t = a V: four VALU per
// (V, U) pair instead of seven.  ds_w = ds w as the kernel formed it (the clamped kernel masks ds first).
struct DwPre {
    static __device__ __forceinline__ f32x4 v(const f32x4 ds_w, const f32x4 V, const f32x4 U, f32x4& t) {
        const f32x4 a = ds_w * U;
        t = a * V;
        return a - t * V;
    }
    static __device__ __forceinline__ f32x4 u(const f32x4 t, const f32x4 U) { return t - t * U; }
};

// The bias / w / b sums of a thread's rows: dbv, dbu (float4 column ad4 of block m), dw and, in the ad4 == 0 threads, db.
struct DwSums {
    f32x4 bv = {0, 0, 0, 0}, bu = {0, 0, 0, 0}, w = {0, 0, 0, 0};
    float ds = 0.f;
    // k_gate_bwd_dw sums every slice: dPreV as it was staged, and with dPreU the w and b terms (dsv = the masked ds)
    __device__ __forceinline__ void add_v(const f32x4 pv) { bv += pv; }
    __device__ __forceinline__ void add_u(const f32x4 pu, float dsv, const f32x4 V, const f32x4 U, int ad4) {
        bu += pu;
        w += (dsv * V) * U;
        if (ad4 == 0) ds += dsv;
    }
    // the dw2 kernels sum every NJ-th slice only, behind a scalar branch in the dPreU part: dPreV is formed again there
    // (3 VALU per element), NOT carried over from the dPreV part
    __device__ __forceinline__ void add_pub(float dsv, const f32x4 w4, const f32x4 V, const f32x4 U, const f32x4 t, const f32x4 pu,
                                            int ad4) {
        bv += (dsv * w4) * U - t * V;
        add_u(pu, dsv, V, U, ad4);
    }
};

// The global operands of the dw2 kernels, through buffer resources whose base / size live in SGPRs and advance by scalar ALU:
// the per-lane byte offsets are loop invariants, and a row at or beyond `rend` is out of range, so the hardware range check
// returns ZERO for it (no clamps, no validity masks: a zero ds row contributes nothing).  Thread t stages NX chunks of x
// (rows (t >> 5) + (32 / NX) i, 16-byte chunk t & 31 of the 128-column tile) and NA float4 pairs of gates (rows (t >> 4) +
// (32 / NA) i, d = 64m + 4 (t & 15)) per 32-row slice: 4 and 2 with 256 threads per K group, 2 and 1 with 512.
template <bool DROP, int NX, int NA>
struct DwSrdSource {
    const float *x, *gates, *ds;
    const uint32_t* xbits;
    int L, LW, rend;
    int vx[NX], vm[NX], vg[NA], vd[NA];
    u32x4_t rx[NX], rv[NA], ru[NA];       // the staged slice: x chunks, V and U, ds and (train mode) the keep words
    unsigned rm[NX];
    float rds[NA];
    __device__ __forceinline__ DwSrdSource(const float* x_, const float* gates_, const float* ds_, const uint32_t* xbits_, int L_,
                                           int rend_, int t, const DwCoord c)
        : x(x_), gates(gates_), ds(ds_), xbits(xbits_), L(L_), LW(L_ >> 5), rend(rend_) {
        const int xrow = t >> 5, xc4 = t & 31, arow = t >> 4, ad4 = t & 15;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            vx[i] = ((xrow + (32 / NX) * i) * L + c.j0 + 4 * xc4) * 4;
            vm[i] = ((xrow + (32 / NX) * i) * LW + ((c.j0 + 4 * xc4) >> 5)) * 4;
            rm[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            vg[i] = ((arow + (32 / NA) * i) * GF_NG + 64 * c.m + 4 * ad4) * 4;
            vd[i] = (arow + (32 / NA) * i) * 4;
        }
    }
    // scalar: the resource of `left` rows from row0 of an operand with `stride` 4-byte words per row.  left = the rows up to
    // rend, formed once per xload / aload and not in here: with the max() inside, the scalar instructions of the pieces kernel's
    // K loop come out in another order (docs/lab_notes.md)
    template <class T>
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t srd(const T* base, int row0, int left, int stride) const {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(base + (size_t)row0 * stride), 0, left * stride * 4, MIL_SRD_FLAGS);
    }
    __device__ __forceinline__ void xload(int i, int row0) {
        const int left = max(rend - row0, 0);
        rx[i] = __builtin_amdgcn_raw_buffer_load_b128(srd(x, row0, left, L), vx[i], 0, 0);
        if (DROP) rm[i] = __builtin_amdgcn_raw_buffer_load_b32(srd(xbits, row0, left, LW), vm[i], 0, 0);
    }
    __device__ __forceinline__ void aload(int i, int row0) {
        const int left = max(rend - row0, 0);
        const __amdgpu_buffer_rsrc_t g = srd(gates, row0, left, GF_NG);
        rv[i] = __builtin_amdgcn_raw_buffer_load_b128(g, vg[i], 0, 0);
        ru[i] = __builtin_amdgcn_raw_buffer_load_b128(g, vg[i] + 192 * 4, 0, 0);
        rds[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd(ds, row0, left, 1), vd[i], 0, 0));
    }
    __device__ __forceinline__ f32x4 xval(int i) const { return __builtin_bit_cast(f32x4, rx[i]); }
    __device__ __forceinline__ f32x4 V(int i) const { return __builtin_bit_cast(f32x4, rv[i]); }
    __device__ __forceinline__ f32x4 U(int i) const { return __builtin_bit_cast(f32x4, ru[i]); }
};

__device__ __forceinline__ void dw_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
}

// The 16 k-steps of one 32-row slice on v_mfma_f32_32x32x2_f32, with the staging of the slices behind it in their shadow.
// Issue order inside a k-step.  The two waves of a SIMD (w and w + 4) share its matrix pipe and the older one wins every
// arbitration: measured with in-kernel cycle stamps (docs/lab_notes.md), waves 0-3 spent 29 % of the loop parked at the
// slice barrier while waves 4-7, starved until then, finished the slice ALONE.  A wave on its own only keeps the pipe
// busy if its non-matrix instructions sit in the shadow of its own MFMAs, so the k-step is laid out as
//     MFMA . fragment reads . MFMA . staging part a . MFMA . staging part b . MFMA
// (one v_mfma_f32_32x32x2_f32 occupies the pipe for 64 cycles; a part is a handful of VALU / one LDS write / one or
// two global loads), each boundary pinned with sched_barrier: hipcc otherwise gathers the staging in front of a
// block of four MFMAs, behind which the wave sits blocked for 3 x 64 cycles with nothing else to issue.
// Timetable: part a writes the LDS image of slice sl + 1 from the registers (x chunk ks - 1 at ks 1..4, dPreV / dPreU of gate
// row i at ks 5 + 2i / 6 + 2i), part b reloads the registers with slice sl + 2 (x chunk ks - 1 at ks 1..4, gate row i at
// ks 6 + 2i).  stage(what, i) is the kernel's staging; ap / bp: the lane's operand words of k-step 0, the second 32-wide
// block STRIDE words on (32: blocks in order, 64: blocks stored {0, 2, 1, 3}, one ds_read2st64_b32 per operand).
enum DwStage { DW_XWRITE, DW_XLOAD, DW_AWRITE_V, DW_AWRITE_U, DW_ALOAD };
template <int STRIDE, class Stage>
__device__ __forceinline__ void dw_slice_f32(const float* ap, const float* bp, f32x16 (&acc)[2][2], Stage&& stage) {
    float fa[2][2], fb[2][2];
    fa[0][0] = ap[0]; fa[0][1] = ap[STRIDE]; fb[0][0] = bp[0]; fb[0][1] = bp[STRIDE];
#pragma unroll
    for (int ks = 0; ks < GB_BKR / 2; ++ks) {
        const int q = ks & 1;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][0], acc[0][0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 1 < GB_BKR / 2) {
            fa[q ^ 1][0] = ap[(ks + 1) * 256]; fa[q ^ 1][1] = ap[(ks + 1) * 256 + STRIDE];
            fb[q ^ 1][0] = bp[(ks + 1) * 256]; fb[q ^ 1][1] = bp[(ks + 1) * 256 + STRIDE];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][0], fb[q][1], acc[0][1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ks >= 1 && ks <= 4) stage(DW_XWRITE, ks - 1);
        if (ks == 5 || ks == 7) stage(DW_AWRITE_V, (ks - 5) >> 1);
        if (ks == 6 || ks == 8) stage(DW_AWRITE_U, (ks - 6) >> 1);
        __builtin_amdgcn_sched_barrier(0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][0], acc[1][0], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ks >= 1 && ks <= 4) stage(DW_XLOAD, ks - 1);
        if (ks == 6 || ks == 8) stage(DW_ALOAD, (ks - 6) >> 1);
        __builtin_amdgcn_sched_barrier(0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][1], fb[q][1], acc[1][1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Epilogue, first half: partial tile -> part[s][128m + 64wi + row][j0 + 64wj + col].  The accumulators hold a column per lane
// (16 rows each); going through LDS turns 64 four-byte stores per lane into sixteen-byte ones: every wave writes its 64 x 64
// tile row-major into its own 16 KB of its group's (now dead) staging area (stride 64 is conflict-free both ways).
// KG = 2: both K groups do that, then the two waves that own the same tile (one per group) each fold and store HALF of its
// rows - one LDS round trip and all eight waves storing, instead of fold -> transpose -> store by four.
// KG = 1: no barrier, the same wave writes and reads (ordered by lgkmcnt).
// LANE_FIRST: two spellings of the same 64 store addresses, each kernel keeping the code it had.  With the lane's part
// (row 4h, column r) in the base pointer the stores are one base + immediates, paired into ds_write2 at KG = 2
// (k_gate_bwd_dw); with it in the index the dw2 kernels get their 64 single stores and 16 v_or.
template <int KG, bool LANE_FIRST>
__device__ __forceinline__ void dw_store_tile(float* smem_all, const f32x16 (&acc)[2][2], float* __restrict__ part, const DwCoord c,
                                              int L, int grp, int wave, int lane) {
    const int wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    float* tw = smem_all + grp * DW_GRP_FLOATS + wave * (64 * 64) + (LANE_FIRST ? mfma32_row(0, h) * 64 + r : 0);
    const int hi = LANE_FIRST ? 0 : h, ri = LANE_FIRST ? 0 : r;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) tw[(32 * a + mfma32_row(i, hi)) * 64 + 32 * b + ri] = acc[a][b][i];
    if (KG == 2) __syncthreads();
    float* pt = part + ((size_t)c.s * GF_NG + 128 * c.m + 64 * wi) * L + c.j0 + 64 * wj;
    const int c4 = lane & 15, rr = lane >> 4;         // 16 float4 columns x 4 rows per pass
    const float* t0 = smem_all + wave * (64 * 64);
    const float* t1 = smem_all + DW_GRP_FLOATS + wave * (64 * 64);
    constexpr int NP = 16 / KG;
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
        const int row = 4 * (pass + NP * grp) + rr;
        f32x4 v = *reinterpret_cast<const f32x4*>(t0 + row * 64 + 4 * c4);
        if (KG == 2) v += *reinterpret_cast<const f32x4*>(t1 + row * 64 + 4 * c4);
        *reinterpret_cast<f32x4*>(pt + (size_t)row * L + 4 * c4) = v;
    }
}
// Epilogue, second half: the workgroup's bias / w / b sums -> pb[4][192] (block m's 64 columns of dbv, dbu, dw; db from the
// m == 0 workgroup), folded over the 16 KG row groups of the dPre staging map.  arow_all (0 .. 16 KG - 1), ad4: the thread's
// row group and float4 column in that map.
template <int KG>
__device__ __forceinline__ void dw_publish_sums(float* smem_all, float* __restrict__ pb, int m, int arow_all, int ad4,
                                                const DwSums sums) {
    float* redf = smem_all;   // [16 KG row groups][3][64]
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        redf[(arow_all * 3 + 0) * 64 + 4 * ad4 + e] = sums.bv[e];
        redf[(arow_all * 3 + 1) * 64 + 4 * ad4 + e] = sums.bu[e];
        redf[(arow_all * 3 + 2) * 64 + 4 * ad4 + e] = sums.w[e];
    }
    __syncthreads();
    if (threadIdx.x < 192) {
        const int which = threadIdx.x / 64, d = threadIdx.x % 64;
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 16 * KG; ++g) v += redf[(g * 3 + which) * 64 + d];
        pb[which * 192 + 64 * m + d] = v;
    }
    if (m == 0) {
        __syncthreads();
        redf[threadIdx.x] = sums.ds;
        __syncthreads();
        if (threadIdx.x == 0) {
            float v = 0.f;
            for (int g = 0; g < 256 * KG; g += 16) v += redf[g];
            pb[3 * 192] = v;
        }
    }
}

// ---------------------------------------------------------------- k_gate_bwd_dw: clamped loaders, bf16 or fp32 x, KG = 1 or 2
// XB16: x is stored as bf16 and widened to fp32 while it is staged (config-5 path; the product stays fp32 MFMA).
// KG: K groups per workgroup.  KG = 2 (tall inputs): 512 threads, the two halves of the workgroup run the same pipeline
// on the two halves of the row chunk (own LDS stages, common barriers) and fold their accumulators through LDS before the
// store, so a launch needs half as many row chunks for the same number of resident waves - half the partial tiles to
// write here and to read in k_gate_bwd_reduce.
// Only the j-tile-0 workgroups publish the bias / w / b sums: pbias[s][4][192].
template <bool XB16, int KG, bool DROP>
__global__ __launch_bounds__(256 * KG) void k_gate_bwd_dw(const void* __restrict__ xv, const float* __restrict__ gates,
                                                     const float* __restrict__ ds, const float* __restrict__ wvec,
                                                     float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                     int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                     const int32_t* __restrict__ rows_dev) {
    __shared__ __attribute__((aligned(16))) float smem_all[KG * DW_GRP_FLOATS];
    R = dw_true_rows(R, rows_dev);
    const int grp = KG == 1 ? 0 : (int)(threadIdx.x >> 8);
    float* smem = smem_all + grp * DW_GRP_FLOATS;      // this K group's stages
    float* ab = smem;                         // [2][32][128] dPre
    float* xb = smem + 2 * GB_BKR * 128;      // [2][32][128] x
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const DwCoord c = dw_coord(NJ);
    // iterations past a group's own slices multiply dead copies (ds = 0)
    const DwRows rw = dw_rows<KG>(c.s, KC, R, grp);
    const int rbeg = rw.rbeg, rend = rw.rend, nslice = rw.nslice;

    const float* x = static_cast<const float*>(xv);
    const unsigned short* xh = static_cast<const unsigned short*>(xv);
    // staging maps
    const int xrow = tid >> 5, xc4 = tid & 31;    // x: rows xrow + 8i (i < 4), 16-byte chunk xc4
    const int hrow = tid >> 4, hc8 = tid & 15;    // bf16 x: rows hrow + 16i (i < 2), 16-byte chunk (8 columns) hc8
    gb_u16x8 rh[2];
    const int arow = tid >> 4, ad4 = tid & 15;    // gates: rows arow + 16i (i < 2), d = 64m + 4*ad4
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * c.m + 4 * ad4);
    f32x4 rx[4], rv[2], ru[2];
    unsigned rm[4] = {0, 0, 0, 0};   // train mode: keep bits of the staged x chunks
    float rds[2], rmask[2];      // raw ds value and its validity mask (applied at use, never at load)
    DwSums sums;

    // Branch-free staging pieces (rows past the chunk end are clamped to its last row and get ds = 0, so they
    // add nothing): the loop body is one basic block and every piece sits between two MFMA groups.
    const int LW = L >> 5;
    auto xload = [&](int i, int rs) {
        if (XB16) {
            if (i < 2) {
                const int gr = max(min(rs + hrow + 16 * i, rend - 1), 0);
                rh[i] = *reinterpret_cast<const gb_u16x8*>(xh + (size_t)gr * L + c.j0 + 8 * hc8);
                if (DROP) rm[i] = xbits[(size_t)gr * LW + ((c.j0 + 8 * hc8) >> 5)];
            }
        } else {
            const int gr = max(min(rs + xrow + 8 * i, rend - 1), 0);
            rx[i] = *reinterpret_cast<const f32x4*>(x + (size_t)gr * L + c.j0 + 4 * xc4);
            if (DROP) rm[i] = xbits[(size_t)gr * LW + ((c.j0 + 4 * xc4) >> 5)];
        }
    };
    auto xwrite = [&](int i, int buf) {
        if (XB16) {                               // eight columns per chunk: the 8-wide form of dw_keep4
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
            *reinterpret_cast<f32x4*>(xb + (buf * GB_BKR + xrow + 8 * i) * 128 + 4 * xc4) = DROP ? dw_keep4(rx[i], rm[i], xc4) : rx[i];
        }
    };
    auto aload = [&](int i, int rs, bool live) {
        const int gr = rs + arow + 16 * i;
        const int gc = max(min(gr, rend - 1), 0);
        const float* gp = gates + (size_t)gc * GF_NG + 64 * c.m + 4 * ad4;
        rv[i] = *reinterpret_cast<const f32x4*>(gp);
        ru[i] = *reinterpret_cast<const f32x4*>(gp + 192);
        rds[i] = ds[gc];                                  // unconditional load: keeps the body branch-free
        rmask[i] = (live && gr < rend) ? 1.f : 0.f;
    };
    // (The bias / w / b sums stay unconditional: a wave-uniform `jt == 0` branch around them splits the k-step into basic
    // blocks and costs more than the six VALU it saves.)
    f32x4 rt[2];
    auto awrite_v = [&](int i, int buf) {
        const f32x4 pv = DwPre::v((rds[i] * rmask[i]) * w4, rv[i], ru[i], rt[i]);
        *reinterpret_cast<f32x4*>(ab + (buf * GB_BKR + arow + 16 * i) * 128 + 4 * ad4) = pv;
        sums.add_v(pv);
    };
    auto awrite_u = [&](int i, int buf) {
        const f32x4 pu = DwPre::u(rt[i], ru[i]);
        *reinterpret_cast<f32x4*>(ab + (buf * GB_BKR + arow + 16 * i) * 128 + 64 + 4 * ad4) = pu;
        sums.add_u(pu, rds[i] * rmask[i], rv[i], ru[i], ad4);
    };

    f32x16 acc[2][2];
    dw_zero(acc);
    {   // prologue: slice 0 -> LDS buffer 0, slice 1 -> registers
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
    for (int sl = 0; sl < rw.nloop; ++sl) {
        const int buf = sl & 1;
        // registers hold slice sl+1 (or, past this group's last slice, a dead copy with ds forced to 0)
        const bool live2 = sl + 2 < nslice;
        const int rs2 = rbeg + max(min(sl + 2, nslice - 1), 0) * GB_BKR;
        dw_slice_f32<32>(ab + buf * GB_BKR * 128 + h * 128 + 64 * wi + r, xb + buf * GB_BKR * 128 + h * 128 + 64 * wj + r, acc,
                         [&](DwStage what, int i) {
                             if (what == DW_XWRITE) xwrite(i, buf ^ 1);
                             if (what == DW_XLOAD) xload(i, rs2);
                             if (what == DW_AWRITE_V) awrite_v(i, buf ^ 1);
                             if (what == DW_AWRITE_U) awrite_u(i, buf ^ 1);
                             if (what == DW_ALOAD) aload(i, rs2, live2);
                         });
        __syncthreads();
    }

    __syncthreads();                                  // the staging buffers are dead from here on
    dw_store_tile<KG, true>(smem_all, acc, part, c, L, grp, wave, lane);
    if (c.jt == 0) dw_publish_sums<KG>(smem_all, pbias + (size_t)c.s * 4 * 192, c.m, arow + 16 * grp, ad4, sums);
}

// ================================================================================ K1 backward: gate dW, "VALU diet" form
// Same product, tiling, split-K layout, k order and outputs (bit for bit) as k_gate_bwd_dw<false, 2, *>; what changes is
// how little VECTOR-ALU work the main loop carries.  Measured on MI355X (tools/mfma_valu_mix.hip): unlike the bf16 MFMAs,
// v_mfma_f32_32x32x2_f32 does NOT hide VALU instructions issued around it - it runs at the f32 VALU rate and every
// v_fma / v_and between two of them costs 3-5 cycles of matrix time, at one or two waves per SIMD alike (4 fillers per
// MFMA: 64 -> 84 cycles; LDS reads, scalar ALU and s_nop fillers are free).  The first kernel spent ~230 VALU
// instructions per wave and 32-row slice (64 MFMAs) on 64-bit address arithmetic, row clamps, LDS addresses, masks:
// 27 % of the loop.  Here
//   * global operands come through buffer resources (DwSrdSource): no clamps, no validity masks, no address VALU;
//   * both LDS images store their four 32-column blocks in the order {0, 2, 1, 3}, so the two operand values a lane
//     needs per k-step are 64 dwords apart and ONE ds_read2st64_b32 with immediate offsets fetches them (no address
//     VALU; the buffer index is a compile-time constant: the slice loop is unrolled by two);
//   * the bias / w / b sums are spread over the NJ column-tile workgroups of a row chunk (slice sl is summed by the
//     workgroup with jt == sl % NJ, scalar branch) instead of being summed by all of them and published by one: every
//     (s, jt) workgroup publishes into pbias[s][jt][4][192].
// What is left is the arithmetic itself: dPre (20 VALU per (V, U) float4 pair) and, in train mode, the keep mask of x.

template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_bwd_dw2(const float* __restrict__ x, const float* __restrict__ gates,
                                                      const float* __restrict__ ds, const float* __restrict__ wvec,
                                                      float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                      int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                      const int32_t* __restrict__ rows_dev) {
    __shared__ __attribute__((aligned(16))) float smem_all[2 * DW_GRP_FLOATS];
    R = dw_true_rows(R, rows_dev);
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    float* smem = smem_all + grp * DW_GRP_FLOATS;      // this K group's stages: [2][32][128] dPre, [2][32][128] x
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const DwCoord c = dw_coord(NJ);
    const DwRows rw = dw_rows<2>(c.s, KC, R, grp);
    const int rbeg = rw.rbeg;

    DwSrdSource<DROP, 4, 2> src(x, gates, ds, xbits, L, rw.rend, tid, c);
    const int xrow = tid >> 5, xc4 = tid & 31, arow = tid >> 4, ad4 = tid & 15;      // the source's staging map
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * c.m + 4 * ad4);
    // LDS positions: 32-column blocks stored in the order {0, 2, 1, 3}
    auto blkpos = [](int col) { return (col & 31) | ((col & 32) << 1) | ((col & 64) >> 1); };
    float* const ab = smem;                       // [2][32][128]
    float* const xb = smem + 2 * GB_BKR * 128;    // [2][32][128]
    float* const xw = xb + xrow * 128 + blkpos(4 * xc4);              // + (buf * 32 + 8 i) * 128
    float* const aw = ab + arow * 128 + blkpos(4 * ad4);              // V block; U block: blkpos(64 + 4 ad4) = + 32
    const float* const ap = ab + h * 128 + 32 * wi + r;               // + buf * 4096 + ks * 256 (+ 64)
    const float* const bp = xb + h * 128 + 32 * wj + r;

    f32x4 rt[2];
    DwSums sums;
    auto xwrite = [&](int i, int buf) {
        *reinterpret_cast<f32x4*>(xw + (buf * GB_BKR + 8 * i) * 128) = DROP ? dw_keep4(src.xval(i), src.rm[i], xc4) : src.xval(i);
    };
    auto awrite_v = [&](int i, int buf) {
        *reinterpret_cast<f32x4*>(aw + (buf * GB_BKR + 16 * i) * 128) = DwPre::v(src.rds[i] * w4, src.V(i), src.U(i), rt[i]);
    };
    auto awrite_u = [&](int i, int buf, bool pub) {
        const f32x4 pu = DwPre::u(rt[i], src.U(i));
        *reinterpret_cast<f32x4*>(aw + (buf * GB_BKR + 16 * i) * 128 + 32) = pu;
        if (pub) sums.add_pub(src.rds[i], w4, src.V(i), src.U(i), rt[i], pu, ad4);      // scalar branch: this slice's sums belong to this workgroup
    };

    f32x16 acc[2][2];
    dw_zero(acc);
    // prologue: slice 0 -> LDS buffer 0, slice 1 -> registers
#pragma unroll
    for (int i = 0; i < 4; ++i) src.xload(i, rbeg);
#pragma unroll
    for (int i = 0; i < 2; ++i) src.aload(i, rbeg);
#pragma unroll
    for (int i = 0; i < 4; ++i) xwrite(i, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) { awrite_v(i, 0); awrite_u(i, 0, c.jt == 0); }
#pragma unroll
    for (int i = 0; i < 4; ++i) src.xload(i, rbeg + GB_BKR);
#pragma unroll
    for (int i = 0; i < 2; ++i) src.aload(i, rbeg + GB_BKR);
    __syncthreads();

    // one slice: between its MFMAs the parts that stage slice sl + 1 and reload slice sl + 2
    auto slice = [&](int sl, auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        const int row2 = rbeg + (sl + 2) * GB_BKR;
        const bool pub = ((sl + 1) % NJ) == c.jt;                   // the slice being written now is sl + 1
        dw_slice_f32<64>(ap + buf * GB_BKR * 128, bp + buf * GB_BKR * 128, acc, [&](DwStage what, int i) {
            if (what == DW_XWRITE) xwrite(i, buf ^ 1);
            if (what == DW_XLOAD) src.xload(i, row2);
            if (what == DW_AWRITE_V) awrite_v(i, buf ^ 1);
            if (what == DW_AWRITE_U) awrite_u(i, buf ^ 1, pub);
            if (what == DW_ALOAD) src.aload(i, row2);
        });
    };
    int sl = 0;
    for (; sl + 1 < rw.nloop; sl += 2) {
        slice(sl, std::integral_constant<int, 0>{});
        __syncthreads();
        slice(sl + 1, std::integral_constant<int, 1>{});
        __syncthreads();
    }
    if (sl < rw.nloop) {
        slice(sl, std::integral_constant<int, 0>{});
        __syncthreads();
    }

    dw_store_tile<2, false>(smem_all, acc, part, c, L, grp, wave, lane);
    dw_publish_sums<2>(smem_all, pbias + ((size_t)c.s * NJ + c.jt) * 4 * 192, c.m, arow + 16 * grp, ad4, sums);
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
// MP (the deferred pool, gate_route_plan): the m == 0 workgroups also form the chunk's share of the bag embeddings
// M_b = sum_n a_n x~_n from the keep-masked x values their staging threads hold anyway.  a_n (the tail's row weights) and the
// bag of every 32-row slice (aligned layout: tile t = rows 32 t ..) come in as wave-uniform scalars one slice ahead: wave w
// stages rows 2 w, 2 w + 1 (+ 16) of a slice, its lanes 0-31 the even row.  Every staging thread keeps the sum of its rows in
// a private float4 of the 8 KiB the two stages leave free in the LDS image - no registers held across the slice - and stores
// it to mpart[s][bag - first bag of the chunk][staging row][L] whenever the bag changes and at the end of the chunk; the fold
// launch sums chunk by chunk, staging row by staging row (gate_reduce.h).  No atomics, nothing crosses threads in here.
template <bool DROP, bool MP>
__device__ __forceinline__ void gate_bwd_dw2_pieces_body(const float* __restrict__ x, const float* __restrict__ gates,
                                                         const float* __restrict__ ds, const float* __restrict__ wvec,
                                                         float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                         int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                         const int32_t* __restrict__ rows_dev, const float* __restrict__ mp_a,
                                                         const int32_t* __restrict__ mp_tile_map, float* __restrict__ mpart) {
    // 128 KiB: the two stages take 120 KiB, the epilogue's eight 64 x 64 fp32 tiles all of it
    __shared__ __attribute__((aligned(16))) float smem_all[2 * DW_GRP_FLOATS];
    static_assert(2 * GQ_BUF * 2 <= (int)sizeof(smem_all), "stages exceed the LDS image");
    static_assert(2 * GQ_BUF * 2 + MP_ROWS * 128 * 4 <= (int)sizeof(smem_all), "no room for the M sums behind the stages");
    unsigned short* const img = reinterpret_cast<unsigned short*>(smem_all);
    R = dw_true_rows(R, rows_dev);
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));               // which 16 rows of every slice
    const int T = threadIdx.x, tid = T & 255, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int h = lane >> 5;
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;                  // transpose-read address roles
    const DwCoord c = dw_coord(NJ);
    const DwRows rw = dw_rows<1>(c.s, KC, R, 0);         // one K group in the rows: all eight waves walk the whole chunk
    const int rbeg = rw.rbeg;

    DwSrdSource<DROP, 2, 1> src(x, gates, ds, xbits, L, rw.rend, T, c);
    const int xrow = T >> 5, xc4 = T & 31, arow = T >> 4, ad4 = T & 15;      // the source's staging map (512 threads)
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(wvec + 64 * c.m + 4 * ad4);
    unsigned short* const xw = img + 3 * GQ_PSZ + xrow * WB_S + 4 * xc4;     // + buf * GQ_BUF + 16 i * WB_S; piece q: + q * GQ_PSZ
    unsigned short* const aw = img + arow * WB_S + 4 * ad4;                  // V columns 0..63; U: + 64
    const int frow = 16 * grp + 8 * h + tq;
    const int acol = 64 * wi + 16 * tg + 4 * tp;                             // + 32 a
    const int bcol = 64 * wj + 16 * tg + 4 * tp;                             // + 32 b

    f32x4 rt;
    DwSums sums;
    auto put3 = [&](unsigned short* dst, const f32x4 v) {          // four columns of one row: one 8-byte store per piece
        ushort4 o[3];
        gp_split3(v[0], o[0].x, o[1].x, o[2].x);
        gp_split3(v[1], o[0].y, o[1].y, o[2].y);
        gp_split3(v[2], o[0].z, o[1].z, o[2].z);
        gp_split3(v[3], o[0].w, o[1].w, o[2].w);
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<ushort4*>(dst + q * GQ_PSZ) = o[q];
    };
    // MP: scalar state of the M sums
    const bool mpw = MP && c.m == 0;
    const int wave8 = __builtin_amdgcn_readfirstlane(T >> 6);
    f32x4* const macc = reinterpret_cast<f32x4*>(smem_all + GQ_BUF + xrow * 128 + 4 * xc4);       // behind the two stages
    int mp_bag = -1, mp_bag0 = -1;
    float mp_a00 = 0.f, mp_a01 = 0.f, mp_a10 = 0.f, mp_a11 = 0.f;     // a_n of rows 2 w, 2 w + 1, 2 w + 16, 2 w + 17 of the next slice
    int mp_next = -1;                                                 // ... its bag ...
    bool mp_in = false;                                               // ... and whether it lies in the chunk at all
    // The scalars of the slice that starts at row0, one slice ahead of their use.  Nothing here may depend on the loaded values:
    // a select behind the loads would wait for two scalar-memory round trips in the middle of the slice (measured: the kernel
    // 82 -> 103 us).  A slice beyond the chunk reads the values of row 0 (finite; its x rows are zero by the range check of
    // the buffer loads, so the products are zeros) and is kept from the bag bookkeeping by mp_in.
    auto mp_fetch = [&](int row0) {
        mp_in = row0 < rw.rend;
        const int rs = mp_in ? row0 : 0;
        const float* ap = mp_a + rs + 2 * wave8;
        mp_a00 = ap[0]; mp_a01 = ap[1]; mp_a10 = ap[16]; mp_a11 = ap[17];
        mp_next = mp_tile_map[4 * (rs >> 5)];
    };
    auto mp_flush = [&]() {                               // the sums of bag mp_bag -> its slot of this chunk
        // Rare (once per bag and chunk): the store address is formed here from the thread index, behind an empty asm so that
        // it is not hoisted out of the K loop as loop invariants - the kernel sits at its 256 VGPRs and they would be spilled
        int t = T;
        asm volatile("" : "+v"(t));
        const int slot = mp_bag - mp_bag0;
        f32x4* const m4 = reinterpret_cast<f32x4*>(smem_all + GQ_BUF + (t >> 5) * 128 + 4 * (t & 31));
        if ((unsigned)slot < MP_SLOTS)
            *reinterpret_cast<f32x4*>(mpart + (((c.s * MP_SLOTS + slot) * MP_ROWS + (t >> 5)) * L + c.j0 + 4 * (t & 31))) = *m4;
        *m4 = f32x4{0, 0, 0, 0};
    };
    auto mp_turn = [&]() {                                // in front of a slice's first xwrite
        if (mpw && mp_in && mp_next != mp_bag) {
            if (mp_bag >= 0) mp_flush();
            else mp_bag0 = mp_next;
            mp_bag = mp_next;
        }
    };
    auto xwrite = [&](int i, int buf) {
        // MP: ONE read-modify-write of the sums per slice, with the second row: they come out of LDS in FRONT of the split (its
        // ~60 VALU instructions cover the trip) and go back behind it with both rows' terms (the first row's chunk is still in
        // its staging registers: the MP slice reloads them behind both writes, and its keep select is formed again)
        f32x4 msum = {0, 0, 0, 0};
        if (MP && i == 1 && mpw) msum = *macc;
        const f32x4 xv = DROP ? dw_keep4(src.xval(i), src.rm[i], xc4) : src.xval(i);
        put3(xw + buf * GQ_BUF + 16 * i * WB_S, xv);
        if (MP && i == 1 && mpw) {
            const f32x4 x0 = DROP ? dw_keep4(src.xval(0), src.rm[0], xc4) : src.xval(0);
            msum += ((T & 32) ? mp_a01 : mp_a00) * x0;
            *macc = msum + ((T & 32) ? mp_a11 : mp_a10) * xv;
        }
    };
    auto awrite_v = [&](int buf) { put3(aw + buf * GQ_BUF, DwPre::v(src.rds[0] * w4, src.V(0), src.U(0), rt)); };
    auto awrite_u = [&](int buf, bool pub) {
        const f32x4 pu = DwPre::u(rt, src.U(0));
        put3(aw + buf * GQ_BUF + 64, pu);
        if (pub) sums.add_pub(src.rds[0], w4, src.V(0), src.U(0), rt, pu, ad4);      // scalar branch: this slice's sums belong to this workgroup
    };

    f32x16 acc[2][2];
    dw_zero(acc);

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
    src.xload(0, rbeg); src.xload(1, rbeg); src.aload(0, rbeg);
    if (mpw) {
        *macc = f32x4{0, 0, 0, 0};
        mp_fetch(rbeg);
        mp_turn();
    }
    xwrite(0, 0); xwrite(1, 0); awrite_v(0); awrite_u(0, c.jt == 0);
    src.xload(0, rbeg + GB_BKR); src.xload(1, rbeg + GB_BKR); src.aload(0, rbeg + GB_BKR);
    if (mpw) mp_fetch(rbeg + GB_BKR);
    __syncthreads();
    frags(std::integral_constant<int, 0>{}, 0);

    // cross terms (p, q) of dPre piece p and x piece q, p + q <= 2, smallest first (the forward's order)
    auto slice = [&](int sl, auto set_c) {
        constexpr int set = decltype(set_c)::value;      // fragment set = stage of slice sl
        constexpr int TP[6] = {0, 1, 2, 0, 1, 0}, TQ[6] = {2, 1, 0, 1, 0, 0};
        const int row2 = rbeg + (sl + 2) * GB_BKR;
        const bool pub = ((sl + 1) % NJ) == c.jt;        // the slice being staged now is sl + 1
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
                    case 0: mp_turn(); xwrite(0, set ^ 1); break;
                    case 1: if (MP) xwrite(1, set ^ 1); else src.xload(0, row2); break;
                    case 2: if (MP) src.xload(0, row2); else xwrite(1, set ^ 1); break;
                    case 3: src.xload(1, row2); if (mpw) mp_fetch(row2); break;
                    case 4: awrite_v(set ^ 1); break;
                    case 5: awrite_u(set ^ 1, pub); break;
                    case 6: src.aload(0, row2); break;
                    default: break;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();                                 // stage set ^ 1 holds slice sl + 1; every wave has read stage `set`
        if (sl + 1 < rw.nloop) frags(std::integral_constant<int, set ^ 1>{}, set ^ 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 3; t < 6; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) mfma(t, g);
    };
    int sl = 0;
    for (; sl + 1 < rw.nloop; sl += 2) {
        slice(sl, std::integral_constant<int, 0>{});
        slice(sl + 1, std::integral_constant<int, 1>{});
    }
    if (sl < rw.nloop) slice(sl, std::integral_constant<int, 0>{});
    if (mpw && mp_bag >= 0) mp_flush();                  // the chunk's last bag (the slot is the thread's own: no barrier)
    __syncthreads();                                     // the stages are dead from here on

    dw_store_tile<2, false>(smem_all, acc, part, c, L, grp, wave, lane);
    dw_publish_sums<2>(smem_all, pbias + ((size_t)c.s * NJ + c.jt) * 4 * 192, c.m, arow, ad4, sums);
}
template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_bwd_dw2_pieces(const float* __restrict__ x, const float* __restrict__ gates,
                                                             const float* __restrict__ ds, const float* __restrict__ wvec,
                                                             float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                             int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                             const int32_t* __restrict__ rows_dev) {
    gate_bwd_dw2_pieces_body<DROP, false>(x, gates, ds, wvec, part, pbias, R, L, KC, NJ, xbits, rows_dev, nullptr, nullptr, nullptr);
}
// mp_a [R] row weights a_n, mp_tile_map [T][4] of an aligned layout, mpart [S][MP_SLOTS][MP_ROWS][L]
template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_bwd_dw2_pieces_mp(const float* __restrict__ x, const float* __restrict__ gates,
                                                                const float* __restrict__ ds, const float* __restrict__ wvec,
                                                                float* __restrict__ part, float* __restrict__ pbias, int R, int L,
                                                                int KC, int NJ, const uint32_t* __restrict__ xbits,
                                                                const float* __restrict__ mp_a,
                                                                const int32_t* __restrict__ mp_tile_map, float* __restrict__ mpart) {
    gate_bwd_dw2_pieces_body<DROP, true>(x, gates, ds, wvec, part, pbias, R, L, KC, NJ, xbits, nullptr, mp_a, mp_tile_map, mpart);
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

// Every instantiation, by name: 8 + 2 + 2
using DwKernel = decltype(&k_gate_bwd_dw<false, 1, false>);
static const DwKernel DW_KERNELS[2][2][2] = {                                   // [x is bf16][KG - 1][keep bits]
    {{k_gate_bwd_dw<false, 1, false>, k_gate_bwd_dw<false, 1, true>}, {k_gate_bwd_dw<false, 2, false>, k_gate_bwd_dw<false, 2, true>}},
    {{k_gate_bwd_dw<true, 1, false>, k_gate_bwd_dw<true, 1, true>}, {k_gate_bwd_dw<true, 2, false>, k_gate_bwd_dw<true, 2, true>}}};
using Dw2Kernel = decltype(&k_gate_bwd_dw2<false>);
static const Dw2Kernel DW2_KERNELS[2][2] = {                                    // [split-bf16 K loop][keep bits]
    {k_gate_bwd_dw2<false>, k_gate_bwd_dw2<true>},
    {k_gate_bwd_dw2_pieces<false>, k_gate_bwd_dw2_pieces<true>}};
using Dw2MpKernel = decltype(&k_gate_bwd_dw2_pieces_mp<false>);
static const Dw2MpKernel DW2_MP_KERNELS[2] = {k_gate_bwd_dw2_pieces_mp<false>, k_gate_bwd_dw2_pieces_mp<true>};   // [keep bits]

// The K loop of the dw2 route: the split-bf16 kernel (k_gate_bwd_dw2_pieces) unless MIL_DW_PIECES=0 asks for the f32-MFMA
// one.  Read per call (under a hipGraph: at capture), so A/B runs and tests toggle it inside one process; the route plan,
// the workspace and the fold are the same for both.
bool gate_dw_pieces_on() {
    const char* e = getenv("MIL_DW_PIECES");
    return e == nullptr || atoi(e) != 0;
}
static inline bool dw_pieces_on() { return gate_dw_pieces_on(); }

// bf16 x has no dw2 kernel: where the plan says dw2 it runs k_gate_bwd_dw<true, 2>
static inline bool gate_dw_is_dw2(const GateDwPlan& p, bool xb16) { return !xb16 && p.dw == MIL_ROUTE_DW2; }
// How many [4][192] groups of bias / w / b sums the plan's launch leaves in the workspace: one per (row chunk, column tile)
// from the dw2 kernels, one per row chunk from k_gate_bwd_dw
static inline int gate_dw_bias_groups(const GateDwPlan& p, int L, bool xb16) { return gate_dw_is_dw2(p, xb16) ? p.S * (L / 128) : p.S; }
static inline size_t gate_bwd_ws_floats(int S, int L) { return (size_t)S * GF_NG * L + (size_t)S * (L / 128) * 4 * 192; }

extern "C" size_t mil_gate_bwd_workspace_floats(int R, int L) {
    if (R <= 0 || L <= 0 || (L % 128) != 0) return 0;
    return gate_bwd_ws_floats(gate_dw_plan(R, L, MIL_NUM_CU).S, L);
}

static void gate_dw_launch(const GateDwPlan& p, bool xb16, const void* x, const float* gates, const float* ds, const float* w, float* part,
                           float* pbias, int R, int L, const uint32_t* xbits, const int32_t* rows_dev, hipStream_t st) {
    const int NJ = L / 128, drop = xbits != nullptr;
    const dim3 grid(p.S * 3 * NJ);
    if (gate_dw_is_dw2(p, xb16)) {
        hipLaunchKernelGGL(DW2_KERNELS[dw_pieces_on()][drop], grid, dim3(512), 0, st, (const float*)x, gates, ds, w, part, pbias, R, L, p.kc,
                           NJ, xbits, rows_dev);
    } else {
        const int kg = p.dw == MIL_ROUTE_DW_KG1 ? 1 : 2;
        hipLaunchKernelGGL(DW_KERNELS[xb16][kg - 1][drop], grid, dim3(256 * kg), 0, st, x, gates, ds, w, part, pbias, R, L, p.kc, NJ, xbits,
                           rows_dev);
    }
}

// The two launches of mil_gate_bwd_params as separate entry points (bench.py times the MFMA kernel alone).
// x: fp32, or bf16 with xb16.  Workspace: the partial tiles [S][384][L], then the groups of bias / w / b sums.
static int gate_bwd_partials_impl(const void* x, bool xb16, const float* gates, const float* ds, const float* w, int R, int L,
                                  int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                  const int32_t* rows_dev, void* stream) {
    if (!x || !gates || !ds || !w || !workspace) return MIL_EINVAL;
    if (D != MIL_GATE_D || L <= 0 || (L % 128) != 0 || R <= 0) return MIL_EINVAL;
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);
    if (workspace_floats < gate_bwd_ws_floats(p.S, L)) return MIL_ENOSPC;
    gate_dw_launch(p, xb16, x, gates, ds, w, workspace, workspace + (size_t)p.S * GF_NG * L, R, L, xbits, rows_dev, (hipStream_t)stream);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// The weight gradient of the deferred pool (gate_route_plan: the dw2 plan on the pieces kernel, R % 32 == 0, whole slices inside
// one bag, at most MP_SLOTS bags per chunk): k_gate_bwd_dw2_pieces_mp, same workspace, plus the M sums in mp.mpart
extern "C" size_t mil_pool_deferred_workspace_floats(int R, int L) {
    if (R <= 0 || L <= 0 || (L % 128) != 0) return 0;
    return (size_t)gate_dw_plan(R, L, MIL_NUM_CU).S * MP_SLOTS * MP_ROWS * L;
}
int gate_bwd_partials_mp(const float* x, const float* gates, const float* ds, const float* w, int R, int L, float* workspace,
                         size_t workspace_floats, const uint32_t* xbits, const GateDwMpool& mp, void* stream) {
    if (!x || !gates || !ds || !w || !workspace || !mp.a || !mp.tile_map || !mp.mpart) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0 || (R % MIL_POOL_TILE) != 0) return MIL_EINVAL;
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);
    if (p.dw != MIL_ROUTE_DW2 || (p.kc % GB_BKR) != 0) return MIL_EINVAL;
    if (workspace_floats < gate_bwd_ws_floats(p.S, L)) return MIL_ENOSPC;
    const int NJ = L / 128;
    hipLaunchKernelGGL(DW2_MP_KERNELS[xbits != nullptr], dim3(p.S * 3 * NJ), dim3(512), 0, (hipStream_t)stream, x, gates, ds, w, workspace,
                       workspace + (size_t)p.S * GF_NG * L, R, L, p.kc, NJ, xbits, mp.a, mp.tile_map, mp.mpart);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

extern "C" int mil_gate_bwd_partials(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                     int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                     void* stream) {
    return gate_bwd_partials_impl(x, false, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, nullptr, stream);
}
// rows_dev: device int32 holding the TRUE number of rows (<= R).  R then is the bucket the launch is sized for (grid,
// split-K plan, workspace); rows beyond the true count contribute nothing.  One launch configuration - one captured
// graph - serves every batch of the bucket.
extern "C" int mil_gate_bwd_partials_rows(const float* x, const float* gates, const float* ds, const float* w, int R, int L,
                                          int D, float* workspace, size_t workspace_floats, const uint32_t* xbits,
                                          const int32_t* rows_dev, void* stream) {
    return gate_bwd_partials_impl(x, false, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, rows_dev, stream);
}

// The fold of the workspace gate_bwd_partials_impl filled for (R, L, xb16): the same plan gives its layout
// the head arguments of a fold launch that forms M itself (the deferred pool)
static HeadBwdArgs head_args_mp(const float* dz, float* dWf, float* dbf, const float* loss_bag, float* loss_out, int B, int L, int C,
                                int accumulate, float xscale, const GateDwMpool& mp, int R) {
    HeadBwdArgs h{dz, mp.M, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate};
    h.mpart = mp.mpart;
    h.tile_map = mp.tile_map;
    h.bag_tile_off = mp.bag_tile_off;
    h.M_out = mp.M;
    h.Mdrop_out = mp.Mdrop;
    h.mbits = mp.mbits;
    h.mscale = mp.mscale;
    h.xscale = xscale;
    h.kc = gate_dw_plan(R, L, MIL_NUM_CU).kc;
    return h;
}
static int gate_bwd_fold(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu, float* dw, float* db,
                         int accumulate, float wscale, void* stream, const HeadBwdArgs* head = nullptr,
                         const AdamFuse* ad = nullptr, uint16_t* Wp = nullptr, bool xb16 = false) {
    const GateDwPlan p = gate_dw_plan(R, L, MIL_NUM_CU);
    return launch_gate_bwd_reduce(workspace, workspace + (size_t)p.S * GF_NG * L, p.S, gate_dw_bias_groups(p, L, xb16), L, dWv, dbv, dWu,
                                  dbu, dw, db, accumulate, wscale, (hipStream_t)stream, head, ad, nullptr, nullptr, Wp);
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
                                   uint16_t* Wp, const GateDwMpool* mp) {
    if (!workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db || !dz || !M || !dWf || !dbf) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0 || B <= 0 || C <= 0 || C > 32 || (loss_bag && !loss_out)) return MIL_EINVAL;
    if (mp != nullptr && (C != 2 || !mp->mpart || !mp->tile_map || !mp->bag_tile_off || !mp->M)) return MIL_EINVAL;
    const HeadBwdArgs head = mp != nullptr ? head_args_mp(dz, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate, xscale, *mp, R)
                                           : HeadBwdArgs{dz, M, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate};
    AdamFuse ad{};
    const int rc = gate_adam_fuse(dWv, dbv, dWu, dbu, dw, db, head, param_flat, grad_flat, n_param, exp_avg, exp_avg_sq, step, step_dev,
                                  lr, lr_dev, beta1, beta2, eps, weight_decay, grad_scale, done, &ad);
    if (rc != MIL_OK) return rc;
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, stream, &head, &ad, Wp);
}

int gate_bwd_reduce_head_mp(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu, float* dw,
                            float* db, int accumulate, float xscale, const float* dz, float* dWf, float* dbf, int B, int C,
                            const float* loss_bag, float* loss_out, const GateDwMpool& mp, void* stream) {
    if (!workspace || !dWv || !dbv || !dWu || !dbu || !dw || !db || !dz || !dWf || !dbf) return MIL_EINVAL;
    if (L <= 0 || (L % 128) != 0 || R <= 0 || B <= 0 || C != 2 || (loss_bag && !loss_out)) return MIL_EINVAL;
    if (!mp.mpart || !mp.tile_map || !mp.bag_tile_off || !mp.M) return MIL_EINVAL;
    const HeadBwdArgs head = head_args_mp(dz, dWf, dbf, loss_bag, loss_out, B, L, C, accumulate, xscale, mp, R);
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xscale, stream, &head);
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

// bf16 x: k_gate_bwd_dw<true, KG> where fp32 x would take k_gate_bwd_dw2
extern "C" int mil_gate_bwd_params_x16(const uint16_t* x, const float* gates, const float* ds, const float* w, int R,
                                       int L, int D, float* workspace, size_t workspace_floats, float* dWv, float* dbv,
                                       float* dWu, float* dbu, float* dw, float* db, int accumulate, const uint32_t* xbits,
                                       float xscale, void* stream) {
    if (!dWv || !dbv || !dWu || !dbu || !dw || !db) return MIL_EINVAL;
    const int rc = gate_bwd_partials_impl(x, true, gates, ds, w, R, L, D, workspace, workspace_floats, xbits, nullptr, stream);
    if (rc != MIL_OK) return rc;
    return gate_bwd_fold(workspace, R, L, dWv, dbv, dWu, dbu, dw, db, accumulate, xbits ? xscale : 1.0f, stream, nullptr, nullptr, nullptr,
                         true);
}
