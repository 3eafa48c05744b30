// K1a: gate forward of the gated-attention MIL pooling (ABMIL) for gfx950, and the route plan of the fp32 gate step.
//
// Reference arithmetic: model/dim1/ABMIL.py:47-56.  The gate GEMM x[R,L] . [Wv;Wu]^T -> [R,384] is a dense fp32
// contraction: v_mfma_f32_32x32x2_f32 (exact f32, 157 TFLOP/s roof), or the split-bf16 loop of
// k_gate_fwd2<.., PW>.  The other stages of K1: attn_pool.hip (pool, ds), gate_bwd_dw.hip, gate_bwd_dx.hip.
//
// The 128-row kernels are built from parts: GateFwdCoord (who am I), GateKeepWords (dropout keep bits), one K loop
// (k_gate_fwd's own, gate_kloop_f32 or gate_kloop_pw: each owns its staging, its LDS image and its barriers),
// gate_fwd_scores_epilogue, and the fused pool pass (gate_pool_request_rows / gate_fwd_pool_pass).
#include "mil_internal.h"
#include "philox.h"
#include <stdlib.h>
#include <type_traits>

// ================================================================================ K1a gate forward
// Workgroup: 512 threads = 8 waves, tile = 128 rows x all 384 gate columns, K-slices of 32, double-buffered in LDS.
//   wave (wr, wc): rows 32*wr..+31, d-chunks {3wc, 3wc+1, 3wc+2} for both V and U  -> 6 accumulators, so V_d and
//   U_d of a row land in the same lane and the gate product / score reduction never leave registers.
// k permutation: lane (r, h) reads 4 consecutive k = 8t+4h..+3 (one ds_read_b128) and feeds element j to the j-th of
// 4 MFMAs, so MFMA (t, j) contracts k in {8t+j, 8t+4+j}: A and B use the same map, the sum over a slice is complete.
// Staging: global -> LDS directly (global_load_lds_dwordx4: no staging VGPRs, no ds_write).  An LDS-DMA
// wave-instruction writes 64 x 16 B contiguously (8 rows of 128 B), so the image cannot be padded: rows are 32 words
// and the 16-byte chunk c of row `row` sits at chunk c ^ ((row >> 1) & 7) (applied to the per-lane SOURCE address,
// the same XOR on the fragment reads).  Over any 16-lane ds_read_b128 group (row >> 1) & 7 takes all 8 values for
// both row parities -> conflict-free (SQ_LDS_BANK_CONFLICT = 0).
// Schedule: the 8 DMA pieces of slice s+1 and the fragment reads of the next k-group are pinned between the MFMA
// groups of slice s (sched_barrier); one barrier per slice, in front of which hipcc drains the DMA (vmcnt(0)).
// Measured at 32 x 1024 x 512 (us): register-staged + padded image 109.4, this form 105.8, bit-identical results;
// main loop alone 92.5 (bare MFMA stream), +staging, +6 for the epilogue (fast activations; ocml tanhf/expf +4).
#define GF_TM 128
#define GF_BK 32

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) const f32x4 lds_cf4;
typedef __attribute__((address_space(3))) f32x4 lds_f4;
typedef __attribute__((address_space(3))) float lds_f32;      // the parts take smem as an LDS pointer, not a generic one

// Lane and workgroup coordinates of the 128-row kernels, built once at the top of the kernel and handed to the parts by
// value.  UNIFORM_WAVE = false (k_gate_fwd, whose DMA sources are per-lane pointers anyway) leaves the wave index a VGPR.
struct GateFwdCoord {
    int tid, lane, wave;        // wave is wave-uniform (an SGPR, through readfirstlane)
    int wr, wc;                 // wave (wr, wc): rows 32 wr .. + 31 of the tile, d-chunks 3 wc .. 3 wc + 2
    int r, h;                   // lane (r, h) of the 32 x 32 MFMA operand layout
    int row0, rows_here;        // first row of the workgroup's tile, and how many of its 128 rows exist
    unsigned lds0;              // LDS byte address of smem
};
template <bool UNIFORM_WAVE = true>
__device__ __forceinline__ GateFwdCoord gate_fwd_coord(const float* smem, int R) {
    GateFwdCoord co;
    co.tid = threadIdx.x;
    co.lane = co.tid & 63;
    co.wave = UNIFORM_WAVE ? __builtin_amdgcn_readfirstlane(co.tid >> 6) : co.tid >> 6;
    co.wr = co.wave >> 1;
    co.wc = co.wave & 1;
    co.r = co.lane & 31;
    co.h = co.lane >> 5;
    co.row0 = blockIdx.x * GF_TM;
    co.rows_here = min(GF_TM, R - co.row0);
    co.lds0 = (unsigned)(uintptr_t)(lds_void*)smem;
    return co;
}

__device__ __forceinline__ void gate_acc_clear(f32x16 (&acc)[3][2]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][u][i] = 0.f;
}

// LDS regions of the epilogue and of the fused pool pass (float offsets into smem: the K loop's buffers are dead by then)
#define GF_SRED_OFF 0                          /* [2 wc][128] the two halves of every row's score */
#define GF_SC_OFF (2 * GF_TM)                  /* [128] final scores, for the fused pool pass */
#define GF_PRED_OFF 1024                       /* [4 tiles][2 virtual waves][NQ][256] pool sums of the wc = 1 waves */
#define GF_PRED_FLOATS(NQ) (4 * 2 * (NQ) * 256)
static_assert(GF_SRED_OFF + 2 * GF_TM <= GF_SC_OFF && GF_SC_OFF + GF_TM <= GF_PRED_OFF, "epilogue LDS regions overlap");

// Activations, the gates store, the score of every row: acc = x . [Wv; Wu]^T of this wave's 32 rows x 3 d-chunks.  In
// train mode the survivors' scale 1/(1-p) is applied here.  copy_scores: the final scores also go to smem + GF_SC_OFF
// (-inf for rows beyond R); the caller puts a barrier in front of reading them.
template <bool DROP>
__device__ __forceinline__ void gate_fwd_scores_epilogue(const GateFwdCoord co, const f32x16 (&acc)[3][2], const float* bv,
                                                         const float* bu, const float* wvec, const float* battn,
                                                         float* scores, float* gates, int R, float xscale, lds_f32* smem,
                                                         bool copy_scores) {
    float part[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d = 32 * (3 * co.wc + c) + co.r;
        const float bvd = bv[d], bud = bu[d], wd = wvec[d];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = fast_tanh(DROP ? fmaf(acc[c][0][i], xscale, bvd) : acc[c][0][i] + bvd);
            const float u = fast_sigmoid(DROP ? fmaf(acc[c][1][i], xscale, bud) : acc[c][1][i] + bud);
            part[i] += wd * v * u;
            if (gates != nullptr) {
                const int gr = co.row0 + 32 * co.wr + mfma32_row(i, co.h);
                if (gr < R) {
                    gates[(size_t)gr * GF_NG + d] = v;
                    gates[(size_t)gr * GF_NG + 192 + d] = u;
                }
            }
        }
    }
    lds_f32* sred = smem + GF_SRED_OFF;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float v = half_sum_lane31(part[i]);
        if (co.r == 31) sred[co.wc * GF_TM + 32 * co.wr + mfma32_row(i, co.h)] = v;
    }
    __syncthreads();
    if (co.tid < GF_TM) {
        const int gr = co.row0 + co.tid;
        const float sc = sred[co.tid] + sred[GF_TM + co.tid] + battn[0];
        if (gr < R) scores[gr] = sc;
        if (copy_scores) smem[GF_SC_OFF + co.tid] = gr < R ? sc : -INFINITY;
    }
}

// L > 4096 (gate_route_plan: MIL_ROUTE_MAIN_LEGACY): the K loop with 64-bit source pointers, in the kernel body.
// DROP: train mode (ABMIL.py:49).  xbits [R][L/32] keep bits (csrc/dropout.hip); a K-slice is 32 columns = ONE word per
// row, loaded one slice ahead next to the DMA pieces; the A fragment of lane (r, h) holds k = 8t + 4h + j, so the word is
// shifted by 4h once and element (t, j) is kept by bit 8t + j (two VALU per element, under the MFMAs).
template <bool DROP>
__global__ __launch_bounds__(512) void k_gate_fwd(const float* __restrict__ x, const float* __restrict__ Wv,
                                                       const float* __restrict__ bv, const float* __restrict__ Wu,
                                                       const float* __restrict__ bu, const float* __restrict__ wvec,
                                                       const float* __restrict__ battn, float* __restrict__ scores,
                                                       float* __restrict__ gates, int R, int L,
                                                       const uint32_t* __restrict__ xbits, float xscale) {
    __shared__ __attribute__((aligned(16))) float smem[2 * (GF_TM + GF_NG) * 32];
    float* xs = smem;                      // [2][128][32]
    float* ws = smem + 2 * GF_TM * 32;     // [2][384][32]
    const GateFwdCoord co = gate_fwd_coord<false>(smem, R);
    const int lane = co.lane, wave = co.wave, wr = co.wr, wc = co.wc, r = co.r, h = co.h, row0 = co.row0;
    // DMA pieces of this wave: 2 x-pieces (8 rows each) and 6 W-pieces; lane -> (row in piece, physical chunk)
    const int prow = lane >> 3, pch = lane & 7;
    const float* gsrc[8];
    int ldst[8];                           // LDS float offset of the piece base (wave-uniform) inside one buffer
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < 2) {
            const int lr = (2 * wave + i) * 8 + prow;                         // row inside the 128-row tile
            const int gr = min(row0 + lr, R - 1);
            gsrc[i] = x + (size_t)gr * L + 4 * (pch ^ ((lr >> 1) & 7));
            ldst[i] = (2 * wave + i) * 8 * 32;
        } else {
            const int wrow = (6 * wave + (i - 2)) * 8 + prow;                 // 0..383
            gsrc[i] = (wrow < 192 ? Wv + (size_t)wrow * L : Wu + (size_t)(wrow - 192) * L) + 4 * (pch ^ ((wrow >> 1) & 7));
            ldst[i] = (6 * wave + (i - 2)) * 8 * 32;
        }
    }
    auto dma_piece = [&](int i, int buf, int k0) {
        float* dst = (i < 2 ? xs + buf * GF_TM * 32 : ws + buf * GF_NG * 32) + ldst[i];
        __builtin_amdgcn_global_load_lds(gsrc[i] + k0, (lds_void*)dst, 16, 0, 0);
    };
    f32x16 acc[3][2];
    gate_acc_clear(acc);

    const int nslice = L / GF_BK;
    // (starting each workgroup's K loop at a different slice, to de-correlate the L2 requests for the shared gate
    //  weights, measured no gain: 107.4 vs 106.2 us fp32, 172 vs 171 us bf16 - the slices stay in natural order)
    const uint32_t* mrow = nullptr;                    // keep bits of this lane's fragment row
    unsigned mnext = 0;
    if (DROP) {
        mrow = xbits + (size_t)min(row0 + 32 * wr + r, R - 1) * nslice;
        mnext = mrow[0];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) dma_piece(i, 0, 0);
    __syncthreads();                                   // hipcc drains the DMA (vmcnt(0)) in front of the barrier
    const int fx = (r >> 1) & 7;                       // swizzle term of this lane's fragment rows (row % 32 == r)
    for (int s = 0; s < nslice; ++s) {
        const int buf = s & 1;
        const int k1 = min(s + 1, nslice - 1) * GF_BK;
        unsigned mcur = 0;
        if (DROP) {
            mcur = mnext >> (4 * h);
            mnext = mrow[min(s + 1, nslice - 1)];
        }
        const float* xa = xs + (buf * GF_TM + 32 * wr + r) * 32;
        const float* wb = ws + (buf * GF_NG + 32 * 3 * wc + r) * 32;
        f32x4 a[2], b[2][3][2];
        auto frag_piece = [&](int t, int q, int p) {
            const int ch = 4 * ((2 * t + h) ^ fx);
            if (p == 0) {
                a[q] = *reinterpret_cast<const f32x4*>(xa + ch);
            } else {
                const int c = (p - 1) >> 1, u = (p - 1) & 1;
                b[q][c][u] = *reinterpret_cast<const f32x4*>(wb + (u * 192 + 32 * c) * 32 + ch);
            }
        };
#pragma unroll
        for (int p = 0; p < 7; ++p) frag_piece(0, 0, p);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = t & 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = 4 * t + j;
                if (g < 8) dma_piece(g, buf ^ 1, k1);     // next slice, one DMA piece per MFMA group
                if (t < 3) {
                    frag_piece(t + 1, q ^ 1, 2 * j);
                    if (2 * j + 1 < 7) frag_piece(t + 1, q ^ 1, 2 * j + 1);
                }
                const float av = DROP ? keep_if(a[q][j], mcur, 8 * t + j) : a[q][j];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        acc[c][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[q][c][u][j], acc[c][u], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
    gate_fwd_scores_epilogue<DROP>(co, acc, bv, bu, wvec, battn, scores, gates, R, xscale, (lds_f32*)smem, false);
}

// ================================================================================ K1a gate forward, L <= 4096
// k_gate_fwd2<DROP, GEN, PQ, PW>: the same tiling, k order and epilogue as k_gate_fwd, with 32-bit buffer offsets.
//   PW   which K loop: gate_kloop_f32 (same results as k_gate_fwd, bit for bit; MIL_GATE_PIECES=0) or gate_kloop_pw
//        (split-bf16, the default of the fp32 one-call step)
//   GEN  the workgroup draws its keep words itself (GateFwdGen, GateKeepWords)
//   PQ   > 0 (= L / 256): the pool partial pass runs behind the epilogue (GateFwdPool, gate_fwd_pool_pass)
#define GF2_XS_BYTES (GF_TM * 32 * 4)          /* gate_kloop_f32: one x buffer  (16 KB) */
#define GF2_WS_BYTES (GF_NG * 32 * 4)          /* gate_kloop_f32: one W buffer  (48 KB) */
#define GP_XS_BYTES (GF_TM * 16 * 4)           /* gate_kloop_pw: one x buffer            (8 KiB) */
#define GP_WS_BYTES (GP_SLICE_ELEMS * 2)       /* gate_kloop_pw: one W piece block      (36 KiB) */
constexpr int gate_fwd2_smem_floats(bool pw) { return pw ? 2 * (GP_XS_BYTES + GP_WS_BYTES) / 4 : 2 * (GF2_XS_BYTES + GF2_WS_BYTES) / 4; }
static_assert(GF_PRED_OFF + GF_PRED_FLOATS(2) <= gate_fwd2_smem_floats(false) &&
                  GF_PRED_OFF + GF_PRED_FLOATS(2) <= gate_fwd2_smem_floats(true),
              "the epilogue / pool regions must fit the LDS image of either K loop");

// GEN (train mode, L <= 1024): the workgroup DRAWS the keep words of its 128 rows itself - the same Philox blocks
// k_dropout_keep_bits would produce (philox.h) - keeps them in LDS for its own A fragments and writes them to xbits for
// the later consumers (pool, weight gradient); workgroup 0 also draws the head's [B, L/32] words.  One launch less per
// step, and the mask words of the loop come from LDS instead of a buffer load.
struct GateFwdGen {
    uint32_t* xbits_out;        // [R, L/32]
    uint32_t* mbits_out;        // [B, L/32] or NULL
    int B;
    uint32_t seed_lo, seed_hi, mseed_lo, mseed_hi;
    uint64_t offset;
    const int32_t* offset_dev;
};

// Keep words of this lane's fragment row (row 32 wr + r of the tile), one word per 32 columns: from xbits through a
// buffer resource, or (GEN) drawn by init() into mlds [128][L/32].  Both K loops walk them the same way:
//   unsigned mnext = kw.first();  per 32 columns s: { use mnext; mnext = kw.word(min(s + 1, nslice - 1)); }
template <bool DROP, bool GEN>
struct GateKeepWords {
    uint32_t* mlds;
    __amdgpu_buffer_rsrc_t srd_m;
    int vmask;                  // GEN: word index of the row in mlds; else byte offset of the row in srd_m
    unsigned w0;                // !GEN: the word of slice 0, requested by init()
    uint64_t off;               // GEN: the Philox offset of this step

    // in front of the K loop's first load; the GEN words are visible after the barrier behind that load
    __device__ __forceinline__ void init(const GateFwdCoord co, const uint32_t* xbits, const GateFwdGen& gen, uint32_t* lds,
                                         int L) {
        const int nslice = L / GF_BK;
        mlds = lds;
        vmask = 0;
        w0 = 0;
        off = 0;
        if (DROP && !GEN) {
            srd_m = __builtin_amdgcn_make_buffer_rsrc((void*)(xbits + (size_t)co.row0 * nslice), 0, co.rows_here * nslice * 4,
                                                      MIL_SRD_FLAGS);
            vmask = (32 * co.wr + co.r) * nslice * 4;
            w0 = __builtin_amdgcn_raw_buffer_load_b32(srd_m, vmask, 0, 0);
        }
        if (GEN) {
            off = gen.offset;
            if (gen.offset_dev != nullptr) off += (uint64_t)(uint32_t)gen.offset_dev[0];
            const size_t blk0 = (size_t)co.row0 * nslice / 4;               // 128 nslice words per workgroup: a multiple of 4
            const int nblk = co.rows_here * nslice / 4;                     // nslice % 4 == 0 (host)
            for (int q = co.tid; q < nblk; q += 512) {
                const uint4 wds = philox_keep_words_half(blk0 + q, off, gen.seed_lo, gen.seed_hi);
                *reinterpret_cast<uint4*>(gen.xbits_out + 4 * (blk0 + q)) = wds;
                *reinterpret_cast<uint4*>(mlds + 4 * q) = wds;
            }
            if (blockIdx.x == 0 && gen.mbits_out != nullptr) {
                const int nw = gen.B * (L >> 5);                            // even (L % 64 == 0)
                for (int q = co.tid; 2 * q < nw; q += 512) {
                    const uint2 wds = philox_keep_words_quarter((uint64_t)q, off, gen.mseed_lo, gen.mseed_hi);
                    gen.mbits_out[2 * q] = wds.x;
                    gen.mbits_out[2 * q + 1] = wds.y;
                }
            }
            vmask = (32 * co.wr + co.r) * nslice;
        }
    }
    __device__ __forceinline__ unsigned first() const { return GEN ? mlds[vmask] : w0; }
    __device__ __forceinline__ unsigned word(int s1) const {
        if (GEN) return mlds[vmask + s1];
        return __builtin_amdgcn_raw_buffer_load_b32(srd_m, vmask, s1 * 4, 0);
    }
};

// ---- K loop on the f32 MFMA, "VALU diet" form: k_gate_fwd's loop without the vector-ALU instructions that the f32 MFMA
// cannot hide (see k_gate_bwd_dw2 / tools/mfma_valu_mix.hip).  LDS image as k_gate_fwd's: [2] x buffers [128][32], then
// [2] W buffers [384][32], chunk c of a row at c ^ ((row >> 1) & 7).
//   * LDS-DMA through buffer resources (buffer_load_dwordx4 ... lds): the per-lane source offset is a loop invariant, the
//     K offset an SGPR, the LDS destination goes to M0 by scalar ALU (no 64-bit pointer adds, no v_readfirstlane);
//     rows of the last tile beyond R read as zeros by the hardware range check;
//   * fragment reads are ds_read_b128 with immediate offsets from twelve precomputed per-lane LDS addresses (the buffer
//     index is a compile-time constant: the slice loop is unrolled by two);
//   * in train mode the keep-mask word of the next slice comes through a buffer resource as well (or from LDS, GEN).
// Left in the loop per 32-column slice and wave: the mask itself (2 VALU per A element, train mode only).
// Owns everything from the slice-0 load to the barrier behind the last slice.
template <bool DROP, bool GEN>
__device__ __forceinline__ void gate_kloop_f32(const GateFwdCoord co, const GateKeepWords<DROP, GEN>& kw, const float* x,
                                               const float* Wv, const float* Wu, int L, f32x16 (&acc)[3][2]) {
    const int lane = co.lane, wave = co.wave, wr = co.wr, wc = co.wc, r = co.r, h = co.h;
    const unsigned lds0 = co.lds0;
    const int nslice = L / GF_BK;
    // ---- DMA pieces of this wave: 2 x pieces (8 rows each), 6 W pieces; lane -> (row in piece, physical 16-byte chunk)
    const int prow = lane >> 3, pch = lane & 7;
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)co.row0 * L), 0, co.rows_here * L * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_v = __builtin_amdgcn_make_buffer_rsrc((void*)Wv, 0, MIL_GATE_D * L * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_u = __builtin_amdgcn_make_buffer_rsrc((void*)Wu, 0, MIL_GATE_D * L * 4, MIL_SRD_FLAGS);
    int vsrc[8];                 // per-lane byte offset of the piece's source (slice 0)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < 2) {
            const int lr = (2 * wave + i) * 8 + prow;
            vsrc[i] = (lr * L + 4 * (pch ^ ((lr >> 1) & 7))) * 4;
        } else {
            const int wrow = (6 * wave + (i - 2)) * 8 + prow;                 // 0..383: pieces never straddle Wv / Wu
            vsrc[i] = ((wrow % MIL_GATE_D) * L + 4 * (pch ^ ((wrow >> 1) & 7))) * 4;
        }
    }
    auto dma_piece = [&](int i, int buf, int kbytes) {            // i, buf compile-time after unrolling; kbytes scalar
        if (i < 2) {
            const unsigned dst = lds0 + (unsigned)(buf * GF2_XS_BYTES + (2 * wave + i) * 8 * 128);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_x, (lds_void*)(uintptr_t)dst, 16, vsrc[i], kbytes, 0, 0);
        } else {
            const int p = 6 * wave + (i - 2);
            const unsigned dst = lds0 + (unsigned)(2 * GF2_XS_BYTES + buf * GF2_WS_BYTES + p * 8 * 128);
            if (p < 24) __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_v, (lds_void*)(uintptr_t)dst, 16, vsrc[i], kbytes, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_u, (lds_void*)(uintptr_t)dst, 16, vsrc[i], kbytes, 0, 0);
        }
    };
    // ---- fragment addresses (bytes): row (32 wr + r) of the x image / row (96 wc + r) of the W image, swizzled chunk of k-group t
    const int fx = (r >> 1) & 7;
    unsigned fa_addr[4], fb_addr[2][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const unsigned ch = 16u * (unsigned)((2 * t + h) ^ fx);
        fa_addr[t] = lds0 + (unsigned)((32 * wr + r) * 128) + ch;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            fb_addr[b][t] = lds0 + (unsigned)(2 * GF2_XS_BYTES + b * GF2_WS_BYTES + (96 * wc + r) * 128) + ch;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) dma_piece(i, 0, 0);
    __syncthreads();                                   // hipcc drains the DMA (vmcnt(0)) in front of the barrier
    unsigned mnext = kw.first();

    auto slice = [&](int s, auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        const int s1 = min(s + 1, nslice - 1);
        const int k1bytes = s1 * GF_BK * 4;
        unsigned mcur = 0;
        if (DROP) {
            mcur = mnext >> (4 * h);
            mnext = kw.word(s1);
        }
        f32x4 a[2], b[2][3][2];
        auto frag_piece = [&](int t, int q, int p) {
            if (p == 0) {
                a[q] = *(lds_cf4*)(uintptr_t)(fa_addr[t] + (unsigned)(buf * GF2_XS_BYTES));
            } else {
                const int c = (p - 1) >> 1, u = (p - 1) & 1;
                b[q][c][u] = *(lds_cf4*)(uintptr_t)(fb_addr[buf][t] + (unsigned)((u * 192 + 32 * c) * 128));
            }
        };
#pragma unroll
        for (int p = 0; p < 7; ++p) frag_piece(0, 0, p);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = t & 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = 4 * t + j;
                if (g < 8) dma_piece(g, buf ^ 1, k1bytes);     // next slice, one DMA piece per MFMA group
                if (t < 3) {
                    frag_piece(t + 1, q ^ 1, 2 * j);
                    if (2 * j + 1 < 7) frag_piece(t + 1, q ^ 1, 2 * j + 1);
                }
                const float av = DROP ? keep_if(a[q][j], mcur, 8 * t + j) : a[q][j];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        acc[c][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[q][c][u][j], acc[c][u], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    int s = 0;
    for (; s + 1 < nslice; s += 2) {
        slice(s, std::integral_constant<int, 0>{});
        __syncthreads();
        slice(s + 1, std::integral_constant<int, 1>{});
        __syncthreads();
    }
    if (s < nslice) {
        slice(s, std::integral_constant<int, 0>{});
        __syncthreads();
    }
}

// ---- split-bf16 K loop (PW): the contraction runs on v_mfma_f32_32x32x16_bf16 over three-piece bf16 operands,
// x = x0 + x1 + x2 and W = w0 + w1 + w2 (each split exact, gp_split3), keeping the six cross terms (p, q) with p + q <= 2:
// per 16 k and output tile six bf16 MFMAs of 32 cycles (192) where the f32 MFMA takes 512.  The dropped terms x1w2, x2w1,
// x2w2 are below 2^-24 relative.
//   * K slices are 16 deep (one bf16 MFMA), double-buffered, buffer = slice parity.  LDS image: [2] x buffers [128][16]
//     fp32 (64-byte rows, 16-byte chunk c of row `row` at c ^ ((row >> 2) & 3): conflict-free for the ds_read_b128 lane
//     groups), then [2] W piece blocks [3][2][384][8] bf16 of the slice (36 KiB, gp_index: copied as it lies in Wp).
//     2 x 44 KiB; 32-deep slices would need 2 x 88 KiB, over the 160 KiB of a CU.
//   * W pieces are precomputed (Wp, refreshed by the optimizer, gate_reduce.h); x is split after the fragment read, in
//     registers, by both waves that share a row tile (the VALU work hides under the bf16 MFMAs).
//   * dropped elements are zeroed before the split (all three pieces 0); 1/(1-p) stays in the epilogue.
//   * non-finite x: x0 = x, x1 = x2 = 0 (gp_split3).  A product term x0 * w_q with w_q == 0 still makes an infinite x a
//     NaN in that gate column, where the f32 loop gives +-inf (tanh/sigmoid then +-1 / 0 / 1): rows with an infinite
//     feature are not carried through this path with the f32 loop's values.
// Owns everything from the slice-0 load to the barrier behind the last slice.
// HR (the deferred pool): the loop also forms this wave's column of the head projections, hacc = x~_row . head[wc] over the
// lane's k (head: the wave's own staged head row, gate_head_rows_stage; LDS byte address), from the fragment values behind
// the keep select - 8 FMA and two broadcast ds_read_b128 per lane and 16-deep slice, under the bf16 MFMAs.
template <bool DROP, bool GEN, bool HR = false>
__device__ __forceinline__ void gate_kloop_pw(const GateFwdCoord co, const GateKeepWords<DROP, GEN>& kw, const float* x,
                                              const unsigned short* Wp, int L, f32x16 (&acc)[3][2], unsigned head = 0,
                                              float* hacc = nullptr) {
    const int lane = co.lane, wave = co.wave, wr = co.wr, wc = co.wc, r = co.r, h = co.h;
    const unsigned lds0 = co.lds0;
    const int nslice = L / GF_BK, n16 = L / 16;
    const __amdgpu_buffer_rsrc_t srd_x =
        __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)co.row0 * L), 0, co.rows_here * L * 4, MIL_SRD_FLAGS);
    const __amdgpu_buffer_rsrc_t srd_p = __builtin_amdgcn_make_buffer_rsrc((void*)Wp, 0, n16 * GP_WS_BYTES, MIL_SRD_FLAGS);
    const int xrow = 16 * wave + (lane >> 2);                         // x DMA: wave w fills rows 16w .. 16w + 15
    const int xsrc = (xrow * L + 4 * ((lane & 3) ^ ((xrow >> 2) & 3))) * 4;
    auto dma16 = [&](int buf, int s16) {
        const unsigned xdst = lds0 + (unsigned)(buf * GP_XS_BYTES + wave * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_x, (lds_void*)(uintptr_t)xdst, 16, xsrc, s16 * 64, 0, 0);
#pragma unroll
        for (int i = 0; i < 5; ++i) {                                 // 36 W pieces of 1 KiB: 4 or 5 per wave
            const int p = wave + 8 * i;
            if (i < 4 || p < 36) {
                const unsigned wdst = lds0 + (unsigned)(2 * GP_XS_BYTES + buf * GP_WS_BYTES + p * 1024);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_p, (lds_void*)(uintptr_t)wdst, 16, lane * 16,
                                                         s16 * GP_WS_BYTES + p * 1024, 0, 0);
            }
        }
    };
    // fragment reads: byte offsets into smem of row (32 wr + r) of the x image (its two swizzled chunks) and of row
    // (h, 96 wc + r) of the W block; lds0 is added at the read
    const unsigned xr = (unsigned)((32 * wr + r) * 64);
    const unsigned pa0 = xr + 16u * (unsigned)((2 * h) ^ ((r >> 2) & 3));
    const unsigned pa1 = xr + 16u * (unsigned)((2 * h + 1) ^ ((r >> 2) & 3));
    const unsigned pb = (unsigned)(2 * GP_XS_BYTES + (h * GF_NG + 96 * wc + r) * 16);
    const unsigned ph = head + 32u * (unsigned)h;                     // HR: the head row's k = 8 h .. 8 h + 7 of slice 0
    float hsum = 0.f;
    // one 16-deep slice from buffer `buf`; mw = keep bits of this lane's 8 k in bits 0..7
    auto slice16 = [&](int s16, unsigned mw, auto buf_c) {
        constexpr int buf = decltype(buf_c)::value;
        const f32x4 xa0 = *(lds_cf4*)(uintptr_t)(lds0 + pa0 + (unsigned)(buf * GP_XS_BYTES));
        const f32x4 xa1 = *(lds_cf4*)(uintptr_t)(lds0 + pa1 + (unsigned)(buf * GP_XS_BYTES));
        f32x4 bq[3][3][2];                                            // [piece][c][u], smallest piece first
#pragma unroll
        for (int q = 2; q >= 0; --q)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    bq[q][c][u] = *(lds_cf4*)(uintptr_t)(lds0 + pb + (unsigned)(buf * GP_WS_BYTES + (q * 2 * GF_NG + u * 192 + 32 * c) * 16));
        // the next slice goes to the other buffer (after this slice's reads in program order: no LDS wait in between)
        dma16(buf ^ 1, min(s16 + 1, n16 - 1));
        f32x4 hw0 = {0, 0, 0, 0}, hw1 = {0, 0, 0, 0};
        if (HR) {
            hw0 = *(lds_cf4*)(uintptr_t)(ph + (unsigned)(s16 * 64));
            hw1 = *(lds_cf4*)(uintptr_t)(ph + (unsigned)(s16 * 64) + 16u);
        }
        gp_bf16x8 ap[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = j < 4 ? xa0[j] : xa1[j - 4];
            if (DROP) v = keep_if(v, mw, j);
            if (HR) hsum = fmaf(v, j < 4 ? hw0[j] : hw1[j - 4], hsum);
            unsigned short p0, p1, p2;
            gp_split3(v, p0, p1, p2);
            ap[0][j] = __builtin_bit_cast(__bf16, p0);
            ap[1][j] = __builtin_bit_cast(__bf16, p1);
            ap[2][j] = __builtin_bit_cast(__bf16, p2);
        }
        // cross terms (p, q), p + q <= 2, smallest first; the B piece q of every tile is read before its first use
        constexpr int TP[6] = {0, 1, 2, 0, 1, 0}, TQ[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    acc[c][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[TP[t]], __builtin_bit_cast(gp_bf16x8, bq[TQ[t]][c][u]),
                                                                        acc[c][u], 0, 0, 0);
        // keep the MFMAs in front of the barrier (and its DMA drain): the next slice's DMA lands under them
        __builtin_amdgcn_sched_barrier(0);
    };
    dma16(0, 0);
    __syncthreads();                                   // hipcc drains the DMA (vmcnt(0)) in front of the barrier
    unsigned mnext = kw.first();
    for (int s = 0; s < nslice; ++s) {                                // 32-deep steps: one keep word, two slices
        unsigned mw = 0;
        if (DROP) {
            mw = mnext;
            mnext = kw.word(min(s + 1, nslice - 1));
        }
        slice16(2 * s, mw >> (8 * h), std::integral_constant<int, 0>{});
        __syncthreads();
        slice16(2 * s + 1, mw >> (16 + 8 * h), std::integral_constant<int, 1>{});
        __syncthreads();
    }
    if (HR) *hacc = hsum;
}

// ---- fused pool pass (PQ > 0, = L / 256): the attention-pool PARTIAL PASS of the workgroup's four 32-row tiles runs
// behind the epilogue, once the 128 scores are final - k_pool_partial's arithmetic, operation for operation (tile weights
// by the same wave reductions, virtual wave v = rows v, v + 4, ..., the four virtual waves of a tile folded in the same
// order, the head-projection by-product through the same 16-value reduction), so partials / hrow equal the stand-alone
// kernel's.  The rows come back from L2 / Infinity Cache (the DMA stream of the main loop read them moments ago): one
// launch and one cold start less per step - the stand-alone pass costs 14 us at 32 x 1024 x 512 although its bytes take 7.
// Only for batches whose tiles are all full and aligned (T * 32 == R, i.e. tile t = rows 32 t ..), which the host checks.
struct GateFwdPool {
    const int32_t* tile_map;    // [T][4] = {bag, row0, nrows, 0}
    float* partials;            // [T][L] then [T][2]
    int T;
    const float* Wf;            // [2][L] head rows (C == 2)
    float* hrow;                // [R][2]
    const uint32_t* mbits;      // [B][L/32] keep words of the head's dropout (train mode without GEN), else NULL
    float mscale;
};
// rows 2 wc + j + 4 i (j < 2, i < 8) of this wave's 32-row tile: lane l holds columns 256 q + 4 l .. + 3
template <int NQ>
struct GatePoolRows {
    f32x4 v[2][MIL_POOL_TILE / 4][NQ];
};
// The x rows are requested in FRONT of the activation epilogue (they depend on nothing it computes), so that their trip
// from L2 / Infinity Cache runs under it.
template <int NQ>
__device__ __forceinline__ void gate_pool_request_rows(const GateFwdCoord co, const float* x, int R, int L, GatePoolRows<NQ>& pv) {
    const int trow0 = co.row0 + 32 * co.wr;
    if (trow0 < R) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                const float* xr = x + (size_t)(trow0 + 2 * co.wc + j + 4 * i) * L + 4 * co.lane;
#pragma unroll
                for (int q = 0; q < NQ; ++q) pv.v[j][i][q] = *reinterpret_cast<const f32x4*>(xr + 256 * q);
            }
    }
}
// Behind gate_fwd_scores_epilogue<DROP>(.., copy_scores = true); pv from gate_pool_request_rows.
template <bool DROP, bool GEN, int NQ>
__device__ __forceinline__ void gate_fwd_pool_pass(const GateFwdCoord co, const GateKeepWords<DROP, GEN>& kw, GatePoolRows<NQ>& pv,
                                                   const uint32_t* xbits, int R, int L, float xscale, const GateFwdGen& gen,
                                                   const GateFwdPool& pool, lds_f32* smem) {
    const int lane = co.lane, wr = co.wr, wc = co.wc;
    const int nslice = L / GF_BK;
    const lds_f32* sc_lds = smem + GF_SC_OFF;
    lds_f32* pred = smem + GF_PRED_OFF;
    __syncthreads();
    const int trow0 = co.row0 + 32 * wr;           // this wave's tile: rows trow0 .. trow0 + 31 (wave-uniform)
    const bool live = trow0 < R;                   // R % 32 == 0 (host): a tile is whole or absent
    const int t = trow0 >> 5;
    // tile weights, as wave 0 of k_pool_partial forms them
    const float s_ = lane < 32 ? sc_lds[32 * wr + lane] : -INFINITY;
    const float m_ = wave_allmax(s_);
    const float p_ = lane < 32 ? expf(s_ - m_) : 0.f;
    const float l_ = wave_allsum(p_);
    const float xs = DROP ? xscale : 1.0f;
    f32x4 pacc[2][NQ];
    if (live) {
        auto& v = pv.v;
        const int sh = 4 * (lane & 7);
        if (DROP) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                    const int rr = 2 * wc + j + 4 * i;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const unsigned wd = GEN ? kw.mlds[(32 * wr + rr) * nslice + 8 * q + (lane >> 3)]
                                                : xbits[(size_t)(trow0 + rr) * (L >> 5) + 8 * q + (lane >> 3)];
                        const unsigned mm = wd >> sh;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[j][i][q][e] = keep_if(v[j][i][q][e], mm, e);
                    }
                }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) pacc[j][q] = f32x4{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                const int rr = 2 * wc + j + 4 * i;
                const float pw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p_), rr)) * xs;
#pragma unroll
                for (int q = 0; q < NQ; ++q) pacc[j][q] += pw * v[j][i][q];
            }
        }
        // head rows as this tile's bag sees them (k_pool_partial's head_row), then the by-product h[row][c]
        const int bag_ = pool.tile_map[4 * t];
        f32x4 wf[2][NQ];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                f32x4 w = *reinterpret_cast<const f32x4*>(pool.Wf + (size_t)c * L + 256 * q + 4 * lane) * xs;
                if (DROP) {
                    const int widx = bag_ * (L >> 5) + 8 * q + (lane >> 3);
                    unsigned wd;
                    if (GEN) {      // the word workgroup 0 writes to mbits_out in this same launch: drawn again here
                        const uint2 pr = philox_keep_words_quarter((uint64_t)(widx >> 1), kw.off, gen.mseed_lo, gen.mseed_hi);
                        wd = (widx & 1) ? pr.y : pr.x;
                    } else {
                        wd = pool.mbits[widx];
                    }
                    const unsigned mm = wd >> sh;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w[e] = keep_if(w[e], mm, e) * pool.mscale;
                }
                wf[c][q] = w;
            }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float d16[16];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int i = 0; i < MIL_POOL_TILE / 4; ++i) {
                    float d = 0.f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        d += v[j][i][q][0] * wf[c][q][0] + v[j][i][q][1] * wf[c][q][1] + v[j][i][q][2] * wf[c][q][2] + v[j][i][q][3] * wf[c][q][3];
                    d16[2 * i + c] = d;
                }
            const float tot = wave_reduce16(d16, lane);
            const int k = wave_reduce16_index(lane), rr = 2 * wc + j + 4 * (k >> 1);
            if ((lane & 3) == 0) pool.hrow[(size_t)(trow0 + rr) * 2 + (k & 1)] = tot;
        }
        if (wc == 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    *(lds_f4*)(pred + ((wr * 2 + j) * NQ + q) * 256 + 4 * lane) = pacc[j][q];
        }
    }
    __syncthreads();
    if (live && wc == 0) {
        float* out = pool.partials + (size_t)t * L;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x4 vv = pacc[0][q];
            vv += pacc[1][q];
            vv += *(lds_cf4*)(pred + ((wr * 2 + 0) * NQ + q) * 256 + 4 * lane);
            vv += *(lds_cf4*)(pred + ((wr * 2 + 1) * NQ + q) * 256 + 4 * lane);
            *reinterpret_cast<f32x4*>(out + 256 * q + 4 * lane) = vv;
        }
        if (lane == 0) {
            float* ml = pool.partials + (size_t)pool.T * L + 2 * t;
            ml[0] = m_;
            ml[1] = l_;
        }
    }
}

// ---- head projections from the K loop (HR; the deferred pool of gate_route_plan).  hrow[n][c] = x~_n . (Wf[c] keep_b mscale
// xscale), the pool pass's by-product (gate_fwd_pool_pass), needs no pass over x of its own: gate_kloop_pw holds every x~ value
// in registers.  Wave (wr, wc) stages head row c = wc as the bag of ITS 32-row tile sees it (aligned layout: a tile lies in one
// bag) into its own [L] floats of LDS in front of the loop - lane l columns 8 l .. 8 l + 7 (+ 512), under GEN with the head's
// keep words drawn again from Philox as the pool pass does - and stores the column behind it: only the wave itself reads them.
#define GF_HR_MAXL 512
template <bool DROP, bool GEN>
__device__ __forceinline__ void gate_head_rows_stage(const GateFwdCoord co, const GateKeepWords<DROP, GEN>& kw, int R, int L,
                                                     float xscale, const GateFwdGen& gen, const GateFwdPool& pool, lds_f32* mine) {
    const int trow0 = co.row0 + 32 * co.wr;
    if (trow0 >= R) return;                                // R % 32 == 0 (host): a tile is whole or absent
    const int bag_ = pool.tile_map[4 * (trow0 >> 5)];
    const float xs = DROP ? xscale : 1.0f;
    for (int col = 8 * co.lane; col < L; col += 512) {
        const float* src = pool.Wf + (size_t)co.wc * L + col;
        f32x4 w0 = *reinterpret_cast<const f32x4*>(src) * xs, w1 = *reinterpret_cast<const f32x4*>(src + 4) * xs;
        if (DROP) {
            const int widx = bag_ * (L >> 5) + (col >> 5);
            unsigned wd;
            if (GEN) {      // the word workgroup 0 writes to mbits_out in this same launch: drawn again here
                const uint2 pr = philox_keep_words_quarter((uint64_t)(widx >> 1), kw.off, gen.mseed_lo, gen.mseed_hi);
                wd = (widx & 1) ? pr.y : pr.x;
            } else {
                wd = pool.mbits[widx];
            }
            const unsigned mm = wd >> (col & 31);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w0[e] = keep_if(w0[e], mm, e) * pool.mscale;
                w1[e] = keep_if(w1[e], mm, 4 + e) * pool.mscale;
            }
        }
        *(lds_f4*)(mine + col) = w0;
        *(lds_f4*)(mine + col + 4) = w1;
    }
}
// the two half-lanes of a row hold the two halves of its k: folded once, stored by the lower one
__device__ __forceinline__ void gate_head_rows_store(const GateFwdCoord co, float hacc, int R, float* hrow) {
    const float tot = hacc + __shfl_xor(hacc, 32);
    const int gr = co.row0 + 32 * co.wr + co.r;
    if (co.h == 0 && gr < R) hrow[(size_t)gr * 2 + co.wc] = tot;
}

template <bool DROP, bool GEN, int PQ, bool PW = false, bool HR = false>
__global__ __launch_bounds__(512) void k_gate_fwd2(const float* __restrict__ x, const float* __restrict__ Wv,
                                                   const float* __restrict__ bv, const float* __restrict__ Wu,
                                                   const float* __restrict__ bu, const float* __restrict__ wvec,
                                                   const float* __restrict__ battn, float* __restrict__ scores,
                                                   float* __restrict__ gates, int R, int L,
                                                   const uint32_t* __restrict__ xbits, float xscale, GateFwdGen gen,
                                                   GateFwdPool pool, const unsigned short* __restrict__ Wp = nullptr) {
    __shared__ __attribute__((aligned(16))) float smem[gate_fwd2_smem_floats(PW)];     // the K loop's image, then the epilogue's
    __shared__ __attribute__((aligned(16))) uint32_t mlds[GEN ? GF_TM * 32 : 4];       // keep words [128][nslice <= 32]
    __shared__ __attribute__((aligned(16))) float hlds[HR ? 4 * 2 * GF_HR_MAXL : 4];   // head rows [4 tiles][2][L <= 512]
    static_assert(!HR || (PW && PQ == 0), "the head projections come from the split-bf16 loop, in place of the pool pass");
    const GateFwdCoord co = gate_fwd_coord(smem, R);
    GateKeepWords<DROP, GEN> kw;
    kw.init(co, xbits, gen, mlds, L);
    f32x16 acc[3][2];
    gate_acc_clear(acc);
    if constexpr (HR) {
        lds_f32* mine = (lds_f32*)hlds + (2 * co.wr + co.wc) * L;
        gate_head_rows_stage<DROP, GEN>(co, kw, R, L, xscale, gen, pool, mine);
        float hacc = 0.f;
        gate_kloop_pw<DROP, GEN, true>(co, kw, x, Wp, L, acc, (unsigned)(uintptr_t)(lds_void*)mine, &hacc);
        gate_head_rows_store(co, hacc, R, pool.hrow);
    } else if constexpr (PW) gate_kloop_pw<DROP, GEN>(co, kw, x, Wp, L, acc);
    else gate_kloop_f32<DROP, GEN>(co, kw, x, Wv, Wu, L, acc);
    GatePoolRows<(PQ > 0 ? PQ : 1)> pv;
    if constexpr (PQ > 0) gate_pool_request_rows(co, x, R, L, pv);
    gate_fwd_scores_epilogue<DROP>(co, acc, bv, bu, wvec, battn, scores, gates, R, xscale, (lds_f32*)smem, PQ > 0);
    if constexpr (PQ > 0) gate_fwd_pool_pass<DROP, GEN, PQ>(co, kw, pv, xbits, R, L, xscale, gen, pool, (lds_f32*)smem);
}

// ================================================================================ K1a gate forward, 32-row tiles
// Small batches (the authors train with ONE bag per GPU: R = 1 000 - 15 000 rows): 128-row tiles would leave most CUs
// idle (8 workgroups for 1024 patches, each walking all of K: the kernel takes its full ~100 us for 1/32 of the
// work).  This form uses 32-row tiles and 12 waves: wave (c, u) owns ONE accumulator tile - d-chunk c of V (u = 0) or
// of U (u = 1) - so the four SIMDs carry three waves each (six waves with two tiles would put two on some SIMDs
// and one on others); the U waves hand sigmoid(U) to their V partners through LDS for the gate product, and the
// scores still complete inside the workgroup.  Register-staged, two register sets: every load has two iterations to
// land (one L2 round trip is longer than one slice of MFMAs here).
#define GS_TM 32
#define GS_LS 36
#define GS_THREADS 768
// RT row tiles of 32 per workgroup (1 .. 3): the launch picks the smallest RT that covers the rows in ONE round of the
// grid - 384 workgroups of 32 rows are two rounds at one workgroup per CU (120 KB of LDS), 192 of 64 rows one round of
// twice the length: a bucket of 12 288 rows 57 -> 46 us.  Every wave then carries RT accumulator tiles against the same B
// fragments.
template <bool DROP, int RT>
__global__ __launch_bounds__(GS_THREADS) void k_gate_fwd_r32(const float* __restrict__ x, const float* __restrict__ Wv,
                                                             const float* __restrict__ bv, const float* __restrict__ Wu,
                                                             const float* __restrict__ bu, const float* __restrict__ wvec,
                                                             const float* __restrict__ battn, float* __restrict__ scores,
                                                             float* __restrict__ gates, int R, int L,
                                                             const uint32_t* __restrict__ xbits, float xscale,
                                                             const int32_t* __restrict__ rows_dev) {
    // bucketed batches (one ragged bag per step: R is the capacity the launch is sized for): tiles beyond the true row
    // count on the device have no reader - the tile map, the pool and the weight gradient all stop at that count
    constexpr int TM = GS_TM * RT;
    if (rows_dev != nullptr && (int)(blockIdx.x * TM) >= __builtin_amdgcn_readfirstlane(rows_dev[0])) return;
    __shared__ __attribute__((aligned(16))) float smem[2 * (TM + GF_NG) * GS_LS];
    float* xs = smem;                            // [2][32 RT][36]
    float* ws = smem + 2 * TM * GS_LS;           // [2][384][36]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = wave >> 1, isu = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * TM;
    const float* wsrc[4];
    int wdst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + GS_THREADS * i, wrow = id >> 3, ch = id & 7;
        wsrc[i] = (wrow < 192 ? Wv + (size_t)wrow * L : Wu + (size_t)(wrow - 192) * L) + 4 * ch;
        wdst[i] = wrow * GS_LS + 4 * ch;
    }
    const int xrow = (tid % (256 * RT)) >> 3, xch = tid & 7;          // threads < 256 RT stage the x rows (768 = 3 x 256)
    const float* xsrc = x + (size_t)min(row0 + xrow, R - 1) * L + 4 * xch;
    const uint32_t* msrc = DROP ? xbits + (size_t)min(row0 + xrow, R - 1) * (L / 32) : nullptr;
    const int xdst = xrow * GS_LS + 4 * xch;
    f32x4 wreg[2][4], xreg[2];
    unsigned mreg[2] = {0, 0};
    auto gload = [&](int set, int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wreg[set][i] = *reinterpret_cast<const f32x4*>(wsrc[i] + k0);
        xreg[set] = *reinterpret_cast<const f32x4*>(xsrc + k0);
        if (DROP) mreg[set] = msrc[k0 >> 5];                     // a slice = 32 columns = one word of keep bits per row
    };
    auto swrite = [&](int set, int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(ws + buf * GF_NG * GS_LS + wdst[i]) = wreg[set][i];
        if (tid < 256 * RT) {
            f32x4 v = xreg[set];
            if (DROP) {
                const unsigned m = mreg[set] >> (4 * xch);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = keep_if(v[e], m, e) * xscale;
            }
            *reinterpret_cast<f32x4*>(xs + buf * TM * GS_LS + xdst) = v;
        }
    };
    f32x16 acc[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    const int nslice = L / GF_BK;
    gload(0, 0);
    swrite(0, 0);
    gload(1, min(1, nslice - 1) * GF_BK);
    gload(0, min(2, nslice - 1) * GF_BK);
    __syncthreads();
    auto iteration = [&](int s, int set) {                       // set = (s + 1) & 1
        const int buf = s & 1;
        const float* xa = xs + buf * TM * GS_LS + r * GS_LS + 4 * h;
        const float* wb = ws + buf * GF_NG * GS_LS + (192 * isu + 32 * c + r) * GS_LS + 4 * h;
        f32x4 fa[RT][4], fb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int q = 0; q < RT; ++q) fa[q][t] = *reinterpret_cast<const f32x4*>(xa + q * GS_TM * GS_LS + 8 * t);
            fb[t] = *reinterpret_cast<const f32x4*>(wb + 8 * t);
        }
        swrite(set, buf ^ 1);                                    // slice s+1: registers -> the other buffer
        gload(set, min(s + 3, nslice - 1) * GF_BK);              // the same registers take slice s+3
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int q = 0; q < RT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][t][jj], fb[t][jj], acc[q], 0, 0, 0);
        __syncthreads();
    };
    for (int s = 0; s < nslice; s += 2) {
        iteration(s, 1);
        if (s + 1 < nslice) iteration(s + 1, 0);
    }
    const int d = 32 * c + r;
    float* uex = smem;                           // [6][32][33]: sigmoid(U) tiles for the V partners
    float* sred = smem + 6 * 32 * 33;            // [6][32]
#pragma unroll
    for (int q = 0; q < RT; ++q) {
        float gv[16];
        if (q > 0) __syncthreads();              // the previous row tile's uex / sred have been read
        if (isu) {
            const float bud = bu[d];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                gv[i] = fast_sigmoid(acc[q][i] + bud);
                uex[(c * 32 + mfma32_row(i, h)) * 33 + r] = gv[i];
            }
        } else {
            const float bvd = bv[d];
#pragma unroll
            for (int i = 0; i < 16; ++i) gv[i] = fast_tanh(acc[q][i] + bvd);
        }
        if (gates != nullptr) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int gr = row0 + GS_TM * q + mfma32_row(i, h);
                if (gr < R) gates[(size_t)gr * GF_NG + 192 * isu + d] = gv[i];
            }
        }
        __syncthreads();
        if (!isu) {
            const float wd = wvec[d];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int lr = mfma32_row(i, h);
                const float part = half_allsum(wd * gv[i] * uex[(c * 32 + lr) * 33 + r]);
                if (r == 0) sred[c * GS_TM + lr] = part;
            }
        }
        __syncthreads();
        if (tid < GS_TM && row0 + GS_TM * q + tid < R) {
            float sc = battn[0];
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) sc += sred[cc * GS_TM + tid];
            scores[row0 + GS_TM * q + tid] = sc;
        }
    }
}

// The few rows beyond whole rounds of the grid (gate_route_plan, MIL_ROUTE_TAIL_SMALL): scores from the V, U that
// mil_linear_small_fwd wrote into the gates buffer.
__global__ __launch_bounds__(64) void k_gate_tail_scores(const float* __restrict__ gates, const float* __restrict__ wvec,
                                                         const float* __restrict__ battn, float* __restrict__ scores) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* gr = gates + (size_t)row * GF_NG;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) v += wvec[64 * q + lane] * gr[64 * q + lane] * gr[192 + 64 * q + lane];
    v = wave_allsum(v);
    if (lane == 0) scores[row] = v + battn[0];
}

// ================================================================================ host side
// ---- the route plan: which kernels the fp32 gate step launches for a shape, decided here and nowhere else
// (mil_gate_route, include/mil_hip.h).  Pure host arithmetic: no HIP call, the CU count comes in as a parameter.
struct GateRouteIn {
    int R, L;
    bool save_gates;        // `gates` is written (the small tail keeps V, U there)
    int keep;               // MIL_ROUTE_BITS_NONE, _GIVEN, or _GENERATOR for "to be drawn" (the plan says where)
    bool pieces;            // weight pieces Wp given
    bool fused_pool;        // the caller wants the pool partial pass in the epilogue and its tile map is all full, aligned tiles
    // ---- what the deferred pool asks beyond that (all zero: never; mil_gate_step_route knows none of it)
    bool defer_hint;        // MIL_STAGE_POOL_DEFERRED came with the call: aligned single-segment layout, M valid at the end of the step
    bool fp32, labels, hrow, host_lengths;      // x is fp32; y, hrow given; no bag_len_dev / rows_dev
    int C, T, B;
    int chunk_bags;         // most bags a row chunk of the weight gradient touches, 0: unknown
    bool mpart;             // workspace given ...
    uint64_t mpart_floats;  // ... of this size
};
// MIL_POOL_DEFERRED=0 turns the deferred pool off; read per call (under a hipGraph: at capture), as MIL_DW_PIECES is
static inline bool pool_deferred_enabled() {
    const char* e = getenv("MIL_POOL_DEFERRED");
    return e == nullptr || atoi(e) != 0;
}
// rows beyond whole rounds of 128-row tiles that fit the few-rows kernels (shared with the input gradient, gate_bwd_dx.hip)
int gate_tail_rows(int R, int tiles_per_round) {
    const int tail = R % GF_TM, full = R / GF_TM;
    return (tail >= 1 && tail <= MIL_SMALL_ROWS && full >= tiles_per_round && full % tiles_per_round == 0) ? tail : 0;
}
static inline int gate_r32_rt(int rows, int ncu) {
    const int tiles = (rows + GS_TM - 1) / GS_TM;
    return tiles <= ncu ? 1 : tiles <= 2 * ncu ? 2 : 3;
}
static mil_gate_route gate_route_plan(const GateRouteIn& in, int ncu) {
    const int R = in.R, L = in.L;
    mil_gate_route p{};
    // fewer 128-row tiles than 3/4 of the CUs: 32-row tiles (4x the workgroups, each a quarter of the time), RT of them per
    // workgroup - the smallest count that covers the rows in one round of one-workgroup-per-CU launches
    const bool r32 = (R + GF_TM - 1) / GF_TM < (3 * ncu) / 4;
    const bool fwd2 = L <= 4096;                 // 128 rows x L floats must stay inside the 32-bit buffer offsets (and int math)
    p.main = r32 ? MIL_ROUTE_MAIN_R32 : !fwd2 ? MIL_ROUTE_MAIN_LEGACY : in.pieces ? MIL_ROUTE_MAIN_FWD2_PW : MIL_ROUTE_MAIN_FWD2;
    p.rt = r32 ? gate_r32_rt(R, ncu) : 0;
    if (!r32) {
        // Tile quantisation: with one 128-row workgroup per CU, R = k * ncu * 128 + (a few rows) costs a whole extra round
        // of the grid for one workgroup (config 3: 32 bags x (1024 patches + 2 tokens) = 256.5 tiles -> 2x the kernel time).
        // When the rows beyond a whole number of rounds fit the few-rows linear (<= 64), they take that path instead.
        // Otherwise a last round that would hold only a few workgroups (T text tokens per bag appended to 32 x 1024 patches:
        // 259 tiles on 256 CUs): every row beyond the whole rounds, up to 1024 of them, goes through the 32-row kernel
        // (10 workgroups of a quarter of the time)
        const int few = in.save_gates ? gate_tail_rows(R, ncu) : 0, per_round = GF_TM * ncu, over = R % per_round;
        if (few > 0) {
            p.tail = MIL_ROUTE_TAIL_SMALL;
            p.tail_rows = few;
        } else if (R >= per_round && over > 0 && over <= 1024) {
            p.tail = MIL_ROUTE_TAIL_BIG;
            p.tail_rows = over;
        }
    }
    if (p.tail != MIL_ROUTE_TAIL_NONE) {
        // the 32-row kernel applies the keep bits while staging; the few-rows linear has no such input
        const bool small_linear = p.tail == MIL_ROUTE_TAIL_SMALL && in.keep == MIL_ROUTE_BITS_NONE;
        p.tail_kernel = small_linear ? MIL_ROUTE_TAIL_KERNEL_LINEAR_SMALL : MIL_ROUTE_TAIL_KERNEL_R32;
        p.tail_rt = small_linear ? 0 : gate_r32_rt(p.tail_rows, ncu);
    }
    const bool all_fwd2 = !r32 && p.tail == MIL_ROUTE_TAIL_NONE && fwd2;        // every row goes through k_gate_fwd2
    // the forward kernel can draw the keep bits itself when a workgroup's [128][L/32] words fit its LDS slot; otherwise the
    // stand-alone generator runs first
    p.bits = in.keep == MIL_ROUTE_BITS_NONE || in.keep == MIL_ROUTE_BITS_GIVEN ? in.keep
             : all_fwd2 && L <= 1024 && (L % 128) == 0 ? MIL_ROUTE_BITS_IN_KERNEL : MIL_ROUTE_BITS_GENERATOR;
    p.pool_fused = in.fused_pool && all_fwd2 && L == 512 && (R % 32) == 0;      // the pool partial pass in the epilogue
    p.dw = -1;
    if ((L % 128) == 0) {
        const GateDwPlan d = gate_dw_plan(R, L, ncu);
        p.dw = d.dw;
        p.S = d.S;
        p.kc = d.kc;
    }
    // The deferred pool: no pool pass over x.  hrow comes out of the split-bf16 K loop (every row on k_gate_fwd2<.., PW, HR>,
    // head rows of L = GF_HR_MAXL in LDS, C == 2: one column per wave of a row tile), the row weights out of k_pool_tail_h's
    // chain half (not the few-long-bags tail of mil_pool_merge_head_ws, not MIL_TAIL_H=0), the M sums out of the m == 0
    // workgroups of k_gate_bwd_dw2_pieces (whole 32-row slices inside one bag, at most MP_SLOTS bags per row chunk), M, Mdrop
    // and dWf out of the fold.
    const char* tail_env = getenv("MIL_TAIL_H");
    p.pool_deferred = in.defer_hint && pool_deferred_enabled() && in.fp32 && p.main == MIL_ROUTE_MAIN_FWD2_PW && all_fwd2 &&
                      L == GF_HR_MAXL && in.C == 2 && in.labels && in.hrow && in.host_lengths && in.T * MIL_POOL_TILE == R &&
                      !(in.T >= 64 * in.B && in.B <= 8) && !(tail_env != nullptr && tail_env[0] == '0') &&
                      p.dw == MIL_ROUTE_DW2 && gate_dw_pieces_on() && in.chunk_bags >= 1 &&
                      in.chunk_bags <= MIL_POOL_DEFERRED_SLOTS && in.mpart &&
                      in.mpart_floats >= (uint64_t)p.S * MIL_POOL_DEFERRED_SLOTS * 16 * L;
    if (p.pool_deferred) p.pool_fused = 0;
    return p;
}

// The step descriptor as the plan reads it: the one place that turns mil_image_only_step + stage mask into a GateRouteIn
mil_gate_route gate_step_plan(const mil_image_only_step* a, uint32_t st, int ncu) {
    const bool train = a->train != 0, grads = a->y != nullptr, fp32 = !a->x_bf16;
    const bool draw = (st & MIL_STAGE_DROPBITS) && (st & MIL_STAGE_GATE_FWD) && train && fp32;
    const bool use_h = a->hrow != nullptr && grads && a->C <= 4;
    GateRouteIn in{};
    in.R = a->R;
    in.L = a->L;
    in.save_gates = grads;
    in.keep = !train ? MIL_ROUTE_BITS_NONE : draw ? MIL_ROUTE_BITS_GENERATOR : MIL_ROUTE_BITS_GIVEN;
    in.pieces = fp32 && a->Wp != nullptr;
    in.fused_pool = fp32 && (st & MIL_STAGE_GATE_FWD) && (st & MIL_STAGE_POOL) && (st & MIL_STAGE_POOL_FUSED) && use_h && a->C == 2 &&
                    !a->bag_len_dev && (!train || draw) && fuse_pool_enabled() && a->T * MIL_POOL_TILE == a->R;
    in.defer_hint = (st & MIL_STAGE_POOL_DEFERRED) != 0;
    in.fp32 = fp32;
    in.labels = grads;
    in.hrow = a->hrow != nullptr;
    in.host_lengths = !a->bag_len_dev && !a->rows_dev;
    in.C = a->C;
    in.T = a->T;
    in.B = a->B;
    in.chunk_bags = a->dw_chunk_bags;
    in.mpart = a->mpart != nullptr;
    in.mpart_floats = a->mpart_floats;
    return gate_route_plan(in, ncu > 0 ? ncu : MIL_NUM_CU);
}

extern "C" int mil_image_only_step_route(const mil_image_only_step* a, uint32_t stages, int ncu, mil_gate_route* out) {
    if (!a || !out || a->struct_bytes != sizeof(mil_image_only_step)) return MIL_EINVAL;       // bf16 x: never deferred
    if (a->R <= 0 || a->L <= 0 || (a->L % GF_BK) != 0 || a->C <= 0) return MIL_EINVAL;
    *out = gate_step_plan(a, stages, ncu);
    return MIL_OK;
}

// C and bucketed describe the step for the caller's benefit; the plan does not depend on them (whether the fused pool is
// asked for at all - C == 2, not bucketed, the stage bits - is the caller's rule, mil_image_only_step_run's in step.hip)
extern "C" int mil_gate_step_route(int R, int L, int C, int save_gates, int keep, int pieces, int fused_pool, int bucketed,
                                   int ncu, mil_gate_route* out) {
    if (!out || R <= 0 || L <= 0 || (L % GF_BK) != 0 || C <= 0) return MIL_EINVAL;
    if (keep != MIL_ROUTE_BITS_NONE && keep != MIL_ROUTE_BITS_GIVEN) keep = MIL_ROUTE_BITS_GENERATOR;
    (void)bucketed;
    GateRouteIn in{};
    in.R = R;
    in.L = L;
    in.save_gates = save_gates != 0;
    in.keep = keep;
    in.pieces = pieces != 0;
    in.fused_pool = fused_pool != 0;
    *out = gate_route_plan(in, ncu > 0 ? ncu : MIL_NUM_CU);
    return MIL_OK;
}

// ---- the launch tables: every instantiation of the forward kernels is named here and nowhere else
using GateFwdR32Kernel = decltype(&k_gate_fwd_r32<false, 1>);
static const GateFwdR32Kernel GATE_FWD_R32_KERNELS[2][3] = {                    // [keep bits][RT - 1]
    {k_gate_fwd_r32<false, 1>, k_gate_fwd_r32<false, 2>, k_gate_fwd_r32<false, 3>},
    {k_gate_fwd_r32<true, 1>, k_gate_fwd_r32<true, 2>, k_gate_fwd_r32<true, 3>}};
using GateFwd2Kernel = decltype(&k_gate_fwd2<false, false, 0, false>);
static const GateFwd2Kernel GATE_FWD2_KERNELS[3][2][2] = {                      // [none / bits given / drawn (GEN)][pool fused][PW]
    {{k_gate_fwd2<false, false, 0, false>, k_gate_fwd2<false, false, 0, true>}, {k_gate_fwd2<false, false, 2, false>, k_gate_fwd2<false, false, 2, true>}},
    {{k_gate_fwd2<true, false, 0, false>, k_gate_fwd2<true, false, 0, true>}, {k_gate_fwd2<true, false, 2, false>, k_gate_fwd2<true, false, 2, true>}},
    {{k_gate_fwd2<true, true, 0, false>, k_gate_fwd2<true, true, 0, true>}, {k_gate_fwd2<true, true, 2, false>, k_gate_fwd2<true, true, 2, true>}}};

// ... with the head projections from the split-bf16 K loop and no pool pass (the deferred pool)
static const GateFwd2Kernel GATE_FWD2_HROW_KERNELS[3] = {                       // [none / bits given / drawn (GEN)]
    k_gate_fwd2<false, false, 0, true, true>, k_gate_fwd2<true, false, 0, true, true>, k_gate_fwd2<true, true, 0, true, true>};

static int launch_gate_fwd_r32(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu,
                               const float* w, const float* b, float* scores, float* gates, int R, int L,
                               const uint32_t* xbits, float xscale, int rt, hipStream_t st, const int32_t* rows_dev = nullptr) {
    const dim3 grid((R + GS_TM * rt - 1) / (GS_TM * rt));
    const float xs = xbits ? xscale : 1.0f;
    hipLaunchKernelGGL(GATE_FWD_R32_KERNELS[xbits != nullptr][rt <= 1 ? 0 : rt == 2 ? 1 : 2], grid, dim3(GS_THREADS), 0, st, x, Wv, bv, Wu, bu, w, b, scores,
                       gates, R, L, xbits, xs, rows_dev);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
// the 128-row tiles of k_gate_fwd2; Wp only with pw
static void launch_gate_fwd2(bool draw, bool pool_fused, bool pw, dim3 grid, hipStream_t st, const float* x, const float* Wv,
                             const float* bv, const float* Wu, const float* bu, const float* w, const float* b, float* scores,
                             float* gates, int R, int L, const uint32_t* xbits, float xs, const GateFwdGen& gen,
                             const GateFwdPool& pool, const uint16_t* Wp) {
    hipLaunchKernelGGL(GATE_FWD2_KERNELS[draw ? 2 : xbits ? 1 : 0][pool_fused][pw], grid, dim3(512), 0, st, x, Wv, bv, Wu, bu, w, b,
                       scores, gates, R, L, xbits, xs, gen, pool, pw ? (const unsigned short*)Wp : nullptr);
}

// gen: the keep bits are drawn by this call (in the forward kernel or by a generator launch in front of it: the plan
// says which), else xbits (nullable) are given.  pool + fused: the caller wants the pool partial pass in the epilogue;
// *fused says whether it ran there.  tmap: the step's tile map is still to be built (it writes rows_dev, which the
// forward reads): it rides on the generator launch where there is one, and is a launch of its own in front of the
// forward otherwise.  Wp (three-piece bf16 planes of [Wv; Wu], gp_index layout): the split-bf16 K loop of k_gate_fwd2.
static int gate_scores_fwd_impl(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu,
                                const float* w, const float* b, float* scores, float* gates, int R, int L, int D,
                                const uint32_t* xbits, float xscale, const GateFwdGen* gen, void* stream,
                                const GateFwdPool* pool = nullptr, int* fused = nullptr, const int32_t* rows_dev = nullptr,
                                const TileMapJob* tmap = nullptr, const uint16_t* Wp = nullptr) {
    if (!x || !Wv || !bv || !Wu || !bu || !w || !b || !scores) return MIL_EINVAL;
    if (D != MIL_GATE_D || L <= 0 || (L % GF_BK) != 0 || R < 0) return MIL_EINVAL;
    if (R == 0) return MIL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (fused != nullptr) *fused = 0;
    // the fused pool pass needs every tile of the map full and aligned (T * 32 == R: tile t = rows 32 t ..) and the head's
    // keep words where the patch rows have theirs
    const bool pool_ok = pool != nullptr && fused != nullptr && pool->T * MIL_POOL_TILE == R && pool->tile_map &&
                         pool->partials && pool->Wf && pool->hrow &&
                         (gen ? gen->mbits_out != nullptr : (xbits != nullptr) == (pool->mbits != nullptr));
    const int keep = gen ? MIL_ROUTE_BITS_GENERATOR : xbits ? MIL_ROUTE_BITS_GIVEN : MIL_ROUTE_BITS_NONE;
    GateRouteIn in{};
    in.R = R;
    in.L = L;
    in.save_gates = gates != nullptr;
    in.keep = keep;
    in.pieces = Wp != nullptr;
    in.fused_pool = pool_ok;
    const mil_gate_route p = gate_route_plan(in, MIL_NUM_CU);

    int rc = MIL_OK;
    if (p.bits == MIL_ROUTE_BITS_GENERATOR) {
        const uint64_t seed = ((uint64_t)gen->seed_hi << 32) | gen->seed_lo, mseed = ((uint64_t)gen->mseed_hi << 32) | gen->mseed_lo;
        if (gen->mbits_out != nullptr && tmap != nullptr) {
            rc = dropout_keep_bits_pair_tilemap(gen->xbits_out, R, gen->mbits_out, gen->B, L, seed, mseed, gen->offset,
                                                gen->offset_dev, *tmap, stream);
            tmap = nullptr;
        } else if (gen->mbits_out != nullptr)
            rc = dropout_keep_bits_pair(gen->xbits_out, R, gen->mbits_out, gen->B, L, seed, mseed, gen->offset, gen->offset_dev, stream);
        else
            rc = mil_dropout_keep_bits(gen->xbits_out, R, L, 0.5f, seed, gen->offset, gen->offset_dev, stream);
        if (rc != MIL_OK) return rc;
        xbits = gen->xbits_out;
    }
    if (tmap != nullptr) {
        rc = mil_build_tile_map(tmap->bag_len, tmap->B, tmap->tile_map, tmap->bag_tile_off, tmap->rows_out, tmap->T_cap, stream);
        if (rc != MIL_OK) return rc;
    }
    if (p.main == MIL_ROUTE_MAIN_R32)
        return launch_gate_fwd_r32(x, Wv, bv, Wu, bu, w, b, scores, gates, R, L, xbits, xscale, p.rt, st, rows_dev);

    const bool draw = p.bits == MIL_ROUTE_BITS_IN_KERNEL;
    if (draw) xbits = gen->xbits_out;
    const int Rm = R - p.tail_rows;
    const dim3 grid((Rm + GF_TM - 1) / GF_TM);
    const float xs = xbits ? xscale : 1.0f;
    if (p.main == MIL_ROUTE_MAIN_LEGACY) {
        hipLaunchKernelGGL(xbits ? k_gate_fwd<true> : k_gate_fwd<false>, grid, dim3(512), 0, st, x, Wv, bv, Wu, bu, w, b, scores, gates,
                           Rm, L, xbits, xs);
    } else {
        const GateFwdGen fgen = draw ? *gen : GateFwdGen{};
        const GateFwdPool fpool = p.pool_fused ? *pool : GateFwdPool{};
        launch_gate_fwd2(draw, p.pool_fused, p.main == MIL_ROUTE_MAIN_FWD2_PW, grid, st, x, Wv, bv, Wu, bu, w, b, scores, gates, Rm, L,
                         xbits, xs, fgen, fpool, Wp);
    }
    if (p.pool_fused) *fused = 1;
    MIL_CHECK_LAUNCH();
    if (p.tail_kernel == MIL_ROUTE_TAIL_KERNEL_R32)
        return launch_gate_fwd_r32(x + (size_t)Rm * L, Wv, bv, Wu, bu, w, b, scores + Rm,
                                   gates ? gates + (size_t)Rm * GF_NG : nullptr, p.tail_rows, L,
                                   xbits ? xbits + (size_t)Rm * (L / 32) : nullptr, xscale, p.tail_rt, st);
    if (p.tail_kernel == MIL_ROUTE_TAIL_KERNEL_LINEAR_SMALL) {
        // V and U through mil_linear_small_fwd straight into the gates buffer, then one tiny scoring launch
        const float* xt = x + (size_t)Rm * L;
        float* gt = gates + (size_t)Rm * GF_NG;
        rc = mil_linear_small_fwd(xt, L, Wv, L, bv, 1 /* tanh */, nullptr, 0, gt, GF_NG, p.tail_rows, MIL_GATE_D, L, stream);
        if (rc != MIL_OK) return rc;
        rc = mil_linear_small_fwd(xt, L, Wu, L, bu, 4 /* sigmoid */, nullptr, 0, gt + MIL_GATE_D, GF_NG, p.tail_rows, MIL_GATE_D, L,
                                  stream);
        if (rc != MIL_OK) return rc;
        hipLaunchKernelGGL(k_gate_tail_scores, dim3(p.tail_rows), dim3(64), 0, st, gt, w, b, scores + Rm);
        MIL_CHECK_LAUNCH();
    }
    return MIL_OK;
}

extern "C" int mil_gate_scores_fwd(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu,
                                   const float* w, const float* b, float* scores, float* gates, int R, int L, int D,
                                   const uint32_t* xbits, float xscale, void* stream) {
    return gate_scores_fwd_impl(x, Wv, bv, Wu, bu, w, b, scores, gates, R, L, D, xbits, xscale, nullptr, stream);
}

static GateFwdGen gate_fwd_gen(uint32_t* xbits_out, uint32_t* mbits_out, int B, uint64_t seed, uint64_t mseed, uint64_t offset,
                               const int32_t* offset_dev) {
    GateFwdGen g{};
    g.xbits_out = xbits_out;
    g.mbits_out = mbits_out;
    g.B = B;
    g.seed_lo = (uint32_t)seed;
    g.seed_hi = (uint32_t)(seed >> 32);
    g.mseed_lo = (uint32_t)mseed;
    g.mseed_hi = (uint32_t)(mseed >> 32);
    g.offset = offset;
    g.offset_dev = offset_dev;
    return g;
}

extern "C" int mil_gate_scores_fwd_draw(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu,
                                        const float* w, const float* b, float* scores, float* gates, int R, int L, int D,
                                        uint32_t* xbits_out, float xscale, uint32_t* mbits_out, int B, uint64_t seed,
                                        uint64_t mseed, uint64_t offset, const int32_t* offset_dev, void* stream) {
    if (!xbits_out || (L % 64) != 0 || (mbits_out && B <= 0)) return MIL_EINVAL;
    const GateFwdGen gen = gate_fwd_gen(xbits_out, mbits_out, B, seed, mseed, offset, offset_dev);
    return gate_scores_fwd_impl(x, Wv, bv, Wu, bu, w, b, scores, gates, R, L, D, nullptr, xscale, &gen, stream);
}

int gate_fwd_rows_dev(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu, const float* w,
                      const float* b, float* scores, float* gates, int R, int L, int draw, uint32_t* xbits, float xscale,
                      uint32_t* mbits, int B, uint64_t seed, uint64_t mseed, uint64_t offset, const int32_t* offset_dev,
                      const int32_t* rows_dev, void* stream, const TileMapJob* tmap, const uint16_t* Wp) {
    if (draw && (!xbits || (L % 64) != 0 || (mbits && B <= 0))) return MIL_EINVAL;
    const GateFwdGen gen = gate_fwd_gen(xbits, mbits, B, seed, mseed, offset, offset_dev);
    return gate_scores_fwd_impl(x, Wv, bv, Wu, bu, w, b, scores, gates, R, L, MIL_GATE_D, draw ? nullptr : xbits, xscale,
                                draw ? &gen : nullptr, stream, nullptr, nullptr, rows_dev, tmap, Wp);
}

int gate_fwd_with_pool(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu, const float* w,
                       const float* b, float* scores, float* gates, int R, int L, int draw, uint32_t* xbits, float xscale,
                       uint32_t* mbits, float mscale, int B, uint64_t seed, uint64_t mseed, uint64_t offset,
                       const int32_t* offset_dev, const int32_t* tile_map, int T, float* partials, const float* Wf, float* hrow,
                       int* fused, void* stream, const uint16_t* Wp) {
    if (draw && (!xbits || !mbits || (L % 64) != 0 || B <= 0)) return MIL_EINVAL;
    GateFwdPool pl{};
    pl.tile_map = tile_map;
    pl.partials = partials;
    pl.T = T;
    pl.Wf = Wf;
    pl.hrow = hrow;
    pl.mbits = draw ? nullptr : mbits;
    pl.mscale = mscale;
    const GateFwdGen gen = gate_fwd_gen(xbits, mbits, B, seed, mseed, offset, offset_dev);
    return gate_scores_fwd_impl(x, Wv, bv, Wu, bu, w, b, scores, gates, R, L, MIL_GATE_D, draw ? nullptr : xbits, xscale,
                                draw ? &gen : nullptr, stream, &pl, fused, nullptr, nullptr, Wp);
}

int gate_fwd_deferred(const mil_image_only_step* a, const mil_gate_route& p, bool draw, float xscale, float mscale, void* stream) {
    if (!p.pool_deferred || p.main != MIL_ROUTE_MAIN_FWD2_PW || p.tail != MIL_ROUTE_TAIL_NONE || !a->Wp || !a->hrow || !a->gates)
        return MIL_EINVAL;
    if (draw && (p.bits != MIL_ROUTE_BITS_IN_KERNEL || !a->xbits || !a->mbits)) return MIL_EINVAL;
    if (a->L != GF_HR_MAXL || a->C != 2 || a->T * MIL_POOL_TILE != a->R || !a->tile_map) return MIL_EINVAL;      // the kernel's LDS and tile bounds
    const bool train = a->train != 0;
    if (train && (!a->xbits || !a->mbits)) return MIL_EINVAL;
    GateFwdPool pl{};
    pl.tile_map = a->tile_map;
    pl.T = a->T;
    pl.Wf = a->Wf;
    pl.hrow = a->hrow;
    pl.mbits = train && !draw ? a->mbits : nullptr;
    pl.mscale = mscale;
    const GateFwdGen gen = draw ? gate_fwd_gen(a->xbits, a->mbits, a->B, a->seed, a->seed ^ 0x9E3779B97F4A7C15ull, a->offset, a->offset_dev)
                                : GateFwdGen{};
    const uint32_t* xbits = train ? a->xbits : nullptr;
    hipLaunchKernelGGL(GATE_FWD2_HROW_KERNELS[draw ? 2 : train ? 1 : 0], dim3((a->R + GF_TM - 1) / GF_TM), dim3(512), 0,
                       (hipStream_t)stream, (const float*)a->x, a->Wv, a->bv, a->Wu, a->bu, a->w, a->b, a->scores, a->gates, a->R, a->L,
                       xbits, train ? xscale : 1.0f, gen, pl, (const unsigned short*)a->Wp);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// The three-piece bf16 planes of [Wv; Wu] the split-bf16 gate forward reads (gp_index layout, 3 * 384 * L halves), formed
// from the fp32 masters.  The one-call step keeps them current itself after every update it applies; a caller that
// writes the parameters another way calls this once afterwards.
__global__ __launch_bounds__(256) void k_gate_pieces(const float* __restrict__ Wv, const float* __restrict__ Wu,
                                                     unsigned short* __restrict__ Wp, int L) {
    const int L4 = L / 4;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= GF_NG * L4) return;
    const int n = idx / L4, k = 4 * (idx % L4);
    const float* src = (n < MIL_GATE_D ? Wv + (size_t)n * L : Wu + (size_t)(n - MIL_GATE_D) * L) + k;
    gp_store4(Wp, n, k, *reinterpret_cast<const f32x4*>(src));
}

extern "C" int mil_gate_pieces(const float* Wv, const float* Wu, uint16_t* Wp, int L, void* stream) {
    if (!Wv || !Wu || !Wp || L <= 0 || (L % 32) != 0) return MIL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(Wv) | reinterpret_cast<uintptr_t>(Wu) | reinterpret_cast<uintptr_t>(Wp)) & 15) return MIL_EINVAL;
    hipLaunchKernelGGL(k_gate_pieces, dim3((GF_NG * (L / 4) + 255) / 256), dim3(256), 0, (hipStream_t)stream, Wv, Wu,
                       (unsigned short*)Wp, L);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
