// TransMIL: the batched product of csrc/transmil.hip (k_tm_bgemm) on three-piece split-bf16 MFMA, opt-in
// (ops: pieces=3 / MIL_TM_PIECES=3).  Same operation, same strides, same epilogue and split-K forms:
//   C[b] = alpha A[b] B[b] + beta D[b] + diag I, element (i, k) of A[b] at A + b sAb + i sAi + k sAk (likewise B, C),
// with the per-head operands read in place from merged rows and the results written in place into merged-head rows.
//
// Arithmetic.  Every staged fp32 element a of A and b of B is split on its way from registers to LDS into three bf16 pieces,
// a = a0 + a1 + a2 exactly (gp_split3), and the contraction runs on v_mfma_f32_32x32x16_bf16 over the six cross terms
// (p, q) with p + q <= 2, issued smallest first into one fp32 accumulator, as the gate forward's split-bf16 K loop does
// (csrc/gate_fwd.hip); the dropped terms a1 b2, a2 b1, a2 b2 are below 2^-24 relative.  Per 16 k and 32 x 32 tile that is
// six MFMAs of 32 cycles where v_mfma_f32_32x32x2_f32 takes 512.  The chain folds into a second accumulator every 512 of
// K, as k_tm_bgemm's does.  No operand is pre-split in HBM.
// Non-finite inputs give non-finite outputs, not necessarily of the same kind: gp_split3 adds no NaN of its own (an
// infinite element keeps p0 = the infinity, p1 = p2 = 0), but an infinity times a zero piece of the other operand is a NaN
// where the fp32 kernel gives an infinity.  The Nystrom core's operands are finite.
//
// Tiles.  TM x 64 per workgroup of 2 x 2 waves, TM = 64 (one accumulator per wave; the same grid as k_tm_bgemm, so the
// pseudo-inverse's 256^3 products keep their 128 workgroups) or 128 (two accumulators per wave down the rows: a split
// element of B feeds two MFMA rows of every wave that reads it, and each thread splits 24 elements per 24 MFMAs of its
// wave where the 64-row form splits 16 per 12).  K goes 32 at a time through a double-buffered LDS image (one barrier
// per slice); the next slice's elements are loaded into registers in front of the current slice's MFMAs and split behind
// them.  A thread stages (row, 8 consecutive k): one 16-byte LDS store per piece.  LDS image of an operand, per buffer:
// [piece][k / 8][row][8] bf16 - the fragment of MFMA step s is k group 2 s + (lane >> 5), row lane & 31, so the two lane
// halves each read 512 contiguous bytes (conflict-free ds_read_b128).  2 x (TM + 64) x 32 x 6 bytes = 48 / 72 KiB.
// Rows, columns and k outside the problem stage as zero; the stores are guarded (tm_bgemm.h).
#include <hip/hip_runtime.h>

#include "mil_common.h"
#include "tm_bgemm.h"
#include "../../include/mil_hip.h"

namespace {

constexpr int BP_BK = 32, BP_KG = BP_BK / 8, BP_FOLD = BG_FOLD_K / BP_BK, BP_TN = 64;

// the pieces of 8 consecutive k of one row into image `img` ([PIECES][BP_KG][ROWS][8] bf16)
template <int PIECES, int ROWS>
__device__ __forceinline__ void bp_put8(unsigned short* img, int row, int kg, const float (&v)[8]) {
    gp_bf16x8 o[3];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned short p0, p1, p2;
        gp_split3(v[j], p0, p1, p2);
        o[0][j] = __builtin_bit_cast(__bf16, p0);
        o[1][j] = __builtin_bit_cast(__bf16, p1);
        o[2][j] = __builtin_bit_cast(__bf16, p2);
    }
#pragma unroll
    for (int q = 0; q < PIECES; ++q) *reinterpret_cast<gp_bf16x8*>(img + ((size_t)(q * BP_KG + kg) * ROWS + row) * 8) = o[q];
}

// blockIdx.z = batch * splits + split, split p takes the 32-deep K slices [p per, (p + 1) per), per = ceil(slices / splits);
// FIXED as k_tm_bgemm<true> (plain stores of alpha x the partial tile into ws[p][batch][M][N], zeros for an empty split).
template <int TM, int PIECES, bool FIXED>
__global__ __launch_bounds__(256) void k_tm_bgemm_pieces(const float* __restrict__ A, long sAb, long sAi, long sAk,
                                                         const float* __restrict__ B, long sBb, long sBk, long sBj, float* C,
                                                         long sCb, long sCi, long sCj, const float* D, int M, int N, int K,
                                                         float alpha, float beta, float diag, int splits) {
    static_assert(PIECES == 3, "two-piece products are not built yet: the term table below is the three-piece one");
    static_assert(TM == 64 || TM == 128, "2 x 2 waves of TM / 64 accumulators each");
    constexpr int RM = TM / 64, NA = TM * BP_BK / 8 / 256, NB = BP_TN * BP_BK / 8 / 256;      // row tiles per wave; (row, k group) jobs per thread
    constexpr int A_IMG = PIECES * BP_KG * TM * 8, B_IMG = PIECES * BP_KG * BP_TN * 8;          // bf16 elements
    __shared__ __attribute__((aligned(16))) unsigned short sa[2][A_IMG];
    __shared__ __attribute__((aligned(16))) unsigned short sb[2][B_IMG];
    const int bz = blockIdx.z / splits, split = blockIdx.z % splits;
    const int i0 = blockIdx.y * TM, j0 = blockIdx.x * BP_TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, r = lane & 31, h = lane >> 5;
    A += (long)bz * sAb;
    B += (long)bz * sBb;
    C += (long)bz * sCb;
    if (D != nullptr) D += (long)bz * sCb;
    const int kslices = (K + BP_BK - 1) / BP_BK;
    const int per = (kslices + splits - 1) / splits;
    const int s0 = split * per, s1 = min(kslices, s0 + per);
    // a thread's job is (row, k group): the lanes run along k when k is contiguous in memory, along the rows otherwise
    const bool a_krow = sAk == 1, b_krow = sBk == 1;

    float ra[NA][8], rb[NB][8];
    auto load = [&](int ks) {
        const int k0 = ks * BP_BK;
#pragma unroll
        for (int p = 0; p < NA; ++p) {
            const int e = tid + 256 * p;
            const int row = a_krow ? e / BP_KG : e % TM, kg = a_krow ? e % BP_KG : e / TM;
            const int gi = i0 + row;
            const float* src = A + gi * sAi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gk = k0 + 8 * kg + j;
                ra[p][j] = (gi < M && gk < K) ? src[gk * sAk] : 0.f;
            }
        }
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            const int e = tid + 256 * p;
            const int col = b_krow ? e / BP_KG : e % BP_TN, kg = b_krow ? e % BP_KG : e / BP_TN;
            const int gj = j0 + col;
            const float* src = B + gj * sBj;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gk = k0 + 8 * kg + j;
                rb[p][j] = (gj < N && gk < K) ? src[gk * sBk] : 0.f;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < NA; ++p) {
            const int e = tid + 256 * p;
            bp_put8<PIECES, TM>(sa[buf], a_krow ? e / BP_KG : e % TM, a_krow ? e % BP_KG : e / TM, ra[p]);
        }
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            const int e = tid + 256 * p;
            bp_put8<PIECES, BP_TN>(sb[buf], b_krow ? e / BP_KG : e % BP_TN, b_krow ? e % BP_KG : e / BP_TN, rb[p]);
        }
    };

    f32x16 acc[RM], tot[RM];
#pragma unroll
    for (int m = 0; m < RM; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] = tot[m][i] = 0.f;
    if (s0 < s1) {
        load(s0);
        store(0);
    }
    __syncthreads();
    for (int ks = s0; ks < s1; ++ks) {
        const int buf = (ks - s0) & 1;
        const bool more = ks + 1 < s1;
        if (more) load(ks + 1);
#pragma unroll
        for (int s = 0; s < BP_BK / 16; ++s) {
            gp_bf16x8 ap[RM][PIECES], bp[PIECES];
#pragma unroll
            for (int q = 0; q < PIECES; ++q) {
                bp[q] = *reinterpret_cast<const gp_bf16x8*>(&sb[buf][((size_t)(q * BP_KG + 2 * s + h) * BP_TN + 32 * wj + r) * 8]);
#pragma unroll
                for (int m = 0; m < RM; ++m)
                    ap[m][q] = *reinterpret_cast<const gp_bf16x8*>(
                        &sa[buf][((size_t)(q * BP_KG + 2 * s + h) * TM + (TM / 2) * wi + 32 * m + r) * 8]);
            }
            // cross terms (p, q), p + q <= 2, smallest first
            constexpr int TP[6] = {0, 1, 2, 0, 1, 0}, TQ[6] = {2, 1, 0, 1, 0, 0};
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int m = 0; m < RM; ++m)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[m][TP[t]], bp[TQ[t]], acc[m], 0, 0, 0);
        }
        if (((ks - s0) & (BP_FOLD - 1)) == BP_FOLD - 1) {
#pragma unroll
            for (int m = 0; m < RM; ++m)
#pragma unroll
                for (int i = 0; i < 16; ++i) { tot[m][i] += acc[m][i]; acc[m][i] = 0.f; }
        }
        // the other buffer was last read in front of the barrier that ended the slice before this one
        if (more) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < RM; ++m) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][i] += tot[m][i];
        tm_bgemm_store<FIXED>(acc[m], C, sCi, sCj, D, M, N, i0 + (TM / 2) * wi + 32 * m, j0 + 32 * wj + r, h, alpha, beta, diag,
                              splits, split);
    }
}

// The one launch table: the tile form from (M, N, batch).  128 rows for the products whose M is the bag (M > 256: O = A1 U,
// dq, dk, dv, and the whole-map products of need_attn True); every product of the 256 landmarks - the pseudo-inverse
// chain, W, U, the landmark gradients - keeps the 64 x 64 grid of k_tm_bgemm, which at batch 8 is 128 workgroups x splits
// where 128-row tiles would leave 64.
inline int bp_tile_m(int M, int N, int batch) {
    (void)N;
    (void)batch;
    return M > 256 ? 128 : 64;
}

template <bool FIXED>
inline void bp_launch(int tile_m, dim3 grid, hipStream_t stream, const float* A, long sAb, long sAi, long sAk, const float* B, long sBb,
                      long sBk, long sBj, float* C, long sCb, long sCi, long sCj, const float* D, int M, int N, int K, float alpha,
                      float beta, float diag, int splits) {
    if (tile_m == 128)
        hipLaunchKernelGGL((k_tm_bgemm_pieces<128, 3, FIXED>), grid, dim3(256), 0, stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb,
                           sCi, sCj, D, M, N, K, alpha, beta, diag, splits);
    else
        hipLaunchKernelGGL((k_tm_bgemm_pieces<64, 3, FIXED>), grid, dim3(256), 0, stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb,
                           sCi, sCj, D, M, N, K, alpha, beta, diag, splits);
}

inline int launch_rc() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MIL_OK : (int)e;
}

}  // namespace

extern "C" {

int mil_tm_bgemm_pieces(const float* A, long sAb, long sAi, long sAk, const float* B, long sBb, long sBk, long sBj, float* C,
                        long sCb, long sCi, long sCj, const float* D, int batch, int M, int N, int K, float alpha, float beta,
                        float diag, int splits, int pieces, void* stream) {
    if (pieces != 3) return MIL_EINVAL;
    const int tm = bp_tile_m(M, N, batch);
    if (!tm_bgemm_args_ok(A, B, C, batch, M, N, K, splits, tm) || !tm_bgemm_atomic_ok(beta, D, splits)) return MIL_EINVAL;
    dim3 grid((N + BP_TN - 1) / BP_TN, (M + tm - 1) / tm, batch * splits);
    bp_launch<false>(tm, grid, (hipStream_t)stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb, sCi, sCj, D, M, N, K, alpha, beta,
                     diag, splits);
    return launch_rc();
}

int mil_tm_bgemm_pieces_fixed(const float* A, long sAb, long sAi, long sAk, const float* B, long sBb, long sBk, long sBj, float* C,
                              long sCb, long sCi, long sCj, const float* D, int batch, int M, int N, int K, float alpha, float beta,
                              float diag, int splits, int pieces, float* ws, void* stream) {
    if (splits == 1)
        return mil_tm_bgemm_pieces(A, sAb, sAi, sAk, B, sBb, sBk, sBj, C, sCb, sCi, sCj, D, batch, M, N, K, alpha, beta, diag, 1,
                                   pieces, stream);
    if (pieces != 3) return MIL_EINVAL;
    const int tm = bp_tile_m(M, N, batch);
    if (!ws || !tm_bgemm_args_ok(A, B, C, batch, M, N, K, splits, tm) || !tm_bgemm_fold_ok(batch, M, N)) return MIL_EINVAL;
    dim3 grid((N + BP_TN - 1) / BP_TN, (M + tm - 1) / tm, batch * splits);
    bp_launch<true>(tm, grid, (hipStream_t)stream, A, sAb, sAi, sAk, B, sBb, sBk, sBj, ws, (long)M * N, (long)N, 1L,
                    (const float*)nullptr, M, N, K, alpha, 0.f, 0.f, splits);
    tm_bgemm_fold(ws, splits, C, sCb, sCi, sCj, D, batch, M, N, beta, diag, (hipStream_t)stream);
    return launch_rc();
}

}  // extern "C"
