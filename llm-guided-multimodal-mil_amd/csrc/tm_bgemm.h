// TransMIL: what the two batched-product kernels share - k_tm_bgemm (csrc/transmil.hip, v_mfma_f32_32x32x2_f32) and
// k_tm_bgemm_pieces (csrc/tm_bgemm_pieces.hip, three-piece split-bf16 on v_mfma_f32_32x32x16_bf16): the argument rules of
// the entries, the epilogue of one 32 x 32 accumulator and the fold launch of the fixed-order split-K form.  Everything sits
// in the including file's anonymous namespace (as nystrom_tile.h / gemm64.h do): nothing is exported.
#pragma once
#include <hip/hip_runtime.h>

#include "mil_common.h"

namespace {

constexpr int BG_FOLD_K = 512;        // the MFMA chain folds into a second accumulator every 512 of K (docs/lab_notes.md)

// One 32 x 32 accumulator (column `col` on the lane, row row0 + mfma32_row(i, h) in register i) through the epilogue
// C = alpha acc + beta D + diag I.  splits > 1 adds atomically onto an initialised C (diag from split 0).
// FIXED: C is the workspace ws + bz M N, and split p stores alpha x its partial tile into ws[p][batch][M][N].
template <bool FIXED>
__device__ __forceinline__ void tm_bgemm_store(const f32x16& acc, float* C, long sCi, long sCj, const float* D, int M, int N,
                                               int row0, int col, int h, float alpha, float beta, float diag, int splits,
                                               int split) {
    if (col >= N) return;
    const long batch = FIXED ? gridDim.z / splits : 0;                    // C = ws + bz M N already (sCb = M N)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = row0 + mfma32_row(i, h);
        if (row >= M) continue;
        float* cp = C + row * sCi + col * sCj;
        float v = alpha * acc[i];
        if constexpr (FIXED) {
            C[(split * batch * M + row) * N + col] = v;
        } else if (splits == 1) {
            if (beta != 0.f) v += beta * (D != nullptr ? D[row * sCi + col * sCj] : *cp);
            if (row == col) v += diag;
            *cp = v;
        } else {
            if (row == col && split == 0) v += diag;
            atomicAdd(cp, v);
        }
    }
}

// C[b][i][j] = sum_p ws[p][b][i][j] (p = 0, 1, .. splits - 1 in that order) + beta D[b][i][j] + diag [i == j], thread per element
// with the lanes along j; D = C when null.  The launch boundary behind the FIXED product kernel is the only ordering it needs.
__global__ __launch_bounds__(256) void k_tm_bgemm_fold(const float* __restrict__ ws, int splits, float* C, long sCb, long sCi,
                                                       long sCj, const float* D, int batch, int M, int N, float beta, float diag) {
    const long per = (long)batch * M * N, e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const int col = (int)(e % N), row = (int)((e / N) % M);
    const long off = (e / ((long)M * N)) * sCb + row * sCi + col * sCj;
    float v = ws[e];
    for (int p = 1; p < splits; ++p) v += ws[p * per + e];
    if (beta != 0.f) v += beta * (D != nullptr ? D[off] : C[off]);
    if (row == col) v += diag;
    C[off] = v;
}

// The argument rules of mil_tm_bgemm (atomic split-K: splits > 1 needs beta == 1 and no D) and of mil_tm_bgemm_fixed
// (any beta, D and diag with any splits; a workspace), with the grid limits of a tile of `tile_m` rows.
inline bool tm_bgemm_args_ok(const void* A, const void* B, const void* C, int batch, int M, int N, int K, int splits, int tile_m) {
    if (!A || !B || !C || batch <= 0 || M <= 0 || N <= 0 || K <= 0 || splits <= 0) return false;
    return (M + tile_m - 1) / tile_m <= 65535 && (long)batch * splits <= 65535;
}
inline bool tm_bgemm_atomic_ok(float beta, const float* D, int splits) { return splits == 1 || (beta == 1.f && D == nullptr); }
inline bool tm_bgemm_fold_ok(int batch, int M, int N) { return ((long)batch * M * N + 255) / 256 <= 0x7fffffffL; }

inline void tm_bgemm_fold(const float* ws, int splits, float* C, long sCb, long sCi, long sCj, const float* D, int batch, int M,
                          int N, float beta, float diag, hipStream_t stream) {
    const long per = (long)batch * M * N;
    hipLaunchKernelGGL(k_tm_bgemm_fold, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, stream, ws, splits, C, sCb, sCi, sCj, D,
                       batch, M, N, beta, diag);
}

}  // namespace
