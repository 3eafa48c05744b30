// TransMIL: PPEG of a step's bags in one launch set - the table of the mil_tm_ppeg_*_packed entries, once.
//
// PPEG works on the UNPADDED sequence rows: the packed rows are the bags' [1 + s_b^2, 512] sequences (cls row first) one after
// another, R = sum (1 + s_b^2) of them, so bag b starts at a row that is no multiple of 256 and the block table of tm_packed.h does
// not describe it.  The table `tab` (device int32, built on the host by ops.tm_ppeg_table from the tuple of sides alone) has a
// length that depends on (nb, R) only, so that a kernel can bound every read of it by its own arguments:
//   gmax = floor(sqrt(nb (R - nb)))           >= sum s_b            (Cauchy-Schwarz on sum s_b^2 = R - nb)
//   cmax = min(gmax, (gmax + 7 nb) / 8)       >= sum ceil(s_b / 8)
//   tab[b],               b <= nb             row_off:   the first sequence row of bag b (its cls row), row_off[nb] = R
//   tab[nb + 1 + b],      b <  nb             side:      s_b
//   tab[2 nb + 1 + b],    b <= nb             grow_off:  the grid rows in front of bag b, grow_off[nb] = G = sum s_b
//   tab[3 nb + 2 + b],    b <= nb             chunk_off: the 8-grid-row chunks in front of bag b, chunk_off[nb] = C = sum ceil(s_b / 8)
//   tab[4 nb + 3 + g],    g <  gmax           bag_of_gridrow: the bag of packed grid row g, -1 for G <= g < gmax
//   tab[4 nb + 3 + gmax + k], k < cmax        bag_of_chunk:   the bag of packed chunk k (bag 0's chunks first, ascending), -1 behind C
// in all 4 nb + 3 + gmax + cmax ints.  The launches are shaped by (nb, R) as well: gmax grid rows (a workgroup whose entry is -1
// returns), ceil(floor(sqrt(R - 2 nb + 1)) / 8) column chunks (no side is larger than that root), cmax chunks.
// A kernel trusts nothing the table holds.  A workgroup returns without touching x, y or a gradient when its bag is outside
// [0, nb), s_b < 1, row_off[b] < 0 or row_off[b] + 1 + s_b^2 > R (tm_ppeg_bag), when its grid row is outside [0, s_b)
// (tm_ppeg_gridrow) or its chunk's first grid row outside [0, s_b) (tm_ppeg_chunk): whatever the table says, no address leaves the
// rows [0, R).  The grid row and the chunk come from blockIdx alone, so the bag and every pointer derived from it are wave-uniform
// (readfirstlane pins them to scalar registers).  What the table alone states is the number of chunks the fixed-order fold adds,
// clamped into [0, cmax]: the workspace of mil_tm_ppeg_bwd_packed_fixed holds the chunks of the sides the table was built from.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace {

constexpr int TM_PPEG_MAX_BAGS = 1024;              // as TM_PACKED_MAX_BAGS
constexpr int TM_PPEG_D = 512;                      // channels of a row
constexpr int TM_PPEG_CHUNK = 8;                    // grid rows of a weight-gradient chunk (PPEG_ROWS)

struct TmPpegDims {
    int gmax, cmax, zmax;                           // grid rows, chunks, 8-column chunks of the widest bag a table of (nb, R) can hold
};

inline int tm_ppeg_isqrt(long v) {                  // floor(sqrt(v)), v >= 0
    long r = (long)__builtin_sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int)r;
}

// what every packed PPEG status entry checks before a launch: 1 <= nb <= 1024, a cls row and a cell per bag, and 512 x R within
// what an int index holds
inline bool tm_ppeg_ok(const void* tab, int nb, int total_rows) {
    return tab != nullptr && nb >= 1 && nb <= TM_PPEG_MAX_BAGS && total_rows >= 2 * nb && total_rows <= INT_MAX / TM_PPEG_D;
}

inline TmPpegDims tm_ppeg_dims(int nb, int total_rows) {        // tm_ppeg_ok(.., nb, total_rows) holds
    TmPpegDims d;
    d.gmax = tm_ppeg_isqrt((long)nb * (total_rows - nb));
    const int c = (d.gmax + 7 * nb) / TM_PPEG_CHUNK;
    d.cmax = c < d.gmax ? c : d.gmax;
    d.zmax = (tm_ppeg_isqrt((long)total_rows - 2 * nb + 1) + 7) / 8;
    return d;
}

// bag b's side and first row; false when b or what the table says of it would leave the rows [0, R)
__device__ __forceinline__ bool tm_ppeg_bag(const int32_t* __restrict__ tab, int nb, int total_rows, int b, int& s, int& row) {
    if (b < 0 || b >= nb) return false;
    row = __builtin_amdgcn_readfirstlane(tab[b]);
    s = __builtin_amdgcn_readfirstlane(tab[nb + 1 + b]);
    return s >= 1 && row >= 0 && (long)row + 1 + (long)s * s <= total_rows;
}

// packed grid row g (from blockIdx) -> its bag's side, first row and the grid row i inside the bag; false: the workgroup returns
__device__ __forceinline__ bool tm_ppeg_gridrow(const int32_t* __restrict__ tab, int nb, int total_rows, int gmax, int g, int& s,
                                                int& row, int& i) {
    if (g < 0 || g >= gmax) return false;
    const int b = __builtin_amdgcn_readfirstlane(tab[4 * nb + 3 + g]);
    if (!tm_ppeg_bag(tab, nb, total_rows, b, s, row)) return false;
    i = g - __builtin_amdgcn_readfirstlane(tab[2 * nb + 1 + b]);
    return i >= 0 && i < s;
}

// packed chunk k (from blockIdx) -> its bag's side, first row and the chunk's first grid row r0; false: the chunk adds nothing
__device__ __forceinline__ bool tm_ppeg_chunk(const int32_t* __restrict__ tab, int nb, int total_rows, int gmax, int cmax, int k,
                                              int& s, int& row, int& r0) {
    if (k < 0 || k >= cmax) return false;
    const int b = __builtin_amdgcn_readfirstlane(tab[4 * nb + 3 + gmax + k]);
    if (!tm_ppeg_bag(tab, nb, total_rows, b, s, row)) return false;
    const int c = k - __builtin_amdgcn_readfirstlane(tab[3 * nb + 2 + b]);
    if (c < 0 || c > (s - 1) / TM_PPEG_CHUNK) return false;
    r0 = c * TM_PPEG_CHUNK;
    return true;
}

// the number of chunks the fold adds: chunk_off[nb], clamped into [0, cmax]
__device__ __forceinline__ int tm_ppeg_chunks(const int32_t* __restrict__ tab, int nb, int cmax) {
    const int c = __builtin_amdgcn_readfirstlane(tab[4 * nb + 2]);
    return c < 0 ? 0 : (c > cmax ? cmax : c);
}

}  // namespace
