// TransMIL: a step's bags as one packed sequence - the segment table of the mil_tm_*_packed entries, once.
//
// The packed rows are the bags' front-padded [n_pad_b, 1536] to_qkv rows one after another, R = 256 x total_blocks of them; every
// n_pad_b is a multiple of 256, so a 256-row block belongs to one bag and no tile of a token-side kernel (128 or 256 rows, aligned)
// straddles two.  The table `tab` (device int32, [nb + 1 + total_blocks], built on the host by ops.tm_packed_table):
//   tab[b], b <= nb           blk_off: the cumulative count of 256-row blocks in front of bag b (blk_off[nb] = total_blocks)
//   tab[nb + 1 + k]           bag_of_blk: the bag of block k - the lookup of a workgroup is one scalar load
// Bag b owns rows [256 blk_off[b], 256 blk_off[b + 1]), its landmark group is l_b = blk_off[b + 1] - blk_off[b], and its small
// operands (qL, kL, W, U, lse3, their gradients) are slice b of buffers stacked [nb, 8, 256, .].
// A kernel trusts nothing the table holds: a block outside [0, total_blocks), a bag outside [0, nb) or a block range outside
// [0, total_blocks] makes the workgroup return (tm_packed_bag, tm_packed_range), so whatever the table says no address leaves
// the rows [0, R) or the nb slices.  The block index comes from blockIdx alone: the bag and every pointer derived from it are
// wave-uniform (readfirstlane pins them to scalar registers).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace {

constexpr int TM_PACKED_MAX_BAGS = 1024;            // as the grouped pseudo-inverse start (PINV_MAX_BAGS)
constexpr int TM_PACKED_BLK = 256;                  // rows of a block

// the bag of block `blk`, or -1
__device__ __forceinline__ int tm_packed_bag(const int32_t* __restrict__ tab, int nb, int total_blocks, int blk) {
    if (blk < 0 || blk >= total_blocks) return -1;
    const int b = __builtin_amdgcn_readfirstlane(tab[nb + 1 + blk]);
    return b >= 0 && b < nb ? b : -1;
}

// the blocks [c0, c1) of bag b (0 <= b < nb); false when they do not lie in [0, total_blocks] or are none
__device__ __forceinline__ bool tm_packed_range(const int32_t* __restrict__ tab, int total_blocks, int b, int& c0, int& c1) {
    c0 = __builtin_amdgcn_readfirstlane(tab[b]);
    c1 = __builtin_amdgcn_readfirstlane(tab[b + 1]);
    return c0 >= 0 && c1 > c0 && c1 <= total_blocks;
}

// The table as ONE trailing kernel argument, for the kernels that are templated on <bool PACKED> themselves because their code
// does not survive being moved into a shared body unchanged: empty, and so no argument at all, in the single-bag instantiation
template <bool PACKED>
struct TmPackedArg {
    const int32_t* tab;
    int nb, total_blocks;
};
template <>
struct TmPackedArg<false> {};

// what every packed status entry checks before a launch: 1 <= nb <= 1024, at least one block per bag, and 256 x total_blocks rows
// within what an int row index holds
inline bool tm_packed_ok(const void* tab, int nb, int total_blocks) {
    return tab != nullptr && nb >= 1 && nb <= TM_PACKED_MAX_BAGS && total_blocks >= nb && total_blocks <= INT_MAX / TM_PACKED_BLK;
}

}  // namespace
