// Functions one .hip file defines and another calls that are not part of the C ABI (include/mil_hip.h).  Included by the
// defining file as well, so the compiler holds every definition against the one prototype; default arguments live here only.
#pragma once
#include <stdlib.h>

#include "mil_common.h"

#define MIL_HIDDEN __attribute__((visibility("hidden")))      /* host planners: not among the library's dynamic symbols */

// MIL_FUSE_POOL=0: keep the pool partial pass a launch of its own (A/B measurements, bit-equality tests)
static inline bool fuse_pool_enabled() {
    const char* e = getenv("MIL_FUSE_POOL");
    return e == nullptr || e[0] != '0';
}

// ---- gate_fwd.hip (called from step.hip, gate_bwd_dx.hip)
// Rows beyond whole rounds of 128-row tiles (tiles_per_round of them per round of the grid) that take the few-rows
// kernels instead of one more round: 1 .. MIL_SMALL_ROWS, or 0
MIL_HIDDEN int gate_tail_rows(int R, int tiles_per_round);
// Gate forward with the pool partial pass in its epilogue when the batch allows it; *fused says whether partials / hrow
// were produced (otherwise the caller runs the stand-alone pool pass).  draw != 0 (train mode): the keep bits are drawn
// by this call into xbits / mbits (seed / mseed / offset as mil_gate_scores_fwd_draw), else xbits / mbits are inputs.
int gate_fwd_with_pool(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu, const float* w,
                       const float* b, float* scores, float* gates, int R, int L, int draw, uint32_t* xbits, float xscale,
                       uint32_t* mbits, float mscale, int B, uint64_t seed, uint64_t mseed, uint64_t offset,
                       const int32_t* offset_dev, const int32_t* tile_map, int T, float* partials, const float* Wf, float* hrow,
                       int* fused, void* stream, const uint16_t* Wp);
// Gate forward of a bucketed batch (rows_dev = true row count on the device, R = capacity; NULL: a plain batch); tmap: the
// tile map is still to be built and goes along (on the generator launch where there is one).
int gate_fwd_rows_dev(const float* x, const float* Wv, const float* bv, const float* Wu, const float* bu, const float* w,
                      const float* b, float* scores, float* gates, int R, int L, int draw, uint32_t* xbits, float xscale,
                      uint32_t* mbits, int B, uint64_t seed, uint64_t mseed, uint64_t offset, const int32_t* offset_dev,
                      const int32_t* rows_dev, void* stream, const TileMapJob* tmap, const uint16_t* Wp);

// The plan of the fp32 step for this descriptor and stage mask (hints included), as mil_image_only_step_run executes it
MIL_HIDDEN mil_gate_route gate_step_plan(const mil_image_only_step* a, uint32_t stages, int ncu);
// The gate forward of the deferred pool (plan p of gate_step_plan, p.pool_deferred set): scores, gates and hrow in one launch
int gate_fwd_deferred(const mil_image_only_step* a, const mil_gate_route& p, bool draw, float xscale, float mscale, void* stream);

// ---- head_loss.hip (called from step.hip)
// The per-bag tail of the deferred pool: k_pool_tail_h's chain half alone, which also stores the row weights a_n to arow [R]
int pool_tail_rows(const int32_t* bag_tile_off, int T, int B, int L, const float* Wf, const float* bf, int C, const float* y,
                   float scale, float* lse, float* z, float* p, float* loss_sum, float* dz, float* dM, float* cdot,
                   const int32_t* tile_map, const float* scores, const float* hrow, float* ds, const uint32_t* mbits, float mscale,
                   int loss_kind, float* arow, void* stream);

// ---- gate_bwd_dw.hip (called from gate_fwd.hip, step.hip)
// MIL_DW_PIECES (read per call): the dw2 route runs the split-bf16 kernel
MIL_HIDDEN bool gate_dw_pieces_on();
// The deferred pool's share of the weight gradient and of its fold: row weights a [R] and tile map in, mpart as workspace;
// the fold then writes M / Mdrop (NULL in eval mode: M is what the head saw) and forms dWf from them
struct GateDwMpool {
    const float* a;
    const int32_t* tile_map;
    const int32_t* bag_tile_off;
    float* mpart;
    float *M, *Mdrop;
    const uint32_t* mbits;
    float mscale;
};
int gate_bwd_partials_mp(const float* x, const float* gates, const float* ds, const float* w, int R, int L, float* workspace,
                         size_t workspace_floats, const uint32_t* xbits, const GateDwMpool& mp, void* stream);
// The weight-gradient part of the route plan for (R, L) on ncu compute units; the same plan sizes the workspace
struct GateDwPlan {
    int dw, S, kc;          // MIL_ROUTE_DW_*, row chunks (split-K factor), rows per chunk
};
MIL_HIDDEN GateDwPlan gate_dw_plan(int R, int L, int ncu);
// Split-K fold + head gradients + Adam in one launch.  step_dev != NULL: the update's number is (*step_dev + 1), read on
// the device (hipGraph replay); the counter is advanced by this launch itself when `done` (a zeroed sign-off word) is
// given, else by the caller afterwards.  Wp: the weight pieces of the split-bf16 forward, rewritten with the update.
int gate_bwd_reduce_head_adam_impl(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu,
                                   float* dw, float* db, int accumulate, float xscale, const float* dz, const float* M,
                                   float* dWf, float* dbf, int B, int C, const float* loss_bag, float* loss_out,
                                   float* param_flat, const float* grad_flat, size_t n_param, float* exp_avg,
                                   float* exp_avg_sq, int step, const int* step_dev, float lr, const float* lr_dev, float beta1,
                                   float beta2, float eps, float weight_decay, float grad_scale, void* stream,
                                   int* done = nullptr, uint16_t* Wp = nullptr, const GateDwMpool* mp = nullptr);
// mil_gate_bwd_reduce_head for the deferred pool
int gate_bwd_reduce_head_mp(const float* workspace, int R, int L, float* dWv, float* dbv, float* dWu, float* dbu, float* dw,
                            float* db, int accumulate, float xscale, const float* dz, float* dWf, float* dbf, int B, int C,
                            const float* loss_bag, float* loss_out, const GateDwMpool& mp, void* stream);

// ---- gated_pool_bf16.hip (called from step.hip)
// bf16-MFMA weight gradient whose fold launch carries the head gradients, the loss and (param_flat != NULL) Adam + the
// refresh of the bf16 weight shadows
int gate_bwd_params_bf16_tail(const uint16_t* x, const uint16_t* gates, const float* ds, const float* w, int R, int L,
                              float* workspace, size_t workspace_floats, float* dWv, float* dbv, float* dWu, float* dbu,
                              float* dw, float* db, int accumulate, const uint32_t* xbits, float xscale, const float* dz,
                              const float* M, float* dWf, float* dbf, int B, int C, const float* loss_bag, float* loss_out,
                              float* param_flat, const float* grad_flat, size_t n_param, float* exp_avg, float* exp_avg_sq,
                              int step, const int* step_dev, float lr, const float* lr_dev, float beta1, float beta2, float eps,
                              float weight_decay, float grad_scale, uint16_t* Wv16, uint16_t* Wu16, void* stream, int* done);
// bf16 gate forward with the pool partial pass in its epilogue when the batch allows (*fused as gate_fwd_with_pool)
int gate_fwd_bf16_with_pool(const uint16_t* x, const uint16_t* Wv, const float* bv, const uint16_t* Wu, const float* bu,
                            const float* w, const float* b, float* scores, uint16_t* gates16, int R, int L, const uint32_t* xbits,
                            float xscale, const int32_t* tile_map, int T, float* partials, const float* Wf, float* hrow,
                            const uint32_t* mbits, float mscale, int* fused, void* stream);

// ---- dropout.hip (called from gate_fwd.hip, step.hip)
// both keep-bit tensors of a step in one launch; _tilemap: mil_build_tile_map rides along as one more workgroup
int dropout_keep_bits_pair(uint32_t* xbits, int R, uint32_t* mbits, int B, int L, uint64_t seed, uint64_t mseed, uint64_t offset,
                           const int32_t* offset_dev, void* stream);
int dropout_keep_bits_pair_tilemap(uint32_t* xbits, int R, uint32_t* mbits, int B, int L, uint64_t seed, uint64_t mseed,
                                   uint64_t offset, const int32_t* offset_dev, const TileMapJob& tm, void* stream);

// ---- linear_nt2.hip (called from linear.hip)
// k_gemm_tn2's row split on ncu compute units (-> splits, *KC_out rows per split) and whether mil_linear_bwd_params takes it
MIL_HIDDEN int gemm_tn2_plan(int rows, int N, int K, int ncu, int* KC_out);
MIL_HIDDEN int gemm_tn2_ok(int lddy, int ldy, int ldx, int rows, int N, int K, int ncu);
int mil_gemm_tn2_rows(const float* dY, int lddy, const float* Y, int ldy, int act, const float* X, int ldx, int rows, int N, int K,
                      float* partial, float* cs_partial, const int32_t* rows_dev, void* stream);
