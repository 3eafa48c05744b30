// Evaluation log and ROC metrics (ABI 24): what the reference's valid() (train_ddp.py:382-513) and test_ddp.py:141-162,286-309
// compute on the host from per-bag reads, kept on the device until the epoch ends.
//   mil_eval_push    one step's probabilities, classes and criterion values appended at the row a device counter names
//   mil_eval_rank    binary models: per sample, how many positives / negatives score at least as high (all pairs, tiled)
//   mil_eval_reduce  confusion matrix, step-weighted loss sums, P, N, the AUC numerator and the Youden index, one workgroup
// Every count is an integer and every sum runs in an order the sizes fix, so two runs give the same bits.  No float atomics,
// no inline assembly; all results leave through ordinary global stores.
#include "mil_internal.h"

// ---------------------------------------------------------------------------------------------
// push: one workgroup of 64 threads; B C <= 64.  ctr = {rows, steps, flag, 0}.
// ---------------------------------------------------------------------------------------------
struct EvalPushArgs {
    const float* p[MIL_EVAL_MAX_TERMS];   // p[0]: the Last head (the one that is logged), then CT, Pth
    const float* y;
    const float* extra;
    int B, C, nterm, ce, capacity;
    float* log_prob;
    int32_t* log_cls;
    int32_t* step_b;
    double* step_loss;
    int32_t* ctr;
};

// one element of BCELoss in double, each log clamped at -100 as torch does
__device__ __forceinline__ double eval_bce_elem(float p, float y) {
    const double pd = (double)p, yd = (double)y;
    const double lp = fmax(log(pd), -100.0), l1p = fmax(log(1.0 - pd), -100.0);
    return -(yd * lp + (1.0 - yd) * l1p);
}

__global__ __launch_bounds__(64) void k_eval_push(EvalPushArgs a) {
    __shared__ double s_el[MIL_EVAL_MAX_TERMS][64];
    __shared__ int s_flag;
    const int tid = threadIdx.x, B = a.B, C = a.C, n = B * C;
    const int row0 = a.ctr[MIL_EVAL_CTR_ROWS], step = a.ctr[MIL_EVAL_CTR_STEPS], flag0 = a.ctr[MIL_EVAL_CTR_FLAG];
    if (tid == 0) s_flag = 0;
    __syncthreads();                                  // every thread holds the counters before thread 0 moves them
    if (row0 < 0 || step < 0 || row0 + B > a.capacity || step >= a.capacity) {
        if (tid == 0) a.ctr[MIL_EVAL_CTR_FLAG] = flag0 | MIL_EVAL_FLAG_OVERFLOW;     // dropped
        return;
    }
    int bad = 0;
    if (a.ce) {
        // CrossEntropyLoss on the sigmoid outputs with float one-hot targets: thread b owns bag b
        if (tid < B)
            for (int t = 0; t < a.nterm; ++t) {
                const float* p = a.p[t] + (size_t)tid * C;
                double mx = (double)p[0];
                for (int c = 1; c < C; ++c) mx = fmax(mx, (double)p[c]);
                double se = 0.0;
                for (int c = 0; c < C; ++c) se += exp((double)p[c] - mx);
                const double lse = mx + log(se);
                double l = 0.0;
                for (int c = 0; c < C; ++c) {
                    l -= (double)a.y[(size_t)tid * C + c] * ((double)p[c] - lse);
                    bad |= (p[c] != p[c]);
                }
                s_el[t][tid] = l;
            }
    } else if (tid < n) {
        for (int t = 0; t < a.nterm; ++t) {
            const float p = a.p[t][tid];
            bad |= (p != p);
            s_el[t][tid] = eval_bce_elem(p, a.y[tid]);
        }
    }
    if (tid < n) a.log_prob[(size_t)row0 * C + tid] = a.p[0][tid];
    if (tid < B) {
        // first maximal index wins, as torch.argmax
        const float* p = a.p[0] + (size_t)tid * C;
        const float* y = a.y + (size_t)tid * C;
        int ip = 0, iy = 0;
        for (int c = 1; c < C; ++c) {
            if (p[c] > p[ip]) ip = c;
            if (y[c] > y[iy]) iy = c;
        }
        a.log_cls[2 * (size_t)(row0 + tid)] = iy;
        a.log_cls[2 * (size_t)(row0 + tid) + 1] = ip;
    }
    if (bad) atomicOr(&s_flag, MIL_EVAL_FLAG_NAN);
    __syncthreads();
    if (tid == 0) {
        const int terms = a.ce ? B : n;
        for (int t = 0; t < MIL_EVAL_MAX_TERMS; ++t) {
            double s = 0.0;
            if (t < a.nterm)
                for (int i = 0; i < terms; ++i) s += s_el[t][i];
            a.step_loss[(size_t)step * MIL_EVAL_LOSS_SLOTS + t] = s / (double)terms;
        }
        a.step_loss[(size_t)step * MIL_EVAL_LOSS_SLOTS + MIL_EVAL_MAX_TERMS] = a.extra ? (double)a.extra[0] : 0.0;
        a.step_b[step] = B;
        a.ctr[MIL_EVAL_CTR_ROWS] = row0 + B;
        a.ctr[MIL_EVAL_CTR_STEPS] = step + 1;
        if (s_flag) a.ctr[MIL_EVAL_CTR_FLAG] = flag0 | s_flag;
    }
}

extern "C" int mil_eval_push(const float* p_last, const float* p_ct, const float* p_pth, const float* y, const float* extra,
                             int B, int C, int nterm, int ce, int capacity, float* log_prob, int32_t* log_cls,
                             int32_t* step_b, double* step_loss, int32_t* ctr, void* stream) {
    if (!p_last || !y || !log_prob || !log_cls || !step_b || !step_loss || !ctr) return MIL_EINVAL;
    if (B < 1 || C < 1 || (long)B * C > 64 || nterm < 1 || nterm > MIL_EVAL_MAX_TERMS || capacity < 1) return MIL_EINVAL;
    if ((nterm >= 2 && !p_ct) || (nterm >= 3 && !p_pth)) return MIL_EINVAL;
    EvalPushArgs a{};
    a.p[0] = p_last; a.p[1] = p_ct; a.p[2] = p_pth;
    a.y = y; a.extra = extra;
    a.B = B; a.C = C; a.nterm = nterm; a.ce = ce; a.capacity = capacity;
    a.log_prob = log_prob; a.log_cls = log_cls; a.step_b = step_b; a.step_loss = step_loss; a.ctr = ctr;
    hipLaunchKernelGGL(k_eval_push, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// ---------------------------------------------------------------------------------------------
// rank: binary scores s_i = log_prob[i][1], positives = label class 1.  One wave per tile of MIL_EVAL_TILE samples i (one per
// lane); the j side goes through LDS a tile at a time and every lane reads the same LDS word (a broadcast).  The grid covers
// the capacity; n comes from the device counter, so nothing is read on the host between the last push and this launch.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MIL_EVAL_TILE) void k_eval_rank(const float* __restrict__ log_prob, const int32_t* __restrict__ log_cls,
                                                            const int32_t* __restrict__ ctr, int capacity,
                                                            int32_t* __restrict__ rank) {
    __shared__ float s_s[MIL_EVAL_TILE];
    __shared__ int s_pos[MIL_EVAL_TILE];
    const int n = min(max(ctr[MIL_EVAL_CTR_ROWS], 0), capacity);
    const int i0 = blockIdx.x * MIL_EVAL_TILE, lane = threadIdx.x, i = i0 + lane;
    if (i0 >= n) return;                                        // the whole workgroup leaves together
    const float si = i < n ? log_prob[2 * (size_t)i + 1] : 0.f;
    int ge_pos = 0, ge_neg = 0, eq_neg = 0;
    for (int j0 = 0; j0 < n; j0 += MIL_EVAL_TILE) {
        const int j = j0 + lane;
        __syncthreads();
        s_s[lane] = j < n ? log_prob[2 * (size_t)j + 1] : 0.f;
        s_pos[lane] = j < n ? (log_cls[2 * (size_t)j] == 1) : 0;
        __syncthreads();
        const int m = min(MIL_EVAL_TILE, n - j0);
        for (int k = 0; k < m; ++k) {
            const float sj = s_s[k];
            const int pos = s_pos[k];
            const int ge = sj >= si, eq = sj == si;
            ge_pos += ge & pos;
            ge_neg += ge & (pos ^ 1);
            eq_neg += eq & (pos ^ 1);
        }
    }
    if (i < n) {
        rank[3 * (size_t)i] = ge_pos;
        rank[3 * (size_t)i + 1] = ge_neg;
        rank[3 * (size_t)i + 2] = eq_neg;
    }
}

extern "C" int mil_eval_rank(const float* log_prob, const int32_t* log_cls, const int32_t* ctr, int capacity, int32_t* rank,
                             void* stream) {
    if (!log_prob || !log_cls || !ctr || !rank) return MIL_EINVAL;
    if (capacity < 1 || capacity > MIL_EVAL_MAX_ROWS) return MIL_EINVAL;
    const int blocks = (capacity + MIL_EVAL_TILE - 1) / MIL_EVAL_TILE;
    hipLaunchKernelGGL(k_eval_rank, dim3(blocks), dim3(MIL_EVAL_TILE), 0, (hipStream_t)stream, log_prob, log_cls, ctr, capacity,
                       rank);
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}

// ---------------------------------------------------------------------------------------------
// reduce: one workgroup of 256 threads.  Thread t takes the samples (steps) t, t + 256, ... in that order, the 256 partial
// results are folded by a fixed tree in LDS: the double sums come out the same every run, the integers are exact anyway.
// out: MIL_EVAL_OUT_WORDS 8-byte words (mil_hip.h) followed by the C x C confusion matrix as int32, conf[label][pred].
// ---------------------------------------------------------------------------------------------
#define ER_NT 256
__device__ __forceinline__ bool youden_better(long long ka, float sa, int ia, long long kb, float sb, int ib) {
    // a beats b: larger tpr - fpr (an exact integer comparison), then the larger score, then the lower index
    if (ka != kb) return ka > kb;
    if (sa != sb) return sa > sb;
    return ia < ib;
}

__global__ __launch_bounds__(ER_NT) void k_eval_reduce(const float* __restrict__ log_prob, const int32_t* __restrict__ log_cls,
                                                      const int32_t* __restrict__ step_b, const double* __restrict__ step_loss,
                                                      const int32_t* __restrict__ ctr, const int32_t* __restrict__ rank,
                                                      int capacity, int C, double thres, long long* __restrict__ out) {
    extern __shared__ int s_conf[];                     // C * C
    __shared__ double s_d[ER_NT];
    __shared__ long long s_l[ER_NT];
    __shared__ float s_f[ER_NT];
    __shared__ int s_i[ER_NT];
    __shared__ long long s_res[8];
    const int tid = threadIdx.x;
    const int n = min(max(ctr[MIL_EVAL_CTR_ROWS], 0), capacity), ns = min(max(ctr[MIL_EVAL_CTR_STEPS], 0), capacity);
    const bool binary = C == 2 && rank != nullptr;
    int32_t* conf = reinterpret_cast<int32_t*>(out + MIL_EVAL_OUT_WORDS);
    double* outd = reinterpret_cast<double*>(out);

    for (int k = tid; k < C * C; k += ER_NT) s_conf[k] = 0;
    __syncthreads();
    // confusion matrix and P, N (integer LDS adds: exact in any order)
    int npos = 0;
    for (int i = tid; i < n; i += ER_NT) {
        const int yl = log_cls[2 * (size_t)i], pl = log_cls[2 * (size_t)i + 1];
        if (yl >= 0 && yl < C && pl >= 0 && pl < C) atomicAdd(&s_conf[yl * C + pl], 1);
        npos += (yl == 1);
    }
    s_l[tid] = npos;
    __syncthreads();
    for (int w = ER_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) s_l[tid] += s_l[tid + w];
        __syncthreads();
    }
    if (tid == 0) s_res[0] = s_l[0];
    __syncthreads();
    const long long P = s_res[0], N = (long long)n - P;
    for (int k = tid; k < C * C; k += ER_NT) conf[k] = s_conf[k];

    // step-weighted loss sums: sum loss_step B_step per slot, and sum B_step
    for (int slot = 0; slot <= MIL_EVAL_LOSS_SLOTS; ++slot) {
        double acc = 0.0;
        for (int s = tid; s < ns; s += ER_NT) {
            const double b = (double)step_b[s];
            acc += slot < MIL_EVAL_LOSS_SLOTS ? step_loss[(size_t)s * MIL_EVAL_LOSS_SLOTS + slot] * b : b;
        }
        __syncthreads();
        s_d[tid] = acc;
        __syncthreads();
        for (int w = ER_NT / 2; w >= 1; w >>= 1) {
            if (tid < w) s_d[tid] += s_d[tid + w];
            __syncthreads();
        }
        if (tid == 0) outd[MIL_EVAL_OUT_LOSS + slot] = s_d[0];
    }

    // the AUC numerator, the counts at the given threshold and the Youden index
    long long s2 = 0, tp_at = 0, fp_at = 0, bk = -1;
    float bs = 0.f;
    int bi = -1;
    if (binary)
        for (int i = tid; i < n; i += ER_NT) {
            const int pos = log_cls[2 * (size_t)i] == 1;
            const float s = log_prob[2 * (size_t)i + 1];
            const long long gp = rank[3 * (size_t)i], gn = rank[3 * (size_t)i + 1], en = rank[3 * (size_t)i + 2];
            if (pos) s2 += 2 * (N - gn) + en;
            if ((double)s >= thres) { tp_at += pos; fp_at += pos ^ 1; }
            const long long key = gp * N - gn * P;
            if (bi < 0 || youden_better(key, s, i, bk, bs, bi)) { bk = key; bs = s; bi = i; }
        }
    for (int q = 0; q < 3; ++q) {
        __syncthreads();
        s_l[tid] = q == 0 ? s2 : (q == 1 ? tp_at : fp_at);
        __syncthreads();
        for (int w = ER_NT / 2; w >= 1; w >>= 1) {
            if (tid < w) s_l[tid] += s_l[tid + w];
            __syncthreads();
        }
        if (tid == 0) s_res[1 + q] = s_l[0];
    }
    __syncthreads();
    s_l[tid] = bk; s_f[tid] = bs; s_i[tid] = bi;
    __syncthreads();
    for (int w = ER_NT / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const int o = tid + w;
            if (s_i[o] >= 0 && (s_i[tid] < 0 || youden_better(s_l[o], s_f[o], s_i[o], s_l[tid], s_f[tid], s_i[tid]))) {
                s_l[tid] = s_l[o]; s_f[tid] = s_f[o]; s_i[tid] = s_i[o];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int istar = s_i[0];
        out[MIL_EVAL_OUT_N] = n;
        out[MIL_EVAL_OUT_STEPS] = ns;
        out[MIL_EVAL_OUT_FLAG] = ctr[MIL_EVAL_CTR_FLAG];
        out[MIL_EVAL_OUT_P] = P;
        out[MIL_EVAL_OUT_NEG] = N;
        out[MIL_EVAL_OUT_S2] = s_res[1];
        out[MIL_EVAL_OUT_TP_AT] = s_res[2];
        out[MIL_EVAL_OUT_FP_AT] = s_res[3];
        out[MIL_EVAL_OUT_JSTAR] = istar >= 0 ? s_l[0] : 0;
        out[MIL_EVAL_OUT_ISTAR] = istar;
        out[MIL_EVAL_OUT_GE_POS] = istar >= 0 ? rank[3 * (size_t)istar] : 0;
        out[MIL_EVAL_OUT_GE_NEG] = istar >= 0 ? rank[3 * (size_t)istar + 1] : 0;
        outd[MIL_EVAL_OUT_SSTAR] = istar >= 0 ? (double)s_f[0] : 0.0;
    }
}

extern "C" size_t mil_eval_out_bytes(int C) {
    if (C < 1 || C > 64) return 0;
    return (size_t)MIL_EVAL_OUT_WORDS * 8 + (((size_t)C * C * 4 + 7) & ~(size_t)7);
}

extern "C" int mil_eval_reduce(const float* log_prob, const int32_t* log_cls, const int32_t* step_b, const double* step_loss,
                               const int32_t* ctr, const int32_t* rank, int capacity, int C, double thres, void* out,
                               void* stream) {
    if (!log_prob || !log_cls || !step_b || !step_loss || !ctr || !out) return MIL_EINVAL;
    if (capacity < 1 || capacity > MIL_EVAL_MAX_ROWS || C < 1 || C > 64) return MIL_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 7) return MIL_EINVAL;
    hipLaunchKernelGGL(k_eval_reduce, dim3(1), dim3(ER_NT), (size_t)C * C * sizeof(int), (hipStream_t)stream, log_prob, log_cls,
                       step_b, step_loss, ctr, rank, capacity, C, thres, reinterpret_cast<long long*>(out));
    MIL_CHECK_LAUNCH();
    return MIL_OK;
}
