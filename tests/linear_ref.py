"""Restatement of the tiled fp32 linear family (csrc/linear.hip, gemm64.h, linear_nt2.hip, mid_linear.hip) for any float
dtype: the routing rules (gemm_route, bwd_params_route: what mil_gemm_route / mil_linear_bwd_params_route must answer), the
product in the route's arithmetic order (K walked in 32-deep slices, one partial sum per split, the fold, the epilogue where
the route puts it, the split last round as two row ranges, the rows_dev contract), the parameter backward, the column sums,
the activation backward and the mid-size kernels.  float64 is the reference, the same code in float32 on the CPU gives `e32`;
mutate= plants one error (tests/test_linear_sensitivity_host.py shows that the per-block bounds of
tests/test_gpu_linear_stages.py see each of them).  Outputs are whole buffers [rows, ld], pre-filled with a sentinel: the
guard columns of a strided run are a block whose reference is the sentinel.  Test-side helper: only the lib_* functions at
the end (the library's own statement of its routes) touch the code under test."""
import functools
import math

import numpy as np
import torch

from transmil_ref import FLOOR, K_CAP, block_err, bound  # noqa: F401  (re-exported to the test files)

QG = 1.702
BK = 32                               # depth of a K slice
SENT = float(np.float32(-12345.678))  # the sentinel, as float32 holds it
GUARD = 8                             # guard columns of a strided output: ld = N + 8
NCU = 256                             # compute units the run lists are chosen for (MI355X)
KERNELS = ("NT2", "G64", "G64N", "TAIL", "NT", "NN", "TN", "TN2", "TN_AX")          # MIL_GEMM_KERNEL_* by value
ACT_NAMES = ("none", "tanh", "relu", "quickgelu")
ROUTE_FIELDS = ("kernel", "S", "kchunk", "rows_main", "main_kernel", "rows_honoured", "need")

GEMM_MUTATIONS = ("k_last_slice", "split_missing", "bias_per_split", "act_per_partial", "tail_res_offset", "tail_aux_offset",
                  "tail_c_offset", "acc_overwrite", "aux1_post", "aux2_from_out", "last_row", "col_shift", "guard_write",
                  "stale_behind", "zero_last_group")
BWD_MUTATIONS = ("dact_from_dy", "db_last_split", "dw_rows_mult", "rows_ignored", "acc_overwrite", "guard_write")
MID_MUTATIONS = ("k_last8", "dw_rows_mult", "dact_from_dy", "last_row")


def _cdiv(a, b):
    return -(-a // b)


def _up(a, b):
    return _cdiv(a, b) * b


# --------------------------------------------------------------------------- the routing rules
def _chunks(K, S):
    """K over S splits in whole 32-deep slices -> (splits that are not empty, K per split)."""
    kc = _up(_cdiv(K, S), BK)
    S = _cdiv(K, kc)
    return (S, kc) if S > 1 else (1, K)


def _nt2_shape_ok(lda, ldb, M, N, K):
    return (N % 256 == 0 and K >= 64 and K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0
            and 256 * lda * 4 < 0x7fff0000 and 256 * ldb * 4 < 0x7fff0000)


def _nt2_fills(M, N, ncu):
    """256 x 256 tiles: at least 3/4 of one round of the chip and 7/8 of the rounds they take."""
    tiles = _cdiv(M, 256) * (N // 256)
    return tiles >= 3 * ncu // 4 and 8 * tiles >= 7 * _cdiv(tiles, ncu) * ncu


def _split_big_tile(M, N, K, a_mode, ncu):
    """Split-K of the 128 x 128 kernel: weight gradients always fill two workgroups per CU; the other forms split only from
    K = 256 on, a handful of tiles (<= 32) to fill the chip with at least two slices per split, up to one round of tiles by
    the cost model (6 us per slice pair of a round against 8 bytes per output element per split at 4 TB/s)."""
    f = np.float32
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    slots = 2 * ncu
    if a_mode == 1:
        S = slots // tiles
    elif K < 256:
        return 1, K
    elif tiles > 32:
        if tiles >= slots:
            return 1, K
        t_round = f(6.0) * f(K) / f(32.0)
        t_part = f(8.0) * f(M) * f(N) / f(4.0e6)
        best, S = t_round, 1
        for c in range(2, 7):
            if c > K // 128:
                break
            cost = f(_cdiv(tiles * c, slots)) / f(c) * t_round + f(c) * t_part
            if cost < f(0.9) * best:
                best, S = cost, c
    else:
        S = min(slots // tiles, K // 64)
    S = min(S, _cdiv(K, BK))
    return _chunks(K, S) if S >= 2 else (1, K)


def _last_round(M, N, K, a_mode, ncu):
    """Tall products on 128-row tiles: the row tiles beyond whole rounds of 2 ncu workgroups, when they fill at most 0.7 of
    a round, run with K split c ways (cost ceil(tiles c / slots) / c + 0.04 c of a round, taken when it beats 1 by 0.05).
    -> (rows of the whole rounds, S, kchunk) or None."""
    f = np.float32
    if a_mode != 0:
        return None
    slots, ct, rt = 2 * ncu, _cdiv(N, 128), _cdiv(M, 128)
    if ct > slots or rt * ct <= slots:
        return None
    rem = rt % (slots // ct)
    if rem == 0 or 10 * rem * ct > 7 * slots:
        return None
    S, best = 1, f(1.0)
    for c in range(2, 9):
        if c > K // 64:
            break
        cost = f(_cdiv(rem * ct * c, slots)) / f(c) + f(0.04) * f(c)
        if cost < best - f(0.05):
            best, S = cost, c
    if S < 2:
        return None
    S, kc = _chunks(K, S)
    return ((rt - rem) * 128, S, kc) if S >= 2 else None


def _small_tiles(M, N, K, a_mode, ncu):
    """k_gemm64n: at most 2048 rows, K >= 256, below k_gemm64's 3 ncu / 2 tiles of 64 x 128 and at least 16 tiles of
    64 x 64; K split to about one workgroup per CU with at least eight slices per split.  -> (S, kchunk) or None."""
    if a_mode != 0 or M > 2048 or K < 256 or K % BK or N % 4:
        return None
    if _cdiv(M, 64) * _cdiv(N, 128) >= 3 * ncu // 2:
        return None
    t = _cdiv(M, 64) * _cdiv(N, 64)
    if t < 16:
        return None
    return _chunks(K, max(1, min((ncu + t // 2) // t, K // 256)))


def gemm_route(M, N, K, a_mode=0, b_mode=0, lda=None, ldb=None, ldc=None, act=0, residual=False, accumulate=False, aux_mode=0,
               workspace=True, bucketed=False, aligned16=True, ncu=NCU):
    """What mil_gemm_route answers for these arguments, field by field (ROUTE_FIELDS)."""
    lda = (K if a_mode == 0 else M) if lda is None else lda
    ldb = (K if b_mode == 0 else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    r = dict(kernel=None, S=1, kchunk=K, rows_main=0, main_kernel=0, rows_honoured=0, need=0)
    plain = not residual and not accumulate and aux_mode == 0 and act <= 2
    if (a_mode, b_mode) == (0, 0) and plain and ldc >= N and aligned16 and not bucketed and _nt2_shape_ok(lda, ldb, M, N, K) \
            and _nt2_fills(M, N, ncu):
        return dict(r, kernel="NT2")
    if a_mode == 0 and K >= 256:
        t64 = _cdiv(M, 64) * _cdiv(N, 128)
        if t64 >= 3 * ncu // 2 or (bucketed and t64 >= ncu // 2 and N % 4 == 0):
            return dict(r, kernel="G64", rows_honoured=1)
    small = _small_tiles(M, N, K, a_mode, ncu)
    if small is not None and (small[0] == 1 or workspace):
        return dict(r, kernel="G64N", S=small[0], kchunk=small[1], need=small[0] * M * N if small[0] > 1 else 0)
    tail = _last_round(M, N, K, a_mode, ncu) if workspace else None
    if tail is not None:
        rows_main, S, kc = tail
        main = gemm_route(rows_main, N, K, a_mode, b_mode, lda, ldb, ldc, act, residual, accumulate, aux_mode, False, False,
                          aligned16, ncu)
        return dict(r, kernel="TAIL", S=S, kchunk=kc, rows_main=rows_main, main_kernel=KERNELS.index(main["kernel"]),
                    need=S * (M - rows_main) * N)
    r["kernel"] = "TN" if a_mode == 1 else ("NT", "NN")[b_mode]
    if workspace:
        S, kc = _split_big_tile(M, N, K, a_mode, ncu)
        if S > 1:
            r.update(S=S, kchunk=kc, need=S * M * N)
    return r


def _tn2_split(rows, N, K, ncu):
    """k_gemm_tn2: one 512-thread workgroup per CU over the 128 x 128 tiles, the rows in chunks of whole 64."""
    tiles = (N // 128) * (K // 128)
    kc = max(64, _up(_cdiv(rows, max(1, ncu // tiles)), 64))
    return _cdiv(rows, kc), kc


def bwd_params_route(rows, n_out, k_in, lddy=None, ldy=0, ldx=None, aligned16=True, ncu=NCU):
    """What mil_linear_bwd_params_route answers: k_gemm_tn2 from 4096 rows with whole 128 x 128 tiles, row chunks of at least
    512, 3/4 of the chip busy (4 S tiles >= 3 ncu) and 31-bit offsets; k_gemm<1,1,true> otherwise."""
    lddy = n_out if lddy is None else lddy
    ldx = k_in if ldx is None else ldx
    r = dict(kernel="TN_AX", S=1, kchunk=rows, rows_main=0, main_kernel=0, rows_honoured=0)
    tn2 = aligned16 and rows >= 4096 and n_out % 128 == 0 and k_in % 128 == 0
    if tn2:
        S, kc = _tn2_split(rows, n_out, k_in, ncu)
        tn2 = (kc >= 512 and 4 * S * (n_out // 128) * (k_in // 128) >= 3 * ncu and kc * max(lddy, ldx) * 4 < 0x7fff0000
               and kc * (ldy or lddy) * 4 < 0x7fff0000)
    if tn2:
        r.update(kernel="TN2", S=S, kchunk=kc, rows_honoured=1)
    else:
        S, kc = _split_big_tile(n_out, k_in, rows, 1, ncu)
        r.update(S=S, kchunk=kc)
    r["need"] = r["S"] * n_out * k_in + r["S"] * n_out
    return r


# --------------------------------------------------------------------------- arithmetic
def f32exact(t):
    return t.float().double()


def act_fwd(v, act):
    return (v, torch.tanh(v), torch.relu(v), v * torch.sigmoid(QG * v))[act] if act else v


def dgelu(p):
    s = torch.sigmoid(QG * p)
    return s * (1 + QG * p * (1 - s))


def dact(g, y, act):
    """g act'(.) from the activation OUTPUT y (tanh, relu)."""
    if act == 1:
        return g * (1 - y * y)
    if act == 2:
        return g * (y > 0).to(g.dtype)
    return g


def _walk(Aop, Bop, k0, k1):
    """sum over the 32-deep slices of [k0, k1), one after the other."""
    acc = torch.zeros(Aop.shape[0], Bop.shape[1], dtype=Aop.dtype)
    for k in range(k0, k1, BK):
        acc = acc + Aop[:, k:min(k + BK, k1)] @ Bop[k:min(k + BK, k1)]
    return acc


def _epilogue(v, bias, act, res, c_old, aux_in, aux_mode, mutate, bias_times=1):
    """-> (C, aux to store or None): v + bias, the aux step, act, + residual, + C."""
    if bias is not None:
        v = v + bias * bias_times
    store = None
    if aux_mode == 1:
        store = act_fwd(v, act) if mutate == "aux1_post" else v
    elif aux_mode == 2:
        v = v * dgelu(v if mutate == "aux2_from_out" else aux_in)
    if mutate != "act_per_partial":
        v = act_fwd(v, act)
    if res is not None:
        v = v + res
    if c_old is not None and mutate != "acc_overwrite":
        v = v + c_old
    return v, store


def _rows_product(Aop, Bop, K, S, kc, bias, act, res, c_old, aux_in, aux_mode, mutate):
    """One launch (+ fold) over the rows of Aop: S == 1 the epilogue in the product kernel, else per-split partial sums, the
    fold in split order and the epilogue there."""
    kend = K - BK if mutate == "k_last_slice" else K
    if S == 1:
        return _epilogue(_walk(Aop, Bop, 0, kend), bias, act, res, c_old, aux_in, aux_mode, mutate)
    v = torch.zeros(Aop.shape[0], Bop.shape[1], dtype=Aop.dtype)
    for s in range(S):
        if mutate == "split_missing" and s == 1:
            continue
        part = _walk(Aop, Bop, s * kc, min(kend, (s + 1) * kc))
        v = v + (act_fwd(part, act) if mutate == "act_per_partial" else part)
    return _epilogue(v, bias, act, res, c_old, aux_in, aux_mode, mutate, S if mutate == "bias_per_split" else 1)


def gemm(A, B, a_mode, b_mode, bias, act, residual, accumulate_into, aux, aux_mode, route, rows=None, mutate=None, ld=None):
    """{"C": [M, ld], "aux": [M, ld] (aux_mode 1)}: whole buffers.  C starts as accumulate_into (its first N columns) or the
    sentinel, aux (mode 1) as the sentinel; aux (mode 2) is the saved pre-activation [M, N].  rows: the true row count of a
    bucket (rows_dev) - rows from 64 ceil(rows / 64) on come out zero (no accumulate), those between rows and that boundary
    are whatever the kernel makes of A's stale rows (here: the same product; the tests do not compare them)."""
    assert mutate is None or mutate in GEMM_MUTATIONS, mutate
    dt = A.dtype
    Aop = A if a_mode == 0 else A.t()
    Bop = B.t() if b_mode == 0 else B
    M, K = Aop.shape
    N = Bop.shape[1]
    ld = N if ld is None else ld
    C = torch.full((M, ld), SENT, dtype=dt)
    c_old = None
    if accumulate_into is not None:
        C[:, :N] = accumulate_into
        c_old = accumulate_into
    auxbuf = torch.full((M, ld), SENT, dtype=dt) if aux_mode == 1 else None
    aux_in = aux if aux_mode == 2 else None
    sl = lambda t, a, b: None if t is None else t[a:b]                                      # noqa: E731
    S, kc = route["S"], route["kchunk"]

    def launch(r0, r1, S_, kc_, o0=None, res0=None, aux0=None):
        """rows [r0, r1) of the product; o0 / res0 / aux0: where their C / residual / aux rows start (default r0)."""
        o0, res0, aux0 = (r0 if v is None else v for v in (o0, res0, aux0))
        n = r1 - r0
        v, store = _rows_product(Aop[r0:r1], Bop, K, S_, kc_, bias, act, sl(residual, res0, res0 + n), sl(c_old, o0, o0 + n),
                                 sl(aux_in, aux0, aux0 + n), aux_mode, mutate)
        C[o0:o0 + n, :N] = v
        if store is not None:
            auxbuf[aux0:aux0 + n, :N] = store

    if route["kernel"] == "TAIL":
        rm = route["rows_main"]
        launch(0, rm, 1, K)
        launch(rm, M, S, kc, 0 if mutate == "tail_c_offset" else None, 0 if mutate == "tail_res_offset" else None,
               0 if mutate == "tail_aux_offset" else None)
    else:
        launch(0, M, S, kc)
    if mutate == "last_row":
        C[M - 1, :N] = SENT if c_old is None else c_old[M - 1]
    if mutate == "col_shift":
        tc = 64 if route["kernel"] == "G64N" else 128
        j0 = tc * ((N - 1) // tc)
        d = min(j0 + tc - N, j0)
        C[:, j0:N] = C[:, j0 - d:N - d].clone()
    if mutate == "guard_write" and ld > N:
        C[:, N] = C[:, N - 1]
    if rows is not None and accumulate_into is None:
        bnd = _up(rows, 64)
        if mutate != "stale_behind":
            C[bnd:, :N] = 0
        if mutate == "zero_last_group":
            C[64 * ((rows - 1) // 64):rows, :N] = 0
    out = {"C": C}
    if auxbuf is not None:
        out["aux"] = auxbuf
    return out


def bwd_params(dy, y, act, x, route, rows=None, accumulate_into=None, mutate=None, ld=None):
    """{"dW": [n_out, ld], "db": [n_out]}: dW (+)= (dy act'(y))^T x, db (+)= its column sums, as per-chunk partial sums over
    the rows (32 at a time) folded in chunk order.  rows: the true row count - k_gemm_tn2 spreads those over its S chunks and
    reads nothing behind them; k_gemm<1,1,true> walks the capacity and relies on zero gradients there."""
    assert mutate is None or mutate in BWD_MUTATIONS, mutate
    cap, n_out = dy.shape
    k_in = x.shape[1]
    ld = k_in if ld is None else ld
    g = dact(dy, dy if mutate == "dact_from_dy" else y, act) if act else dy
    S, kc, n = route["S"], route["kchunk"], cap
    if route["kernel"] == "TN2" and rows is not None and mutate != "rows_ignored":
        n = min(cap, rows)
        kc = max(2 * BK, _up(_cdiv(n, S), 2 * BK))
    dW = torch.zeros(n_out, k_in, dtype=dy.dtype)
    db = torch.zeros(n_out, dtype=dy.dtype)
    for s in range(S):
        r0, r1 = min(n, s * kc), min(n, (s + 1) * kc)
        if mutate == "dw_rows_mult" and s == S - 1:
            r1 = r0 + (r1 - r0) // kc * kc
        part = torch.zeros_like(dW)
        for r in range(r0, r1, BK):
            part = part + g[r:min(r + BK, r1)].t() @ x[r:min(r + BK, r1)]
        dW = dW + part
        if not (mutate == "db_last_split" and s == S - 1):
            db = db + g[r0:r1].sum(0)
    out = torch.full((n_out, ld), SENT, dtype=dy.dtype)
    if accumulate_into is not None and mutate != "acc_overwrite":
        dW, db = dW + accumulate_into[0], db + accumulate_into[1]
    out[:, :k_in] = dW
    if mutate == "guard_write" and ld > k_in:
        out[:, k_in] = out[:, k_in - 1]
    return {"dW": out, "db": db}


def colsum(Y, accumulate_into=None, mutate=None):
    """out[j] (+)= sum_i Y[i][j]: 256-row chunks folded in order when there is more than one."""
    M = Y.shape[0]
    v = torch.zeros(Y.shape[1], dtype=Y.dtype)
    for r in range(0, M - (M % 256 if mutate == "last_chunk" and M > 256 else 0), 256):
        v = v + Y[r:r + 256].sum(0)
    return {"out": v if accumulate_into is None or mutate == "acc_overwrite" else v + accumulate_into}


def act_bwd(dy, y, act, mutate=None):
    return {"dpre": dact(dy, dy if mutate == "dact_from_dy" else y, act)}


def _mid_walk(Aop, Bop, ks, drop8=False):
    """k_mid: the K groups of 8 dealt to ks waves in contiguous runs, each wave's sum, then the fold in wave order."""
    K = Aop.shape[1]
    kend = K - 8 if drop8 else K
    per = _cdiv(_cdiv(K, 8), ks) * 8
    acc = torch.zeros(Aop.shape[0], Bop.shape[1], dtype=Aop.dtype)
    for w in range(ks):
        k0, k1 = min(kend, w * per), min(kend, (w + 1) * per)
        acc = acc + Aop[:, k0:k1] @ Bop[k0:k1]
    return acc


def mid_ks(rows, cols, ncu=NCU):
    """waves that split K in a k_mid workgroup: 8 on 32 x 32 tiles (up to 4 ncu of them), 2 on 64 x 64."""
    return 8 if _cdiv(rows, 32) * _cdiv(cols, 32) <= 4 * ncu else 2


def mid_fwd(x, W, b, act, residual, mutate=None, ld=None, ncu=NCU):
    assert mutate is None or mutate in MID_MUTATIONS, mutate
    M, N = x.shape[0], W.shape[0]
    v = _mid_walk(x, W.t(), mid_ks(M, N, ncu), mutate == "k_last8")
    if b is not None:
        v = v + b
    v = act_fwd(v, act)
    if residual is not None:
        v = v + residual
    y = torch.full((M, N if ld is None else ld), SENT, dtype=x.dtype)
    y[:, :N] = v
    if mutate == "last_row":
        y[M - 1, :N] = SENT
    return {"y": y}


def mid_bwd(dy, yv, act, x, W, mutate=None, ncu=NCU):
    """dx = dpre W (contraction over n_out), dW = dpre^T x (over the rows, in groups of 8), db = column sums of dpre."""
    assert mutate is None or mutate in MID_MUTATIONS, mutate
    M, N = dy.shape
    K = x.shape[1]
    g = dact(dy, dy if mutate == "dact_from_dy" else yv, act) if act else dy
    gw = g[:M - M % 8] if mutate == "dw_rows_mult" else g
    xw = x[:gw.shape[0]]
    return {"dx": _mid_walk(g, W, mid_ks(M, K, ncu), mutate == "k_last8"), "dW": _mid_walk(gw.t(), xw, mid_ks(N, K, ncu)),
            "db": gw.sum(0)}


# --------------------------------------------------------------------------- operands
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 11) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=4)
def gemm_case(M, N, K):
    """float32-exact operands in float64: A [M, K] (mean 0.25), W [N, K] / sqrt(K), bias."""
    g = _gen(M, N, K)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    c = dict(A=r(M, K) + 0.25, W=r(N, K) / math.sqrt(K), bias=0.5 * r(N))
    return {n: f32exact(t) for n, t in c.items()}


def gemm_extra(which, M, N, K):
    """The optional [M, N] operands, each from its own seed: 1 residual, 2 C0 (what accumulate adds to), 3 pre (the saved
    pre-activation of aux mode 2)."""
    return f32exact(torch.randn((M, N), generator=_gen(M, N, K, which), dtype=torch.float64))


@functools.lru_cache(maxsize=4)
def bwd_case(rows, N, K, act):
    """dy, x, the saved output y = act(pre) [rows, N] (float32 rounding of the float64 value), dW0 / db0 for accumulate."""
    g = _gen(rows, N, K, act, 5)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    c = dict(dy=0.1 * r(rows, N), x=r(rows, K) + 0.25, y=act_fwd(r(rows, N), act), dW0=r(N, K), db0=r(N), W=r(N, K) / math.sqrt(K),
             b=0.5 * r(N), residual=r(rows, N))
    return {n: f32exact(t) for n, t in c.items()}


def _run(entry, kernel, M, N, K, **kw):
    d = dict(entry=entry, kernel=kernel, M=M, N=N, K=K, a_mode=0, b_mode=0, bias=False, act=0, res=False, acc=False, aux=0, ws=True,
             rows=None, strided=False)
    d["b_mode"] = int(kernel == "NN")
    d.update(kw)
    return d


# The smallest shapes that reach each kernel at 256 CUs (chosen with mil_gemm_route / the rules above, asserted against the
# device's own answer in tests/test_gpu_linear_stages.py):
#   G64   t64 = ceil(M / 64) ceil(N / 128) >= 384, K >= 256: 24 row tiles x N = 2048 (M 1473 .. 1536), 77 x N = 520 (M >= 4865);
#         bucketed from t64 = 128: M = 2048 x N = 512
#   G64N  M <= 2048, >= 16 tiles of 64 x 64: S = 1 from 172 tiles (11 x N = 1024), S > 1 below (130 x 520: 27 tiles)
#   NT2   224 .. 256 tiles of 256 x 256: 28 row tiles x N = 2048 (M 6913 .. 7168), K = 64
#   TAIL  128 <= K < 256 (from K = 256 on k_gemm64 takes every shape of more than a round), more than 512 tiles of 128 x 128
#         and at most 16 row tiles over: N = 2048 from M = 4097, N = 2056 (17 column tiles, 30 row tiles per round) from 3841
#   NT / NN  K < 256 one chunk; K >= 256 and fewer than 16 tiles of 64 x 64: split, or one chunk without a workspace
#   TN    always split (ops.gemm(a_mode=1) for dW)
#   TN2   rows >= 4096 with chunks of >= 512 rows: 512 x 1024 outputs (8 chunks); TN_AX everything else
def gemm_runs():
    R = lambda *a, **k: _run("gemm", *a, **k)                                                # noqa: E731
    out = [
        R("G64", 1500, 2048, 256, bias=True, act=1),
        R("G64", 1473, 2048, 512, b_mode=1, res=True, strided=True),
        R("G64", 4870, 520, 256, b_mode=1, acc=True),
        R("G64", 4870, 520, 256, bias=True, act=3, aux=1, strided=True),
        R("G64", 1500, 2048, 256, b_mode=1, aux=2),
        R("G64", 1536, 2048, 256, bias=True, act=2),
        R("G64N", 700, 1024, 256, bias=True, act=1),
        R("G64N", 700, 1028, 256, b_mode=1, res=True, strided=True),
        R("G64N", 130, 520, 512, bias=True, act=3, aux=1, strided=True),
        R("G64N", 130, 520, 512, b_mode=1, bias=True, res=True, acc=True),
        R("G64N", 130, 520, 512, b_mode=1, aux=2),
        R("G64N", 130, 520, 2048, bias=True, act=2),
        R("G64N", 130, 520, 512, bias=True, act=1),
        R("NT2", 7168, 2048, 64, bias=True, act=1),
        R("NT2", 7000, 2048, 64, bias=True, act=2, strided=True),
        R("NT2", 6913, 2048, 96),
        R("TAIL", 4226, 2048, 128, bias=True, act=1),
        R("TAIL", 4226, 2048, 224, b_mode=1, bias=True, res=True, acc=True),
        R("TAIL", 3970, 2056, 160, bias=True, act=3, aux=1, strided=True),
        R("TAIL", 3970, 2056, 128, b_mode=1, aux=2),
        R("TAIL", 4226, 2048, 128, bias=True, act=2, res=False),
        R("NT", 200, 132, 64, bias=True, act=1, strided=True),
        R("NT", 300, 264, 224, bias=True, act=3, aux=1, res=True),
        R("NN", 200, 132, 96, res=True, acc=True, strided=True),
        R("NN", 129, 260, 32, aux=2, bias=True, act=2),
        R("NT", 50, 512, 256, bias=True, act=1),
        R("NT", 50, 520, 512, bias=True, act=3, aux=1, res=True, acc=True, strided=True),
        R("NN", 50, 516, 256, bias=True, act=2, res=True),
        R("NN", 50, 512, 256, aux=2, acc=True),
        R("NT", 50, 512, 256, bias=True, act=1, ws=False),
        R("NN", 50, 516, 256, bias=True, act=2, res=True, ws=False),
        R("TN", 512, 260, 300, a_mode=1, b_mode=1),
        R("TN", 132, 128, 1000, a_mode=1, b_mode=1, acc=True, strided=True),
    ]
    for rows in (1, 1024, 1025, 2048):                      # bucketed: rows_dev at 1, 64 k, 64 k + 1 and M
        out.append(R("G64", 2048, 512, 256, bias=True, act=1, rows=rows, b_mode=rows % 2))
    for rows in (1, 128, 129, 200):                         # the other routes clear the rows behind the bucket afterwards
        out.append(R("NT", 200, 132, 64, bias=True, act=2, rows=rows, strided=rows == 129))
    out.append(R("G64N", 700, 1024, 256, bias=True, rows=321))
    out.append(R("NN", 50, 512, 256, rows=33))
    return out


def bwd_runs():
    R = lambda *a, **k: _run("bwd_params", *a, **k)                                          # noqa: E731
    return [
        R("TN_AX", 65, 132, 64, act=1),
        R("TN_AX", 1000, 2048, 512, act=2, strided=True),
        R("TN_AX", 4095, 512, 256, act=0, acc=True),
        R("TN_AX", 300, 512, 768, act=1, rows=300),
        R("TN2", 4096, 512, 1024, act=1),
        R("TN2", 4099, 1024, 512, act=2, acc=True, strided=True),
        R("TN2", 4096, 512, 1024, act=0, rows=1),
        R("TN2", 4200, 512, 1024, act=1, rows=2049, acc=True),
        R("TN2", 4200, 512, 1024, act=2, rows=4200),
    ]


def other_runs():
    return [
        _run("colsum", "", 300, 132, 0), _run("colsum", "", 300, 132, 0, acc=True), _run("colsum", "", 1000, 520, 0, acc=True),
        _run("colsum", "", 256, 64, 0), _run("colsum", "", 1000, 520, 0),
        _run("act_bwd", "", 77, 130, 0, act=1), _run("act_bwd", "", 1001, 257, 0, act=2),
        _run("mid_fwd", "k8", 70, 136, 64, bias=True, act=1), _run("mid_fwd", "k8", 999, 136, 72, bias=True, act=3, strided=True),
        _run("mid_fwd", "k2", 1000, 1056, 64, bias=True, act=2), _run("mid_fwd", "k8", 333, 512, 512, res=True, bias=True),
        _run("mid_bwd", "k8", 70, 136, 64, act=1), _run("mid_bwd", "k8", 999, 136, 72, act=2), _run("mid_bwd", "k2", 1000, 1056, 1056, act=0),
        _run("mid_bwd", "k2", 1001, 1056, 1056, act=1),
    ]


def lds(run):
    """Leading dimensions of a run's operands: dense, or GUARD floats wider (strided)."""
    pad = GUARD if run["strided"] else 0
    M, N, K = run["M"], run["N"], run["K"]
    if run["entry"] == "gemm":
        return dict(lda=(K if run["a_mode"] == 0 else M) + pad, ldb=(K if run["b_mode"] == 0 else N) + pad, ldc=N + pad)
    return dict(lddy=N + pad, ldy=(N + pad) if run["act"] else 0, ldx=K + pad)


def _route_args(run):
    if run["entry"] == "gemm":
        return (run["M"], run["N"], run["K"], run["a_mode"], run["b_mode"]), dict(
            lds(run), act=run["act"], residual=run["res"], accumulate=run["acc"], aux_mode=run["aux"], workspace=run["ws"],
            bucketed=run["rows"] is not None)
    return (run["M"], run["N"], run["K"]), lds(run)


def route_of(run, ncu=NCU):
    """The rules' route for a gemm / bwd_params run."""
    a, kw = _route_args(run)
    return (gemm_route if run["entry"] == "gemm" else bwd_params_route)(*a, ncu=ncu, **kw)


def run_inputs(run):
    """The run's operands, float32-exact in float64 (the GPU test uploads their float32 form)."""
    M, N, K = run["M"], run["N"], run["K"]
    if run["entry"] == "gemm":
        if run["a_mode"] == 1:                                  # dW = dy^T x: A = dy [K rows, M], B = x [K rows, N]
            c = bwd_case(K, M, N, 0)
            return dict(A=c["dy"], B=c["x"], bias=None, residual=None, C0=c["dW0"] if run["acc"] else None, pre=None)
        c = gemm_case(M, N, K)
        A = c["A"]
        if run["rows"] is not None:                             # stale rows behind the bucket's true count
            A = A.clone()
            A[run["rows"]:] = 3.0 * A[run["rows"]:] + 1.0
        return dict(A=A, B=c["W"] if run["b_mode"] == 0 else c["W"].t().contiguous(), bias=c["bias"] if run["bias"] else None,
                    residual=gemm_extra(1, M, N, K) if run["res"] else None, C0=gemm_extra(2, M, N, K) if run["acc"] else None,
                    pre=gemm_extra(3, M, N, K) if run["aux"] == 2 else None)
    if run["entry"] in ("bwd_params", "mid_bwd", "mid_fwd"):
        c = dict(bwd_case(M, N, K, run["act"] if run["entry"] != "mid_fwd" else 0))
        if run["entry"] == "bwd_params" and run["rows"] is not None and run["kernel"] == "TN_AX":
            c["dy"] = c["dy"].clone()
            c["dy"][run["rows"]:] = 0                           # the contract of the kernel that walks the capacity
        return c
    g = _gen(M, N, 3)
    r = lambda *s: f32exact(torch.randn(s, generator=g, dtype=torch.float64))                # noqa: E731
    return dict(Y=r(M, N) + 0.1, out0=r(N), dy=r(M, N), y=act_fwd(r(M, N), run["act"]))


def restate(run, dtype=torch.float64, mutate=None, route=None, inputs=None, ncu=NCU):
    """The run's outputs in `dtype`; route: the library's answer (GPU test), default the rules' own; inputs: run_inputs(run)
    when the caller holds them already."""
    M, N, K = run["M"], run["N"], run["K"]
    c = {n: (None if v is None else v.to(dtype)) for n, v in (inputs or run_inputs(run)).items()}
    pad = GUARD if run["strided"] else 0
    e = run["entry"]
    if e == "gemm":
        return gemm(c["A"], c["B"], run["a_mode"], run["b_mode"], c["bias"], run["act"], c["residual"], c["C0"], c["pre"], run["aux"],
                    route or route_of(run), run["rows"], mutate, N + pad)
    if e == "bwd_params":
        return bwd_params(c["dy"], c["y"], run["act"], c["x"], route or route_of(run), run["rows"],
                          (c["dW0"], c["db0"]) if run["acc"] else None, mutate, K + pad)
    if e == "colsum":
        return colsum(c["Y"], c["out0"] if run["acc"] else None, mutate)
    if e == "act_bwd":
        return act_bwd(c["dy"], c["y"], run["act"], mutate)
    if e == "mid_fwd":
        return mid_fwd(c["x"], c["W"], c["b"] if run["bias"] else None, run["act"], c["residual"] if run["res"] else None, mutate, N + pad,
                       ncu)
    return mid_bwd(c["dy"], c["y"], run["act"], c["x"], c["W"], mutate, ncu)


# --------------------------------------------------------------------------- blocks
def _tile_rows(kernel):
    return {"NT2": 256, "G64": 64, "G64N": 64}.get(kernel, 128)


def out_blocks(M, N, ld, kernel="NT", rows_main=0, rows=None, acc=False):
    """Blocks of an output buffer [M, ld]: the first 64 rows, the last (ragged) row tile, the last row, the rows of the split
    last round, the last clamped column tile, the guard columns, the whole.  Bucketed (rows given): the true rows, the true
    rows of the last 64-row group, the rows behind the 64-row boundary (zero) - the rows between the count and the boundary are
    unspecified by the header and belong to no block but the guard."""
    cols = slice(0, N)
    out = {}
    tr, tc = _tile_rows(kernel), (64 if kernel == "G64N" else 128)
    if rows is None:
        out.update(all=(slice(None), cols), r0=(slice(0, min(64, M)), cols), rlast=(slice(tr * ((M - 1) // tr), M), cols),
                   lastrow=(slice(M - 1, M), cols))
        if rows_main:
            out["tail"] = (slice(rows_main, M), cols)
            out["tail0"] = (slice(0, M - rows_main), cols)
    else:
        bnd = _up(rows, 64)
        out.update(true=(slice(0, rows), cols), truelast=(slice(64 * ((rows - 1) // 64), rows), cols))
        if bnd < M and not acc:
            out["behind"] = (slice(bnd, M), cols)
    if N % tc:
        rsel = slice(None) if rows is None else slice(0, rows)
        out["clast"] = (rsel, slice(tc * ((N - 1) // tc), N))
    if ld > N:
        out["guard"] = (slice(None), slice(N, ld))
    return out


def dw_blocks(N, K, ld):
    out = {"all": (slice(None), slice(0, K)), "t0": (slice(0, min(128, N)), slice(0, min(128, K))),
           "tL": (slice(128 * ((N - 1) // 128), N), slice(128 * ((K - 1) // 128), K))}
    if ld > K:
        out["guard"] = (slice(None), slice(K, ld))
    return out


def vec_blocks(n):
    return {"all": (Ellipsis,), "last4": (slice(n - 4, n),)}


def blocks_of(run, route=None):
    M, N, K = run["M"], run["N"], run["K"]
    pad = GUARD if run["strided"] else 0
    e = run["entry"]
    if e == "gemm":
        route = route or route_of(run)
        b = out_blocks(M, N, N + pad, route["kernel"], route["rows_main"], run["rows"], run["acc"])
        return {"C": b, "aux": b} if run["aux"] == 1 else {"C": b}
    if e == "bwd_params":
        return {"dW": dw_blocks(N, K, K + pad), "db": vec_blocks(N)}
    if e == "colsum":
        return {"out": vec_blocks(N)}
    if e == "act_bwd":
        return {"dpre": {"all": (Ellipsis,), "lastrow": (slice(M - 1, M),)}}
    if e == "mid_fwd":
        return {"y": out_blocks(M, N, N + pad, "G64")}
    return {"dx": out_blocks(M, K, K, "G64"), "dW": dw_blocks(N, K, K), "db": vec_blocks(N)}


def expected(name):
    """What a block's reference must be: "sentinel" (guard columns), "zero" (behind the bucket) or None (non-zero, finite)."""
    return {"guard": "sentinel", "behind": "zero"}.get(name)


def tag(run):
    keep = {k: v for k, v in run.items() if (v not in (False, None, 0, "") and k != "ws") or k in ("M", "N", "K")}
    if not run["ws"]:
        keep["workspace"] = "none"
    return " ".join(f"{k} {ACT_NAMES[v] if k == 'act' else v}" for k, v in keep.items())


# k of bound(e32, k) per entry: the smallest integer k with gpu_err <= k max(e32, 1e-7) on every block of the entry's runs on an
# MI355X, rounded up to the next of 2, 4, 8, 16 (cap K_CAP); beside it the largest ratio measured (the table "tiled linear
# stages" in docs/lab_notes.md)
K_STAGE = {"gemm": 8,          # 5.97  G64N 700 x 1028 x 256 NN + residual, strided, C.clast
           "bwd_params": 4,    # 2.50  TN2 4096 rows, 512 x 1024, tanh, dW.t0
           "colsum": 2,        # 1.00  1000 x 520 accumulate, out.all
           "act_bwd": 2,       # 0.69  77 x 130 tanh, dpre.lastrow
           "mid_fwd": 2,       # 1.62  64 x 64 tiles, 1000 x 1056 x 64 relu, y.lastrow
           "mid_bwd": 4}       # 3.68  64 x 64 tiles, 1000 x 1056 x 1056, db.all


def hold(case, got, ref, r32, blocks, stage):
    """Every block of every tensor of `got` within bound(e32, K_STAGE[stage]) of `ref`, the guard blocks met exactly; prints
    the worst block first."""
    bad, worst, wname = [], 0.0, ""
    for t in got:
        e32, eg = block_err(r32[t], ref[t], blocks[t]), block_err(got[t], ref[t], blocks[t])
        for b, e in eg.items():
            ratio = e / max(e32[b], FLOOR)
            if ratio > worst:
                worst, wname = ratio, f"{t}.{b}"
            if not e <= (0.0 if expected(b) else bound(e32[b], K_STAGE[stage])):
                bad.append((t, b, e, e32[b]))
    print(f"\nRATIO | {stage} | {case} | {wname} | {worst:.2f}", end="")
    assert not bad, (stage, case, bad[:8])
    return worst


# --------------------------------------------------------------------------- the library's own statement of the routes
def _lib_route(p):
    d = {n: getattr(p, n) for n in ROUTE_FIELDS if n != "need"}
    d["kernel"] = KERNELS[p.kernel]
    d["need"] = int(p.workspace_floats)
    return d


def lib_gemm_route(M, N, K, a_mode=0, b_mode=0, lda=None, ldb=None, ldc=None, act=0, residual=False, accumulate=False, aux_mode=0,
                   workspace=True, bucketed=False, aligned16=True, ncu=NCU):
    """mil_gemm_route (the plan the launches execute) in gemm_route's terms; ncu = 0: the current device's CU count."""
    import ctypes
    from mil_amd import _lib
    lda = (K if a_mode == 0 else M) if lda is None else lda
    ldb = (K if b_mode == 0 else N) if ldb is None else ldb
    p = _lib.GemmPlan()
    rc = _lib.lib().mil_gemm_route(M, N, K, a_mode, b_mode, lda, ldb, N if ldc is None else ldc, act, int(residual), int(accumulate),
                                   aux_mode, int(workspace), int(bucketed), int(aligned16), ncu, ctypes.byref(p))
    assert rc == 0, (rc, M, N, K, a_mode, b_mode)
    return _lib_route(p)


def lib_bwd_params_route(rows, n_out, k_in, lddy=None, ldy=0, ldx=None, aligned16=True, ncu=NCU):
    import ctypes
    from mil_amd import _lib
    p = _lib.GemmPlan()
    rc = _lib.lib().mil_linear_bwd_params_route(rows, n_out, k_in, n_out if lddy is None else lddy, ldy, k_in if ldx is None else ldx,
                                                int(aligned16), ncu, ctypes.byref(p))
    assert rc == 0, (rc, rows, n_out, k_in)
    return _lib_route(p)


def lib_route_of(run, ncu=0):
    """route_of(run) as the library states it for the current device."""
    a, kw = _route_args(run)
    return (lib_gemm_route if run["entry"] == "gemm" else lib_bwd_params_route)(*a, ncu=ncu, **kw)
