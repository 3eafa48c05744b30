"""Restatements of the token-side few-rows entries (csrc/small_linear.hip) for any float dtype: y = act((x + x2) W^T + b) +
residual, its backward on a sum of up to four gradients, the n-split partial input gradient, the LayerNorm folded into the
next layer's forward and into the previous layer's input gradient, the grouped weight gradient and the four-way sum.
float64 is the reference, the same code in float32 on the CPU gives `e32`; mutate= plants one error
(tests/test_small_linear_sensitivity_host.py shows that the per-block bounds of tests/test_gpu_small_linear_stages.py see
each of them).  Every backward takes the forward's saved tensors as arguments, so the float32 rounding of the float64
forward can be fed to the entry and to both dtypes alike.  Test-side helper: nothing here reads the code under test."""
import functools
import math

import numpy as np
import torch

from transmil_ref import FLOOR, K_CAP, block_err, bound  # noqa: F401  (re-exported to the two test files)

E = 512                              # the LayerNorm's width (SLN_E)
QG = 1.702
EPS = 1e-5
LOW_STD = 0.1                        # spread of row 2 of the norm's input (mean 30): where a one-pass variance cancels most
KCH = 512                            # operand chunk of the kernels' contraction
ACT_NAMES = ("none", "tanh", "relu", "quickgelu", "sigmoid")

FWD_MUTATIONS = ("k_last16", "k_chunk2", "xin_x")
BWD_MUTATIONS = ("odd_last_row", "rows32", "k_last16", "k_chunk2", "skip_dy3", "missing_w1", "dysum_after", "gelu_from_out",
                 "sigmoid_y")
SPLIT_MUTATIONS = ("split_range",)
LN_FWD_MUTATIONS = ("onepass", "eps_outside", "var_e1", "xin_x")
LN_BWD_MUTATIONS = ("rows32", "skip_g3", "skip_g5", "missing_w1", "no_xhat_term", "no_gamma")


def f32exact(t):
    return t.float().double()


def act_fwd(v, act):
    if act == 1:
        return torch.tanh(v)
    if act == 2:
        return torch.relu(v)
    if act == 3:
        return v * torch.sigmoid(QG * v)
    if act == 4:
        return torch.sigmoid(v)
    return v


def dact(g, saved, act, mutate=None):
    """g act'(.): from the activation OUTPUT for tanh, relu, sigmoid, from the PRE-activation for QuickGELU."""
    if act == 1:
        return g * (1 - saved * saved)
    if act == 2:
        return g * (saved > 0).to(g.dtype)
    if act == 3:
        s = torch.sigmoid(QG * saved)
        return g * s * (1 + QG * saved * (1 - s))
    if act == 4:
        return g * saved if mutate == "sigmoid_y" else g * saved * (1 - saved)
    return g


def _kmask(n, mutate, dtype):
    """1 for the terms that enter a contraction of length n.  "k_last16": the last 16 do not; "k_chunk2": those of the second
    512-chunk do not."""
    w = torch.ones(n, dtype=dtype)
    if mutate == "k_last16":
        w[n - 16:] = 0
    if mutate == "k_chunk2":
        w[KCH:2 * KCH] = 0
    return w


def _row_mask(M, mutate, dtype):
    """1 for the rows that enter a contraction over the rows.  "odd_last_row": the last of an odd count does not (the second
    of a row pair); "rows32": rows from 32 on do not (the second trip)."""
    w = torch.ones(M, 1, dtype=dtype)
    if mutate == "odd_last_row" and M % 2:
        w[-1] = 0
    if mutate == "rows32":
        w[32:] = 0
    return w


def _sum_addends(first, more, skip, mutate):
    """first + the addends of `more` that are there; "missing_w1": the first missing one's stand-in (first again) counts."""
    g = first.clone()
    stood_in = False
    for i, e in enumerate(more):
        if e is not None:
            if i != skip:
                g = g + e
        elif mutate == "missing_w1" and not stood_in:
            g = g + first
            stood_in = True
    return g


def fwd(x, W, b=None, act=0, residual=None, x2=None, mutate=None):
    """-> y [M, N], xin = x + x2 [M, K] (with x2 only), and for the backward's feed: pre, a = act(pre)."""
    assert mutate is None or mutate in FWD_MUTATIONS, mutate
    xin = x if x2 is None else x + x2
    pre = (xin * _kmask(x.shape[1], mutate, x.dtype)) @ W.t()
    if b is not None:
        pre = pre + b
    a = act_fwd(pre, act)
    out = {"y": a if residual is None else a + residual, "pre": pre, "a": a}
    if x2 is not None:
        out["xin"] = x if mutate == "xin_x" else xin
    return out


def bwd(dy, saved, act, x, W, extras=(None, None, None), mutate=None):
    """dysum = dy + dy2 + dy3 + dy4, dpre = dysum act'(saved), dx = dpre W, dW = dpre^T x, db = sum_m dpre."""
    assert mutate is None or mutate in BWD_MUTATIONS, mutate
    M, N = dy.shape
    g = _sum_addends(dy, extras, 1 if mutate == "skip_dy3" else -1, mutate)
    if act == 3 and mutate == "gelu_from_out":
        saved = act_fwd(saved, 3)
    dpre = dact(g, saved, act, mutate)
    dp = dpre * _row_mask(M, mutate, dy.dtype)
    return {"dysum": dpre if mutate == "dysum_after" else g, "dx": (dpre * _kmask(N, mutate, dy.dtype)) @ W,
            "dW": dp.t() @ x, "db": dp.sum(0)}


def dw(dy, saved, act, x, mutate=None):
    """The weight-gradient half alone (mil_linear_small_dw_grouped)."""
    dp = dact(dy, saved, act) * _row_mask(dy.shape[0], mutate, dy.dtype)
    return {"dW": dp.t() @ x, "db": dp.sum(0)}


def bwd_split(dy, saved, act, W, nsplit, mutate=None):
    """parts [nsplit, M, K]: part s = dpre[:, s N / S : (s + 1) N / S] W[s N / S : .., :].  "split_range": every inner
    boundary 16 further."""
    assert mutate is None or mutate in SPLIT_MUTATIONS, mutate
    N = dy.shape[1]
    dpre = dact(dy, saved, act)
    cut = [s * (N // nsplit) + (16 if mutate == "split_range" and 0 < s < nsplit else 0) for s in range(nsplit + 1)]
    parts = torch.stack([dpre[:, cut[s]:cut[s + 1]] @ W[cut[s]:cut[s + 1]] for s in range(nsplit)])
    return {"parts": parts, "dx": parts.sum(0)}


def ln_fwd(u, gamma, beta, eps, W, b=None, act=0, residual=None, x2=None, mutate=None):
    """xn = LN(u) gamma + beta (two-pass variance, eps inside the root), xin = xn + x2, y = act(xin W^T + b) + residual.
    "onepass": var = E[u^2] - mean^2 with the two moments exact and each rounded to float32 once - what the formula costs in
    float32 under any summation order (in float64 the one-pass form is no error at all)."""
    assert mutate is None or mutate in LN_FWD_MUTATIONS, mutate
    n = u.shape[1]
    mean = u.mean(1, keepdim=True)
    if mutate == "onepass":
        m32, sq32 = mean.double().float(), (u.double() * u.double()).mean(1, keepdim=True).float()
        var = (sq32 - m32 * m32).clamp_min(0).to(u.dtype)
    else:
        d = u - mean
        var = (d * d).sum(1, keepdim=True) / (n - 1 if mutate == "var_e1" else n)
    rstd = 1 / (var.sqrt() + eps) if mutate == "eps_outside" else 1 / torch.sqrt(var + eps)
    xn = (u - mean) * rstd * gamma + beta
    out = fwd(xn, W, b, act, residual, x2, "xin_x" if mutate == "xin_x" else None)
    out.update(xn=xn, mean=mean[:, 0], rstd=rstd[:, 0])
    return out


def _lanes_sum(part):
    """[rows, 32] float32 -> [rows, 1]: the xor butterfly 16, 8, 4, 2, 1 over the 32 threads of a row."""
    s = part.copy()
    for m in (16, 8, 4, 2, 1):
        s = (s + s[:, np.arange(32) ^ m]).astype(np.float32)
    return s[:, :1]


def _thread_sum(v):
    """[rows, 512] float32 -> [rows, 32]: thread p adds columns 4 p + 128 j, j = 0 .. 3, each four as (a + b) + (c + d)."""
    s = np.zeros((v.shape[0], 32), np.float32)
    for j in range(4):
        b = v[:, 128 * j:128 * (j + 1)].reshape(-1, 32, 4)
        s = (s + ((b[..., 0] + b[..., 1]) + (b[..., 2] + b[..., 3]))).astype(np.float32)
    return s


def ln_norm_in_kernel_order(u, gamma, beta, eps, corrected=True):
    """xn, mean, rstd of mil_linear_small_ln_fwd in float32 numpy with the summation order of k_small_fwd_ln (32 threads per
    row).  corrected: the mean of the centred row is added back to the mean and taken off the row before the variance;
    False: the order the kernel had before (docs/lab_notes.md, token-side small-linear stages, finding 3)."""
    f = np.float32
    u, gamma, beta = (t.numpy().astype(f) for t in (u, gamma, beta))
    mean = _lanes_sum(_thread_sum(u)) / f(E)
    d = u - mean
    if corrected:
        corr = _lanes_sum(_thread_sum(d)) / f(E)
        mean, d = mean + corr, d - corr
    rstd = f(1) / np.sqrt(_lanes_sum(_thread_sum(d * d)) / f(E) + f(eps))
    xn = d * rstd * gamma + beta
    assert xn.dtype == f and mean.dtype == f and rstd.dtype == f
    return {"xn": torch.from_numpy(xn), "mean": torch.from_numpy(mean[:, 0]), "rstd": torch.from_numpy(rstd[:, 0])}


def ln_bwd(gs, u, mean, rstd, gamma, W=None, mutate=None):
    """gs: (g1, g2 .. g5 or None).  g = sum gs, xhat = (u - mean) rstd from the GIVEN statistics, gg = g gamma,
    du = rstd (gg - mean(gg) - xhat mean(gg xhat)), dx = du W, dgamma = sum_m g xhat, dbeta = sum_m g."""
    assert mutate is None or mutate in LN_BWD_MUTATIONS, mutate
    skip = {"skip_g3": 1, "skip_g5": 3}.get(mutate, -1)
    g = _sum_addends(gs[0], gs[1:], skip, mutate)
    xhat = (u - mean[:, None]) * rstd[:, None]
    gg = g if mutate == "no_gamma" else g * gamma
    s1, s2 = gg.mean(1, keepdim=True), (gg * xhat).mean(1, keepdim=True)
    du = rstd[:, None] * (gg - s1 - (0 if mutate == "no_xhat_term" else xhat * s2))
    gm = g * _row_mask(u.shape[0], mutate, u.dtype)
    out = {"du": du, "dgamma": (gm * xhat).sum(0), "dbeta": gm.sum(0)}
    if W is not None:
        out["dx"] = du @ W
    return out


def sum4(a, b, c=None, d=None):
    out = a + b
    if c is not None:
        out = out + (c if d is None else c + d)
    return {"out": out}


# --------------------------------------------------------------------------- torch autograd of the same operations
def _torch_act(v, act):
    return [lambda t: t, torch.tanh, torch.relu, lambda t: t * torch.sigmoid(QG * t), torch.sigmoid][act](v)


def autograd_linear(x, W, b, act, residual, x2, dy):
    t = {n: v.detach().clone().requires_grad_(True) for n, v in (("x", x), ("W", W), ("b", b), ("x2", x2)) if v is not None}
    xin = t["x"] + t["x2"] if x2 is not None else t["x"]
    y = _torch_act(torch.nn.functional.linear(xin, t["W"], t.get("b")), act)
    if residual is not None:
        y = y + residual
    y.backward(dy)
    return {"y": y.detach(), "dx": t["x"].grad, "dW": t["W"].grad, "db": t["b"].grad if b is not None else dy.new_zeros(0)}


def autograd_ln(u, gamma, beta, eps, Wp, g):
    """LayerNorm(u0 + xp Wp^T) with xp = 0 under the gradient g at its output -> du, dx = du Wp, dgamma, dbeta."""
    t = {n: v.detach().clone().requires_grad_(True) for n, v in (("u", u), ("gamma", gamma), ("beta", beta))}
    xp = torch.zeros(u.shape[0], Wp.shape[1], dtype=u.dtype, requires_grad=True)
    xn = torch.nn.functional.layer_norm(t["u"] + xp @ Wp.t(), (u.shape[1],), t["gamma"], t["beta"], eps)
    xn.backward(g)
    return {"xn": xn.detach(), "du": t["u"].grad, "dx": xp.grad, "dgamma": t["gamma"].grad, "dbeta": t["beta"].grad}


# --------------------------------------------------------------------------- block makers
def row_blocks(M, width):
    """[M, width]: every row, the last partial 16-row tile, the first and last 16-column tile, the whole."""
    out = {f"r{i}": (slice(i, i + 1),) for i in range(M)}
    if M % 16:
        out["rtail"] = (slice(16 * (M // 16), M),)
    out["c0"] = (slice(None), slice(0, 16))
    out["cL"] = (slice(None), slice(width - 16, width))
    out["all"] = (Ellipsis,)
    return out


def dw_blocks(N, K):
    """[N, K]: the whole, the first and last 16-column tile, the last (partial) 64 x 128 tile, the last row."""
    return {"all": (Ellipsis,), "c0": (slice(None), slice(0, 16)), "cL": (slice(None), slice(K - 16, K)),
            "tile": (slice(64 * ((N - 1) // 64), N), slice(128 * ((K - 1) // 128), K)), "rlast": (slice(N - 1, N),)}


def vec_blocks(n, group=128):
    out = {f"g{i}": (slice(group * i, min(n, group * (i + 1))),) for i in range(-(-n // group))}
    out["all"] = (Ellipsis,)
    return out


def elem_blocks(M):
    out = {f"r{i}": (slice(i, i + 1),) for i in range(M)}
    out["all"] = (Ellipsis,)
    return out


def part_blocks(nsplit, M, K):
    out = {}
    for s in range(nsplit):
        out.update({f"p{s}.{n}": (s,) + ix for n, ix in row_blocks(M, K).items() if n != "all"})
        out[f"p{s}.all"] = (s,)
    return out


def lin_blocks(M, N, K):
    return {"y": row_blocks(M, N), "xin": row_blocks(M, K), "xn": row_blocks(M, K), "mean": elem_blocks(M), "rstd": elem_blocks(M),
            "dysum": row_blocks(M, N), "dx": row_blocks(M, K), "dW": dw_blocks(N, K), "db": vec_blocks(N)}


def ln_bwd_blocks(M, K):
    return {"du": row_blocks(M, E), "dx": row_blocks(M, K), "dgamma": vec_blocks(E), "dbeta": vec_blocks(E)}


def expected_zero(act, N, tensor, name):
    """The planted exact zero: the last output column of a ReLU layer is dead in every row, so row N - 1 of dW is zero."""
    return act == 2 and tensor == "dW" and name == "rlast"


# --------------------------------------------------------------------------- the cases (shared by the host and GPU tests)
ROWS = (1, 7, 16, 17, 31, 33, 63, 64)
FWD_SHAPES = ((16, 16), (48, 32), (512, 512), (256, 528), (512, 1024), (2048, 512))          # (N, K)
BWD_SHAPES = ((16, 16), (48, 48), (512, 256), (1024, 512), (512, 2048))
ACT_SHAPE_FWD, ACT_SHAPE_BWD = (512, 512), (512, 256)
SPLITS = ((1024, 2), (2048, 2), (2048, 4))
LN_N = (16, 256, 2048)
LN_K = (16, 48, 256, 512)
EXTRA_PATTERNS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1))          # dy2, dy3, dy4 present
G_PATTERNS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 0), (1, 1, 0, 1),
              (1, 1, 1, 1))                                                                  # g2 .. g5 present
DW_BLOCK = [(512, 512), (512, 512), (256, 512), (512, 256), (2048, 512), (512, 2048), (256, 512), (512, 256)]
DW_ALL = DW_BLOCK * 2 + [(256, 512), (512, 256), (512, 512)]                                # the 19 layers of test_gpu_dw_grouped.py
DW_ACTS = [0, 2, 1, 0, 2, 0, 4, 3] * 2 + [0, 0, 1]
DW_ROWS = (1, 7, 33, 64)
SUM4_N = (4, 1020, 1024, 262144)


def pairs(shapes):
    """(M, shape): every shape with M in {7, 33, 64}, every M with two shapes."""
    out = [(m, s) for s in shapes for m in (7, 33, 64)]
    for i, m in enumerate(ROWS):
        for s in (shapes[i % len(shapes)], shapes[(i + 3) % len(shapes)]):
            if (m, s) not in out:
                out.append((m, s))
    return out


def _runs(shapes, act_shape):
    out = []
    for m, (n, k) in pairs(shapes):
        for act in (range(5) if (n, k) == act_shape and m in (7, 33, 64) else (0,)):
            out.append(dict(M=m, N=n, K=k, act=act))
    return out


def fwd_runs(x2):
    """bias on two of three runs and on every ReLU one (the dead column needs it), residual on every other, act as _runs."""
    return [dict(r, bias=i % 3 != 2 or r["act"] == 2, res=i % 2 == 0, x2=x2) for i, r in enumerate(_runs(FWD_SHAPES, ACT_SHAPE_FWD))]


def bwd_runs(summed):
    """summed: the extras cycle through EXTRA_PATTERNS and dysum is asked for on every other run that forms dx.
    outs cycles through everything / dx only / dW and db only / db without dW."""
    out = []
    for i, r in enumerate(_runs(BWD_SHAPES, ACT_SHAPE_BWD)):
        outs = ("dx", "dW", "db") if i % 5 < 2 else (("dx",), ("dW", "db"), ("db",))[i % 5 - 2]
        ex = EXTRA_PATTERNS[i % len(EXTRA_PATTERNS)] if summed else (0, 0, 0)
        out.append(dict(r, extras=ex, dysum=summed and "dx" in outs and (i % 2 == 1 or not any(ex)), outs=outs))
    return out


def split_runs():
    return [dict(M=m, N=n, K=k, act=(0, 2, 3)[(i + j) % 3], nsplit=s) for i, (n, s) in enumerate(SPLITS) for j, (k, m) in
            enumerate(((512, 7), (512, 33), (48, 7), (48, 33)))]


def ln_fwd_runs():
    out = [(m, n) for n in LN_N for m in (7, 33, 64)] + [(m, LN_N[i % 3]) for i, m in enumerate(ROWS)]
    return [dict(M=m, N=n, K=E, act=i % 5, bias=i % 3 != 2 or i % 5 == 2, res=i % 2 == 0, x2=i % 4 < 2, ln=True)
            for i, (m, n) in enumerate(dict.fromkeys(out))]


def ln_bwd_runs():
    """Every addend pattern at three (M, K); outs cycles through all / no dgamma / no dx / no du."""
    out = []
    for i, pat in enumerate(G_PATTERNS):
        for j in range(3):
            c = 3 * i + j
            outs = (("dx", "du", "dgamma", "dbeta"), ("dx", "du"), ("du", "dgamma", "dbeta"), ("dx", "dgamma", "dbeta"))[c % 4]
            out.append(dict(M=ROWS[(c * 3 + 1) % len(ROWS)], K=LN_K[c % 4], pat=pat, outs=outs))
    return out


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def lin_case(M, N, K, act, ln=False):
    """float32-exact inputs in float64, every optional one included (a run uses those it names).  x has mean 0.25; with ln it
    is the norm's input u: rows of mean 30 and std 1, (M >= 2) one row of constant 0.5 and (M >= 3) row 2 of mean 30 and std 0.1.  ReLU: W[N - 1] = 0, b[N - 1] = -1,
    so that output column is dead in every row."""
    g = _gen(M, N, K, act, ln)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    c = dict(x=r(M, K) + (30.0 if ln else 0.25), x2=0.5 * r(M, K), W=r(N, K) / math.sqrt(K), b=0.5 * r(N), residual=r(M, N),
             dy=r(M, N), dy2=r(M, N), dy3=0.5 * r(M, N), dy4=2.0 * r(M, N), gamma=1.0 + 0.2 * r(K), beta=0.3 * r(K))
    if ln and M >= 2:
        c["x"][min(5, M - 1)] = 0.5
    if ln and M >= 3:
        c["x"][2] = 30.0 + LOW_STD * (c["x"][2] - 30.0)
    if act == 2:
        c["W"][N - 1] = 0
        c["b"][N - 1] = -1.0
    return {n: f32exact(t) for n, t in c.items()}


@functools.lru_cache(maxsize=None)
def ln_bwd_case(M, K):
    """g1 .. g5, u (as lin_case's), gamma, W_P [512, K]: float32-exact in float64; mean, rstd: the float32 rounding of the
    float64 statistics of u."""
    g = _gen(M, K, 77)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    c = dict(g1=r(M, E), g2=r(M, E), g3=0.5 * r(M, E), g4=2.0 * r(M, E), g5=r(M, E), u=r(M, E) + 30.0, gamma=1.0 + 0.2 * r(E),
             W=r(E, K) / math.sqrt(E))
    if M >= 2:
        c["u"][min(5, M - 1)] = 0.5
    if M >= 3:
        c["u"][2] = 30.0 + LOW_STD * (c["u"][2] - 30.0)
    c = {n: f32exact(t) for n, t in c.items()}
    d = c["u"] - c["u"].mean(1, keepdim=True)
    c["mean"] = f32exact(c["u"].mean(1))
    c["rstd"] = f32exact(1 / torch.sqrt((d * d).mean(1) + EPS))
    return c


def run_fwd(run, dtype=torch.float64, mutate=None):
    c = lin_case(run["M"], run["N"], run["K"], run["act"], run.get("ln", False))
    t = lambda n, on=True: c[n].to(dtype) if on else None                                    # noqa: E731
    args = (t("W"), t("b", run["bias"]), run["act"], t("residual", run["res"]), t("x2", run["x2"]))
    if run.get("ln"):
        return ln_fwd(t("x"), t("gamma"), t("beta"), EPS, *args, mutate=mutate)
    return fwd(t("x"), *args, mutate=mutate)


def saved_of(run):
    """What the backward of `run` is fed: the float32 rounding of the float64 forward's output (pre-activation for
    QuickGELU) of the layer with bias and without residual, x2."""
    c = lin_case(run["M"], run["N"], run["K"], run["act"])
    f = fwd(c["x"], c["W"], c["b"], run["act"])
    return f32exact(f["pre"] if run["act"] == 3 else f["a"])


def run_bwd(run, dtype=torch.float64, mutate=None):
    c = lin_case(run["M"], run["N"], run["K"], run["act"])
    ex = tuple(c[n].to(dtype) if on else None for n, on in zip(("dy2", "dy3", "dy4"), run["extras"]))
    r = bwd(c["dy"].to(dtype), saved_of(run).to(dtype), run["act"], c["x"].to(dtype), c["W"].to(dtype), ex, mutate)
    return {n: v for n, v in r.items() if n in run["outs"] or (n == "dysum" and run["dysum"])}


def run_dw(run, dtype=torch.float64, mutate=None):
    """One layer of mil_linear_small_dw_grouped: run["outs"] of dW, db."""
    c = lin_case(run["M"], run["N"], run["K"], run["act"])
    r = dw(c["dy"].to(dtype), saved_of(run).to(dtype), run["act"], c["x"].to(dtype), mutate)
    return {n: v for n, v in r.items() if n in run["outs"]}


def run_split(run, dtype=torch.float64, mutate=None):
    c = lin_case(run["M"], run["N"], run["K"], run["act"])
    return bwd_split(c["dy"].to(dtype), saved_of(run).to(dtype), run["act"], c["W"].to(dtype), run["nsplit"], mutate)


def run_ln_bwd(run, dtype=torch.float64, mutate=None):
    c = ln_bwd_case(run["M"], run["K"])
    gs = [c["g1"].to(dtype)] + [c[n].to(dtype) if on else None for n, on in zip(("g2", "g3", "g4", "g5"), run["pat"])]
    r = ln_bwd(gs, c["u"].to(dtype), c["mean"].to(dtype), c["rstd"].to(dtype), c["gamma"].to(dtype), c["W"].to(dtype), mutate)
    return {n: v for n, v in r.items() if n in run["outs"]}


def tag(run):
    return " ".join(f"{k} {ACT_NAMES[v] if k == 'act' else v}" for k, v in run.items())


# k of bound(e32, k) per stage: the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) that the first
# full run on an MI355X showed at the cap (the table "token-side small-linear stages" in docs/lab_notes.md), capped at K_CAP
K_STAGE = {"fwd": 4, "fwd_add": 4, "bwd": 4, "bwd_sum": 8, "bwd_split": 4, "ln_fwd": 4, "ln_bwd": 4, "ln_bwd3": 4, "ln_bwd5": 8,
           "dw_grouped": 4, "sum4": 2}


def hold(stage, case, got, ref, r32, blocks):
    """Every block of every tensor of `got` within bound(e32, K_STAGE[stage]) of `ref`; prints the worst block per tensor
    first.  A block whose reference is all zero is met exactly or not at all (block_err)."""
    bad, worst = [], 0.0
    for t in got:
        e32, eg = block_err(r32[t], ref[t], blocks[t]), block_err(got[t], ref[t], blocks[t])
        w = max(eg, key=lambda b: eg[b] / max(e32[b], FLOOR))
        ratio = eg[w] / max(e32[w], FLOOR)
        worst = max(worst, ratio)
        print(f"RATIO | {stage} | {case} | {t}.{w} | gpu {eg[w]:.2e} | e32 {e32[w]:.2e} | {ratio:.2f}")
        bad += [(t, b, e, e32[b]) for b, e in eg.items() if not e <= bound(e32[b], K_STAGE[stage])]
    assert not bad, (stage, case, bad[:8])
    return worst
