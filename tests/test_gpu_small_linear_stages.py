"""GPU: every C entry of the token-side few-rows family (csrc/small_linear.hip) on its own against the float64 restatement
of tests/small_linear_ref.py, per block: max|got - ref| / max|ref| over a block <= k x max(e32, 1e-7), e32 being what the
float32 restatement loses on the CPU over the same block.  tests/test_small_linear_sensitivity_host.py shows what these
bounds see; the k of each stage (small_linear_ref.K_STAGE) comes from the measured ratios in docs/lab_notes.md.  Every
backward is fed the float32 rounding of the float64 forward, as is the float32 restatement: one entry under test at a time.
Every run is made dense and strided.  Strided: operands and outputs are 16-byte-aligned column slices of buffers 4 or 16
floats wider; the gap columns and three rows behind every input hold NaN - a result that depends on memory outside the
described operands fails - and the gap columns, three guard rows behind every output and 64 floats behind every contiguous
side output hold a sentinel that is compared bit for bit afterwards (dense: the guard rows and tails)."""
import ctypes
import math

import pytest
import torch

import small_linear_ref as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -12345.678                    # the sentinel; the bit pattern is what is compared
SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
EINVAL = -22
GUARD, TAIL = 3, 64
E = S.E
LAYOUTS = pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class In:
    """An operand on the device.  strided: columns [off, off + width) of a NaN buffer `pad` floats wider and GUARD rows longer."""

    def __init__(self, t, strided=False, pad=4, off=0):
        t = t.float()
        if strided and t.dim() == 2:
            buf = torch.full((t.shape[0] + GUARD, t.shape[1] + pad), math.nan, dtype=torch.float32)
            buf[:t.shape[0], off:off + t.shape[1]] = t
            self.ld = t.shape[1] + pad
        else:
            buf, off = t.contiguous(), 0
            self.ld = t.shape[-1]
        self.buf = buf.to(DEV)
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * off)


class Out:
    """An output full of the sentinel.  flat: [rows, width] contiguous + TAIL floats; else GUARD rows behind it and, strided,
    columns [off, off + width) of a buffer `pad` floats wider."""

    def __init__(self, rows, width, strided=False, pad=16, off=4, flat=False, lead=None):
        self.shape = (rows, width) if lead is None else (lead, rows, width)
        n = rows * width * (lead or 1)
        if flat:
            self.buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=DEV)
            self.view, self.ld, off = self.buf[:n].view(self.shape), width, 0
        else:
            pad, off = (pad, off) if strided else (0, 0)
            self.buf = torch.full((rows + GUARD, width + pad), SENT, dtype=torch.float32, device=DEV)
            self.view, self.ld = self.buf[:rows, off:off + width], width + pad
        self.off = off
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * off)

    def untouched_outside(self):
        bits = self.buf.clone()
        if bits.dim() == 1:
            bits[:self.view.numel()] = SENT
        else:
            bits[:self.shape[0], self.off:self.off + self.shape[1]] = SENT
        return bool((bits.view(torch.int32) == SENT_BITS).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENT_BITS).all())

    def get(self):
        return self.view.detach().cpu()


def _p(o):
    return None if o is None else o.p


def _ld(o):
    return 0 if o is None else o.ld


def _vec(n):
    return Out(1, n, flat=True)


def _check_outs(case, outs):
    torch.cuda.synchronize()
    for name, o in outs.items():
        assert o.untouched_outside(), f"{case}: wrote outside {name}"


def _hold(stage, case, got, ref, r32, blocks):
    S.hold(stage, case, got, ref, r32, blocks)


def _case_name(run, strided):
    return S.tag(run) + (" strided" if strided else " dense")


# --------------------------------------------------------------------------- forward
def _forward(stage, run, strided):
    L = _lib()
    M, N, K, act = run["M"], run["N"], run["K"], run["act"]
    ln = run.get("ln", False)
    c = S.lin_case(M, N, K, act, ln)
    x, W = In(c["x"], strided, 4, 0), In(c["W"], strided, 16, 4)
    b = In(c["b"]) if run["bias"] else None
    res = In(c["residual"], strided, 16, 4) if run["res"] else None
    x2 = In(c["x2"], strided, 4, 0) if run["x2"] else None
    outs = {"y": Out(M, N, strided, 4, 0)}
    if x2 is not None:
        outs["xin"] = Out(M, K, flat=True)
    if ln:
        gamma, beta = In(c["gamma"]), In(c["beta"])
        outs["xn"], outs["stats"] = Out(M, K, flat=True), Out(M, 2, flat=True)
        rc = L.mil_linear_small_ln_fwd(x.p, x.ld, gamma.p, beta.p, S.EPS, _p(x2), _ld(x2), W.p, W.ld, _p(b), act, _p(res), _ld(res),
                                       outs["y"].p, outs["y"].ld, outs["xn"].p, _p(outs.get("xin")), outs["stats"].p, M, N, _st())
    elif stage == "fwd":
        rc = L.mil_linear_small_fwd(x.p, x.ld, W.p, W.ld, _p(b), act, _p(res), _ld(res), outs["y"].p, outs["y"].ld, M, N, K, _st())
    else:
        rc = L.mil_linear_small_fwd_add(x.p, x.ld, _p(x2), _ld(x2), _p(outs.get("xin")), W.p, W.ld, _p(b), act, _p(res), _ld(res),
                                        outs["y"].p, outs["y"].ld, M, N, K, _st())
    case = _case_name(run, strided)
    assert rc == 0, case
    _check_outs(case, outs)
    got = {n: o.get() for n, o in outs.items() if n != "stats"}
    if ln:
        st = outs["stats"].get()
        got["mean"], got["rstd"] = st[:, 0], st[:, 1]
    _hold(stage, case, got, S.run_fwd(run), S.run_fwd(run, torch.float32), S.lin_blocks(M, N, K))


@LAYOUTS
def test_fwd(strided):
    """mil_linear_small_fwd: M 1 .. 64 over (N, K) = (16, 16) .. (2048, 512), K = 528 (a 16-wide second chunk) and 1024 (the
    16-wave kernel), all five activations at (512, 512), with and without bias / residual."""
    for run in S.fwd_runs(False):
        _forward("fwd", run, strided)


@LAYOUTS
def test_fwd_add(strided):
    """mil_linear_small_fwd_add: the same runs with x2, xin = x + x2 written by column tile 0."""
    for run in S.fwd_runs(True):
        _forward("fwd_add", run, strided)


@LAYOUTS
def test_ln_fwd(strided):
    """mil_linear_small_ln_fwd: u rows of mean 30 and std 1 and one row of constant 0.5; N 16, 256, 2048; with and without x2,
    residual, bias; a row of mean 30 and std 0.1; xn, xin, the statistics (mean and rstd as tensors of their own) and y."""
    for run in S.ln_fwd_runs():
        _forward("ln_fwd", run, strided)


# --------------------------------------------------------------------------- backward
def _backward(stage, run, strided):
    L = _lib()
    M, N, K, act = run["M"], run["N"], run["K"], run["act"]
    c = S.lin_case(M, N, K, act)
    summed = any(run["extras"]) or run["dysum"]
    dy = In(c["dy"], strided and not summed, 16, 4)            # the extras' stride is N: lddy must be N beside them
    ex = [In(c[n]) if on else None for n, on in zip(("dy2", "dy3", "dy4"), run["extras"])]
    saved = In(S.saved_of(run), strided, 4, 0) if act else None
    x = In(c["x"], strided, 16, 4) if ("dW" in run["outs"] or "db" in run["outs"]) else None
    W = In(c["W"], strided, 4, 0) if "dx" in run["outs"] else None
    outs = {}
    if "dx" in run["outs"]:
        outs["dx"] = Out(M, K, strided, 4, 0)
    if "dW" in run["outs"]:
        outs["dW"] = Out(N, K, strided, 16, 4)
    if "db" in run["outs"]:
        outs["db"] = _vec(N)
    if run["dysum"]:
        outs["dysum"] = Out(M, N, flat=True)
    o = lambda n: _p(outs.get(n))                                                            # noqa: E731
    if stage == "bwd":
        rc = L.mil_linear_small_bwd(dy.p, dy.ld, _p(saved), _ld(saved), act, _p(x), _ld(x), _p(W), _ld(W), o("dx"), _ld(outs.get("dx")),
                                    o("dW"), _ld(outs.get("dW")), o("db"), M, N, K, _st())
    else:
        rc = L.mil_linear_small_bwd_sum(dy.p, dy.ld, _p(ex[0]), _p(ex[1]), _p(ex[2]), o("dysum"), _p(saved), _ld(saved), act, _p(x),
                                        _ld(x), _p(W), _ld(W), o("dx"), _ld(outs.get("dx")), o("dW"), _ld(outs.get("dW")), o("db"),
                                        M, N, K, _st())
    case = _case_name(run, strided)
    assert rc == 0, case
    _check_outs(case, outs)
    got = {n: (v.get()[0] if n == "db" else v.get()) for n, v in outs.items()}
    _hold(stage, case, got, S.run_bwd(run), S.run_bwd(run, torch.float32), S.lin_blocks(M, N, K))


@LAYOUTS
def test_bwd(strided):
    """mil_linear_small_bwd: M 1 .. 64 over (N, K) = (16, 16), (48, 48) (a clamped dW tile in n and k), (512, 256) with all five
    activations, (1024, 512) (the 16-wave kernel), (512, 2048); everything / dx only / dW and db only / db without dW.  Row
    N - 1 of dW behind the dead ReLU column is an exact zero."""
    for run in S.bwd_runs(False):
        _backward("bwd", run, strided)


@LAYOUTS
def test_bwd_sum(strided):
    """mil_linear_small_bwd_sum: the same runs with 0 .. 3 extras (also dy3 alone, dy4 alone: stand-ins in front of a present
    addend), dysum on and off."""
    for run in S.bwd_runs(True):
        _backward("bwd_sum", run, strided)


@LAYOUTS
def test_bwd_split(strided):
    """mil_linear_small_bwd_split: (N, nsplit) = (1024, 2), (2048, 2) (the 16-wave kernel), (2048, 4) at K 512 and 48, M 7 and
    33; the parts and their sum."""
    L = _lib()
    for run in S.split_runs():
        M, N, K, act, ns = run["M"], run["N"], run["K"], run["act"], run["nsplit"]
        c = S.lin_case(M, N, K, act)
        dy, W = In(c["dy"], strided, 16, 4), In(c["W"], strided, 4, 0)
        saved = In(S.saved_of(run), strided, 4, 0) if act else None
        parts = Out(M, K, flat=True, lead=ns)
        rc = L.mil_linear_small_bwd_split(dy.p, dy.ld, _p(saved), _ld(saved), act, W.p, W.ld, parts.p, M, N, K, ns, _st())
        case = _case_name(run, strided)
        assert rc == 0, case
        _check_outs(case, {"dx_parts": parts})
        got = {"parts": parts.get(), "dx": parts.get().double().sum(0)}
        blocks = {"parts": S.part_blocks(ns, M, K), "dx": S.row_blocks(M, K)}
        _hold("bwd_split", case, got, S.run_split(run), S.run_split(run, torch.float32), blocks)


# --------------------------------------------------------------------------- LayerNorm backward
def _ln_backward(stage, run, strided):
    L = _lib()
    M, K, pat = run["M"], run["K"], run["pat"]
    c = S.ln_bwd_case(M, K)
    g1, u = In(c["g1"], strided, 16, 4), In(c["u"], strided, 4, 0)
    g2 = In(c["g2"], strided, 4, 0) if pat[0] else None
    g3 = In(c["g3"], strided, 16, 4) if pat[1] else None
    g4 = In(c["g4"]) if pat[2] else None
    g5 = In(c["g5"]) if pat[3] else None
    stats, gamma = In(torch.stack([c["mean"], c["rstd"]], 1)), In(c["gamma"])
    W = In(c["W"], strided, 16, 4) if "dx" in run["outs"] else None
    outs = {}
    if "dx" in run["outs"]:
        outs["dx"] = Out(M, K, strided, 4, 0)
    if "du" in run["outs"]:
        outs["du"] = Out(M, E, flat=True)
    if "dgamma" in run["outs"]:
        outs["dgamma"], outs["dbeta"] = _vec(E), _vec(E)
    o = lambda n: _p(outs.get(n))                                                            # noqa: E731
    tail = (u.p, u.ld, stats.p, gamma.p, _p(W), _ld(W), o("dx"), _ld(outs.get("dx")), o("du"), o("dgamma"), o("dbeta"), M, K, _st())
    if stage == "ln_bwd":
        rc = L.mil_linear_small_ln_bwd(g1.p, g1.ld, _p(g2), _ld(g2), *tail)
    elif stage == "ln_bwd3":
        rc = L.mil_linear_small_ln_bwd3(g1.p, g1.ld, _p(g2), _ld(g2), _p(g3), _ld(g3), *tail)
    else:
        rc = L.mil_linear_small_ln_bwd5(g1.p, g1.ld, _p(g2), _ld(g2), _p(g3), _ld(g3), _p(g4), _p(g5), *tail)
    case = _case_name(run, strided)
    assert rc == 0, case
    _check_outs(case, outs)
    got = {n: (v.get()[0] if n in ("dgamma", "dbeta") else v.get()) for n, v in outs.items()}
    _hold(stage, case, got, S.run_ln_bwd(run), S.run_ln_bwd(run, torch.float32), S.ln_bwd_blocks(M, K))


@LAYOUTS
def test_ln_bwd(strided):
    """mil_linear_small_ln_bwd: one and two addends; K of W_P 16 .. 512; with and without dx, du, dgamma / dbeta."""
    for run in S.ln_bwd_runs():
        if not any(run["pat"][1:]):
            _ln_backward("ln_bwd", run, strided)


@LAYOUTS
def test_ln_bwd3(strided):
    """mil_linear_small_ln_bwd3: g2 and g3 in every combination."""
    for run in S.ln_bwd_runs():
        if not any(run["pat"][2:]):
            _ln_backward("ln_bwd3", run, strided)


@LAYOUTS
def test_ln_bwd5(strided):
    """mil_linear_small_ln_bwd5: one to five addends, among them exactly one of g4 / g5 beside a g1 whose row stride is 528
    (strided): the missing one's stand-in must stay inside a described operand - the gaps of g1's buffer are NaN."""
    for run in S.ln_bwd_runs():
        _ln_backward("ln_bwd5", run, strided)


# --------------------------------------------------------------------------- grouped weight gradient, four-way sum
def _dw_layers(M, layers, strided):
    """[(run, outs dict)] and the descriptor array of `layers` = [(N, K, act, outs)]."""
    from mil_amd import _lib as ML
    arr = (ML.SmallDwDesc * len(layers))()
    keep, res = [], []
    for d, (N, K, act, which) in zip(arr, layers):
        run = dict(M=M, N=N, K=K, act=act, outs=which)
        c = S.lin_case(M, N, K, act)
        dy, x = In(c["dy"], strided, 16, 4), In(c["x"], strided, 4, 0)
        saved = In(S.saved_of(run), strided, 16, 4) if act else None
        outs = {}
        if "dW" in which:
            outs["dW"] = Out(N, K, strided, 16, 4)
        if "db" in which:
            outs["db"] = _vec(N)
        keep.append((dy, x, saved))
        d.dy, d.yv, d.x = dy.p.value, (saved.p.value if act else None), x.p.value
        d.dW, d.db = (outs["dW"].p.value if "dW" in outs else None), (outs["db"].p.value if "db" in outs else None)
        d.lddy, d.ldyv, d.ldx, d.lddw, d.act, d.M, d.N, d.K = dy.ld, _ld(saved), x.ld, _ld(outs.get("dW")), act, M, N, K
        res.append((run, outs))
    return arr, res, keep


@LAYOUTS
@pytest.mark.parametrize("M", S.DW_ROWS)
def test_dw_grouped(M, strided):
    """mil_linear_small_dw_grouped: the fusion step's 19 layers in one launch against the float64 restatement on the CPU, then
    one descriptor alone and 32 descriptors (small layers with dW only and db only among them)."""
    L = _lib()
    full = [(n, k, a, ("dW", "db")) for (n, k), a in zip(S.DW_ALL, S.DW_ACTS)]
    small = [((16, 16), (48, 48))[i % 2] + (i % 5, (("dW", "db"), ("dW",), ("db",))[i % 3]) for i in range(13)]
    for name, layers in (("19", full), ("1", full[4:5]), ("32", full + small)):
        arr, res, keep = _dw_layers(M, layers, strided)
        rc = L.mil_linear_small_dw_grouped(arr, len(layers), _st())
        assert rc == 0, name
        torch.cuda.synchronize()
        for i, (run, outs) in enumerate(res):
            case = f"n {name} layer {i} " + _case_name(run, strided)
            _check_outs(case, outs)
            got = {n: (v.get()[0] if n == "db" else v.get()) for n, v in outs.items()}
            _hold("dw_grouped", case, got, S.run_dw(run), S.run_dw(run, torch.float32), S.lin_blocks(M, run["N"], run["K"]))


def test_sum4():
    """mil_sum4: n 4, 1020 (a partial workgroup), 1024, 262144; c and d present and absent."""
    L = _lib()
    for n in S.SUM4_N:
        g = torch.Generator().manual_seed(n)
        a, b, c, d = (S.f32exact(torch.randn(n, generator=g, dtype=torch.float64) + i) for i in range(4))
        for nc in (0, 1, 2):
            ins = [In(t) for t in (a, b, c, d)[:2 + nc]] + [None] * (2 - nc)
            out = _vec(n)
            assert L.mil_sum4(ins[0].p, ins[1].p, _p(ins[2]), _p(ins[3]), out.p, n, _st()) == 0
            _check_outs(f"sum4 n {n}", {"out": out})
            args = [t.float() if j < 2 + nc else None for j, t in enumerate((a, b, c, d))]
            ref = S.sum4(*[None if t is None else t.double() for t in args])
            blocks = {"out": {"all": (Ellipsis,), "first4": (slice(0, 4),), "last4": (slice(n - 4, n),), "last1k": (slice(max(0, n - 1024), n),)}}
            _hold("sum4", f"n {n} addends {2 + nc}", {"out": out.get()[0]}, ref, S.sum4(*args), blocks)


# --------------------------------------------------------------------------- rejections
def test_rejections_launch_nothing():
    """Every refused call returns MIL_EINVAL and leaves its sentinel-filled outputs as they were."""
    from mil_amd import _lib as ML
    L = _lib()
    M, N, K = 7, 48, 32
    c = S.lin_case(M, N, K, 1)
    x, x2, W, b, dy, dy2 = (In(c[n]) for n in ("x", "x2", "W", "b", "dy", "dy2"))
    sv = In(S.saved_of(dict(M=M, N=N, K=K, act=1)))
    dyw = In(c["dy"], True, 4, 0)                                   # lddy = N + 4
    y, xin, dx, dW, db, dysum = Out(64, N), Out(64, K), Out(64, K), Out(N, K), _vec(N), Out(64, N)
    st = _st()
    off1 = lambda o: ctypes.c_void_p(o.p.value + 4)                                         # noqa: E731
    fwd = lambda x_=x.p, M_=M, K_=K, act=1, x2_=None, xin_=None: L.mil_linear_small_fwd_add(  # noqa: E731
        x_, K, x2_, K, xin_, W.p, K, b.p, act, None, 0, y.p, N, M_, N, K_, st)
    bwd = lambda dy_=dy, M_=M, N_=N, act=1, sv_=sv.p, dy2_=None, dysum_=None, dx_=dx.p: L.mil_linear_small_bwd_sum(  # noqa: E731
        dy_.p if isinstance(dy_, In) else dy_, dy_.ld if isinstance(dy_, In) else N, dy2_, None, None, dysum_, sv_, N, act, x.p, K, W.p, K,
        dx_, K, dW.p, K, db.p, M_, N_, K, st)
    calls = {
        "fwd M 0": lambda: fwd(M_=0), "fwd M 65": lambda: fwd(M_=65), "fwd K 24": lambda: fwd(K_=24), "fwd act 5": lambda: fwd(act=5),
        "fwd x off by one float": lambda: fwd(x_=off1(x)), "fwd x2 without xin": lambda: fwd(x2_=x2.p),
        "bwd M 0": lambda: bwd(M_=0), "bwd M 65": lambda: bwd(M_=65), "bwd N 40": lambda: bwd(N_=40), "bwd act 5": lambda: bwd(act=5),
        "bwd act without saved": lambda: bwd(sv_=None), "bwd dy off by one float": lambda: bwd(dy_=off1(dy)),
        "bwd dysum without dx": lambda: bwd(dysum_=dysum.p, dx_=None), "bwd extras with lddy != N": lambda: bwd(dy_=dyw, dy2_=dy2.p),
    }
    # the n-split: N = 2048 is the valid shape
    Ns = 2048
    cs = S.lin_case(M, Ns, K, 0)
    dys, Ws, parts = In(cs["dy"]), In(cs["W"]), Out(M, K, flat=True, lead=4)
    split = lambda N_=Ns, ns=4, M_=M, act=0, dy_=dys.p: L.mil_linear_small_bwd_split(dy_, N_, None, 0, act, Ws.p, K, parts.p, M_, N_, K, ns, st)  # noqa: E731
    calls.update({"split nsplit 3": lambda: split(ns=3), "split N 1536 nsplit 4": lambda: split(N_=1536), "split M 65": lambda: split(M_=65),
                  "split act without saved": lambda: split(act=2), "split dy off by one float": lambda: split(dy_=off1(dys))})
    # the LayerNorm pair
    cl, cb = S.lin_case(M, 16, E, 0, True), S.ln_bwd_case(M, 16)
    u, gamma, beta, Wl, x2l = (In(cl[n]) for n in ("x", "gamma", "beta", "W", "x2"))
    yl, xn, xinl, stats = Out(64, 16), Out(64, E, flat=True), Out(64, E, flat=True), Out(64, 2, flat=True)
    lnf = lambda M_=M, act=0, u_=u.p, x2_=None, xin_=None: L.mil_linear_small_ln_fwd(        # noqa: E731
        u_, E, gamma.p, beta.p, S.EPS, x2_, E, Wl.p, E, None, act, None, 0, yl.p, 16, xn.p, xin_, stats.p, M_, 16, st)
    g1, g4, g5, ub, gb, Wb = (In(cb[n]) for n in ("g1", "g4", "g5", "u", "gamma", "W"))
    sb = In(torch.stack([cb["mean"], cb["rstd"]], 1))
    dxl, du, dg, dbt = Out(64, 16), Out(64, E, flat=True), _vec(E), _vec(E)
    lnb = lambda M_=M, g1_=g1.p, ld=E, g4_=None, g5_=None, dg_=dg.p, dbt_=dbt.p: L.mil_linear_small_ln_bwd5(  # noqa: E731
        g1_, ld, None, 0, None, 0, g4_, g5_, ub.p, E, sb.p, gb.p, Wb.p, 16, dxl.p, 16, du.p, dg_, dbt_, M_, 16, st)
    calls.update({"ln_fwd M 0": lambda: lnf(M_=0), "ln_fwd M 65": lambda: lnf(M_=65), "ln_fwd act 5": lambda: lnf(act=5),
                  "ln_fwd u off by one float": lambda: lnf(u_=off1(u)), "ln_fwd x2 without xin": lambda: lnf(x2_=x2l.p),
                  "ln_bwd M 0": lambda: lnb(M_=0), "ln_bwd M 65": lambda: lnb(M_=65), "ln_bwd g1 off by one float": lambda: lnb(g1_=off1(g1)),
                  "ln_bwd dgamma without dbeta": lambda: lnb(dbt_=None), "ln_bwd ldg1 508": lambda: lnb(ld=508),
                  "ln_bwd ldg1 508 with g4": lambda: lnb(ld=508, g4_=g4.p), "ln_bwd ldg1 508 with g4, g5": lambda: lnb(ld=508, g4_=g4.p, g5_=g5.p)})
    # the four-way sum and the grouped weight gradient
    s4 = Out(1, 1024, flat=True)
    a4 = In(torch.ones(1028))
    calls.update({"sum4 n 1022": lambda: L.mil_sum4(a4.p, a4.p, None, None, s4.p, 1022, st),
                  "sum4 d without c": lambda: L.mil_sum4(a4.p, a4.p, None, a4.p, s4.p, 1024, st),
                  "sum4 a off by one float": lambda: L.mil_sum4(off1(a4), a4.p, None, None, s4.p, 1024, st)})
    arr = (ML.SmallDwDesc * 33)()
    for d in arr:
        d.dy, d.yv, d.x, d.dW, d.db = dy.p.value, sv.p.value, x.p.value, dW.p.value, db.p.value
        d.lddy, d.ldyv, d.ldx, d.lddw, d.act, d.M, d.N, d.K = N, N, K, K, 1, M, N, K

    def grouped(n=1, **kw):
        saved = {k: getattr(arr[0], k) for k in kw}
        for k, v in kw.items():
            setattr(arr[0], k, v)
        rc = L.mil_linear_small_dw_grouped(arr, n, st)
        for k, v in saved.items():
            setattr(arr[0], k, v)
        return rc
    calls.update({"grouped n 33": lambda: grouped(33), "grouped neither dW nor db": lambda: grouped(dW=None, db=None),
                  "grouped M 0": lambda: grouped(M=0), "grouped M 65": lambda: grouped(M=65), "grouped act 5": lambda: grouped(act=5),
                  "grouped act without saved": lambda: grouped(yv=None)})
    for name, call in calls.items():
        assert call() == EINVAL, name
    torch.cuda.synchronize()
    for name, o in dict(y=y, xin=xin, dx=dx, dW=dW, db=db, dysum=dysum, parts=parts, yl=yl, xn=xn, xinl=xinl, stats=stats, dxl=dxl,
                        du=du, dgamma=dg, dbeta=dbt, sum4=s4).items():
        assert o.untouched(), f"a refused call wrote {name}"
