"""GPU: every entry of the tiled fp32 linear family (csrc/linear.hip, gemm64.h, linear_nt2.hip, mid_linear.hip) on its own
against the float64 restatement of tests/linear_ref.py, route by route and block by block.  Each run first asks the library
which kernel its shape takes on this device (mil_gemm_route / mil_linear_bwd_params_route with ncu = 0) and holds that against
the kernel the run is listed for; the reference then follows that route's arithmetic order.  Per block: max|got - ref| /
max|ref| <= k x max(e32, 1e-7), e32 being what the float32 restatement loses on the CPU over the same block and k the entry's
linear_ref.K_STAGE (measured, docs/lab_notes.md); guard columns hold their sentinel bit for bit, the rows behind a bucket's
64-row boundary are exactly zero.  tests/test_linear_sensitivity_host.py shows what these bounds see.  Strided runs give every
operand a leading dimension 8 floats wider than its row (inputs: NaN in the gap); outputs start full of the sentinel."""
import ctypes
import math

import pytest
import torch

import linear_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEMM, BWD, OTHER = R.gemm_runs(), R.bwd_runs(), R.other_runs()


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _in(t, strided):
    """[rows, w] float32 on the device; strided: a view of a NaN buffer GUARD floats wider."""
    if t is None:
        return None
    t = t.float()
    if not strided or t.dim() != 2:
        return t.contiguous().to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + R.GUARD), math.nan, dtype=torch.float32)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]]


def _out(rows, width, strided, init=None):
    """-> (whole buffer [rows, ld] full of the sentinel, its [rows, width] view), the view starting as `init` when given."""
    buf = torch.full((rows, width + (R.GUARD if strided else 0)), R.SENT, dtype=torch.float32, device=DEV)
    view = buf[:, :width]
    if init is not None:
        view.copy_(init.float())
    return buf, view


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ld(t):
    return 0 if t is None else t.stride(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hold(run, got, route, stage):
    c = R.run_inputs(run)
    kw = dict(route=route, inputs=c, ncu=_cu())
    return R.hold(R.tag(run) + f" route {route['kernel'] if route else run['kernel']}", {n: v.cpu() for n, v in got.items()},
                  R.restate(run, **kw), R.restate(run, torch.float32, **kw), R.blocks_of(run, route), stage)


@pytest.mark.parametrize("i", range(len(GEMM)), ids=[R.tag(r).replace(" ", "_") for r in GEMM])
def test_gemm(i):
    """mil_gemm / mil_gemm_rows / mil_gemm_aux: the smallest shapes that reach each of k_gemm_nt2, k_gemm64 (also reading
    rows_dev), k_gemm64n with and without a K split, the split last round, k_gemm<0,0> / <0,1> in one chunk, split and
    unsplit for want of a workspace, k_gemm<1,1>; bias with tanh / relu / QuickGELU, residual, accumulate and both aux modes in
    the product kernel and in k_splitk_reduce, clamped column tiles, ragged row tiles, rows_dev at 1, 64 k, 64 k + 1 and M."""
    from mil_amd import _lib, ops
    run = GEMM[i]
    route = R.lib_route_of(run, 0)
    assert route["kernel"] == run["kernel"], (R.tag(run), route)
    M, N, K, st = run["M"], run["N"], run["K"], run["strided"]
    c = R.run_inputs(run)
    A, B, res = _in(c["A"], st), _in(c["B"], st), _in(c["residual"], st)
    bias = _in(c["bias"], False)
    Cbuf, C = _out(M, N, st, c["C0"])
    rows_dev = torch.tensor([run["rows"]], dtype=torch.int32, device=DEV) if run["rows"] is not None else None
    got = {"C": Cbuf}
    if run["aux"] or st:
        L = _lib.checked()
        nws = _lib.lib().mil_gemm_workspace_floats(M, N, K, run["a_mode"]) if run["ws"] else 0
        assert nws >= route["need"], (nws, route)
        ws = torch.empty(max(nws, 1), dtype=torch.float32, device=DEV) if nws else None
        head = (_p(A), _ld(A), run["a_mode"], _p(B), _ld(B), run["b_mode"], _p(C), _ld(C), M, N, K, _p(bias), run["act"], _p(res), _ld(res),
                int(run["acc"]), _p(ws), nws)
        if run["aux"]:
            assert rows_dev is None
            if run["aux"] == 1:
                got["aux"], aux = _out(M, N, st)
            else:
                aux = _in(c["pre"], st)
            L.mil_gemm_aux(*head, _p(aux), _ld(aux), run["aux"], _st())
        elif rows_dev is not None:
            L.mil_gemm_rows(*head, _p(rows_dev), _st())
        else:
            L.mil_gemm(*head, _st())
    else:
        ops.gemm(A, run["a_mode"], B, run["b_mode"], M, N, K, out=C, bias=bias, act=run["act"], residual=res, accumulate=run["acc"],
                 split_k=run["ws"], rows_dev=rows_dev)
    torch.cuda.synchronize()
    _hold(run, got, route, "gemm")


@pytest.mark.parametrize("i", range(len(BWD)), ids=[R.tag(r).replace(" ", "_") for r in BWD])
def test_linear_bwd_params(i):
    """mil_linear_bwd_params_rows: k_gemm<1,1,true> below 4096 rows (one slice to many splits, a clamped tile in both
    directions), k_gemm_tn2 from 4096 rows with and without rows_dev (1, a count inside a chunk, the capacity; the padding
    rows of dy are not zero there: the kernel must not read them), accumulate 0 and 1, dense and strided."""
    from mil_amd import _lib
    run = BWD[i]
    route = R.lib_route_of(run, 0)
    assert route["kernel"] == run["kernel"], (R.tag(run), route)
    rows, N, K, st = run["M"], run["N"], run["K"], run["strided"]
    c = R.run_inputs(run)
    dy, x = _in(c["dy"], st), _in(c["x"], st)
    y = _in(c["y"], st) if run["act"] else None
    dWbuf, dW = _out(N, K, st, c["dW0"] if run["acc"] else None)
    db = (c["db0"].float() if run["acc"] else torch.full((N,), R.SENT)).to(DEV)
    nws = _lib.lib().mil_linear_bwd_params_workspace_floats(rows, N, K)
    assert nws >= route["need"]
    ws = torch.empty(nws, dtype=torch.float32, device=DEV)
    rows_dev = torch.tensor([run["rows"]], dtype=torch.int32, device=DEV) if run["rows"] is not None else None
    _lib.checked().mil_linear_bwd_params_rows(_p(dy), _ld(dy), _p(y), _ld(y), run["act"], _p(x), _ld(x), rows, N, K, _p(dW), _ld(dW), _p(db),
                                              int(run["acc"]), _p(ws), nws, _p(rows_dev), _st())
    torch.cuda.synchronize()
    _hold(run, {"dW": dWbuf, "db": db}, route, "bwd_params")


@pytest.mark.parametrize("i", range(len(OTHER)), ids=[R.tag(r).replace(" ", "_") for r in OTHER])
def test_colsum_act_bwd_and_the_mid_kernels(i):
    """mil_colsum (one chunk, several, both accumulate values), mil_act_bwd (tanh, relu), mil_linear_mid_fwd / _bwd on the
    32 x 32 grid (up to 4 tiles per CU) and the 64 x 64 one: ragged rows, clamped tiles, K and row counts off the group of 8."""
    from mil_amd import _lib, ops
    run = OTHER[i]
    M, N, K, st, e = run["M"], run["N"], run["K"], run["strided"], run["entry"]
    c = R.run_inputs(run)
    if e == "colsum":
        out = (c["out0"].float() if run["acc"] else torch.full((N,), R.SENT)).to(DEV)
        ops.colsum(_in(c["Y"], False), out=out, accumulate=run["acc"])
        got = {"out": out}
    elif e == "act_bwd":
        got = {"dpre": ops.act_bwd(_in(c["dy"], False), _in(c["y"], False), run["act"])}
    elif e == "mid_fwd":
        assert run["kernel"] == f"k{R.mid_ks(M, N, _cu())}"
        x, W, res = _in(c["x"], st), _in(c["W"], st), _in(c["residual"], st) if run["res"] else None
        b = _in(c["b"], False) if run["bias"] else None
        if st:
            ybuf, y = _out(M, N, True)
            _lib.checked().mil_linear_mid_fwd(_p(x), _ld(x), _p(W), _ld(W), _p(b), run["act"], _p(res), _ld(res), _p(y), _ld(y), M, N, K, _st())
        else:
            ybuf = ops.linear_mid_fwd(x, W, b, run["act"], res)
        got = {"y": ybuf}
    else:
        assert run["kernel"] == f"k{R.mid_ks(N, K, _cu())}"
        dx, dW, db = ops.linear_mid_bwd(_in(c["dy"], False), _in(c["y"], False), run["act"], _in(c["x"], False), _in(c["W"], False), True, True, True)
        got = {"dx": dx, "dW": dW, "db": db}
    torch.cuda.synchronize()
    _hold(run, got, None, e)
