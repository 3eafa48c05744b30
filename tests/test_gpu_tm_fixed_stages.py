"""GPU: every mil_tm_*_fixed entry of csrc/transmil.hip on its own, through the C ABI.  Each is held per block to the float64
restatement of its stage with transmil_ref.hold and the K_STAGE values of the atomic entries (a fixed-order chunked sum is a
reordering of the same terms), runs twice into fresh buffers with equal bits, and leaves the sentinels around its outputs and
behind the `_ws_floats` extent of its workspace bit-identical."""
import ctypes

import pytest
import torch

import tm_fixed_ref as F
import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = F.SENT
TAIL = 64                            # sentinel floats behind a workspace's `_ws_floats` extent


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _ws(nfloats):
    """A workspace of nfloats (NaN: a partial that is read without having been written shows) + TAIL sentinel floats."""
    ws = torch.full((int(nfloats) + TAIL,), SENT, device=DEV)
    ws[:int(nfloats)] = float("nan")
    return ws


def _ws_tail_ok(ws):
    return bool((ws[-TAIL:].cpu().view(torch.int32) == torch.tensor(SENT).view(torch.int32)).all())


# --------------------------------------------------------------------------- mil_tm_bgemm_fixed
def _bgemm_run(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits, fixed=True):
    """One call into fresh buffers -> C [b, M, N] on the CPU, after the sentinel checks around C and behind the workspace."""
    b, Mr, K = A.shape
    Nc = B.shape[2]
    abuf, _, oa, sa = F.place(A, la)
    bbuf, _, ob, sb = F.place(B, lb)
    cbuf, cmask, oc, sc = F.place(C0, lc, SENT)
    dbuf = F.place(D, lc)[0].to(DEV) if D is not None else None
    ad, bd, cd = abuf.to(DEV), bbuf.to(DEV), cbuf.to(DEV)
    args = (_p(ad[oa:]), *sa, _p(bd[ob:]), *sb, _p(cd[oc:]), *sc, _p(dbuf[oc:]) if dbuf is not None else None, b, Mr, Nc, K,
            alpha, beta, diag, splits)
    if fixed:
        n = _lib().mil_tm_bgemm_ws_floats(b, Mr, Nc, splits)
        assert n == F.ws_floats("mil_tm_bgemm_ws_floats", b, Mr, Nc, splits), (tag, n)
        ws = _ws(n)
        rc = _lib().mil_tm_bgemm_fixed(*args, _p(ws), _st())
    else:
        rc = _lib().mil_tm_bgemm(*args, _st())
    assert rc == 0, (tag, rc)
    torch.cuda.synchronize()
    out = cd.cpu()
    assert F.bits_equal(out[~cmask], cbuf[~cmask]), f"{tag}: wrote outside C"
    if fixed:
        assert _ws_tail_ok(ws), f"{tag}: wrote behind the workspace"
        if splits == 1:
            assert bool(torch.isnan(ws[:-TAIL]).all()) or n == 0, f"{tag}: splits 1 touched the workspace"
    return torch.as_strided(out, (b, Mr, Nc), sc, oc).clone()


def _bgemm_hold(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits):
    got = _bgemm_run(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits)
    again = _bgemm_run(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits)
    assert F.bits_equal(got, again), f"{tag}: two runs differ"
    Dr = D if D is not None else C0
    ref = R.bgemm(A, B, alpha, beta, Dr, diag)
    r32 = R.bgemm(A.float(), B.float(), alpha, beta, Dr.float(), diag)
    R.hold("bgemm", tag, {"C": got}, {"C": ref}, {"C": r32}, {"C": R.bgemm_blocks(A.shape[1], B.shape[2])})
    return got


@pytest.mark.parametrize("K", [17, 100, 7936])
def test_bgemm_fixed(K):
    """K tails, ragged M and N, the four layouts of C, beta 0 / 1 / -7 with D, diag with split-K, splits one, three and one
    above the number of K slices (some splits empty: they store zeros)."""
    slices = -(-K // 16)
    for Mr in (1, 63, 65, 130):
        for Nc in (1, 63, 65, 130):
            A, B, D = R.bgemm_case(2, Mr, Nc, K)
            C0 = (D * 0.5 + 1.0).float().double()
            t = f"{Mr}x{Nc}x{K}"
            for splits in (1, 3, slices + 1):
                _bgemm_hold(f"{t} plain->padded beta 0 splits {splits}", A, B, None, C0, "plain", "plain", "padded", 0.5, 0.0, 0.0,
                            splits)
            _bgemm_hold(t + " T,T->T beta 1 diag splits 3", A, B, None, C0, "T", "T", "T", 1.0, 1.0, 2.5, 3)
            _bgemm_hold(t + " plain,T->plain beta 1 splits slices+1", A, B, None, C0, "plain", "T", "plain", -0.5, 1.0, 0.0, slices + 1)
            for splits in (3, slices + 1):
                _bgemm_hold(f"{t} beta -7 D diag 15 ->padded splits {splits}", A, B, D, C0, "plain", "T", "padded", -1.0, -7.0, 15.0,
                            splits)
            if Nc <= 64:
                _bgemm_hold(t + " ->merged_out splits 3", A, B, None, C0, "T", "plain", "merged_out", 1.0, 0.0, 0.0, 3)
            # one split: the launch of mil_tm_bgemm itself
            for la, lb, lc, Dd, alpha, beta, diag in (("T", "T", "T", D, -1.0, -7.0, 15.0), ("plain", "plain", "padded", None, 2.0, 0.75, -3.0)):
                one = _bgemm_run(t + " splits 1", A, B, Dd, C0, la, lb, lc, alpha, beta, diag, 1)
                old = _bgemm_run(t + " mil_tm_bgemm", A, B, Dd, C0, la, lb, lc, alpha, beta, diag, 1, fixed=False)
                assert F.bits_equal(one, old), f"{t}: splits 1 differs from mil_tm_bgemm"


def test_bgemm_fixed_einval_rules_launch_nothing():
    A, B, _ = R.bgemm_case(2, 65, 63, 100)
    ad, bd = _dev(A), _dev(B)
    c = torch.full((2, 65, 63), SENT, device=DEV)
    ws = torch.full((3 * 2 * 65 * 63,), SENT, device=DEV)
    sa, sb, sc = (65 * 100, 100, 1), (100 * 63, 63, 1), (65 * 63, 63, 1)

    def call(splits, wsp, cp=c):
        return _lib().mil_tm_bgemm_fixed(_p(ad), *sa, _p(bd), *sb, _p(cp), *sc, None, 2, 65, 63, 100, 1.0, 0.0, 0.0, splits, _p(wsp), _st())
    assert call(3, None) == -22                       # split-K needs its workspace
    assert call(0, ws) == -22
    assert call(32768, ws) == -22                     # batch x splits > 65535
    assert call(3, ws, None) == -22
    torch.cuda.synchronize()
    assert bool((c == SENT).all()) and bool((ws == SENT).all())


# --------------------------------------------------------------------------- mil_tm_row_gather_bwd_fixed
def _gather_bwd(dd, idx, src_rows, with_extra=True):
    rows, E = dd.shape
    id_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    dsrc = torch.full((src_rows + 1, E), SENT, device=DEV)          # not zeroed: every row is written
    dex = torch.full((E + 8,), SENT, device=DEV) if with_extra else None
    n = _lib().mil_tm_row_gather_ws_floats(src_rows)
    assert n == F.ws_floats("mil_tm_row_gather_ws_floats", src_rows)
    ws = _ws(n)
    rc = _lib().mil_tm_row_gather_bwd_fixed(_p(dd.to(DEV)), _p(id_d), rows, E, _p(dsrc), src_rows, _p(dex), _p(ws), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((dsrc[src_rows] == SENT).all()) and _ws_tail_ok(ws)
    if with_extra:
        assert bool((dex[E:] == SENT).all())
    return dsrc[:src_rows].cpu(), dex[:E].cpu() if with_extra else None


@pytest.mark.parametrize("lengths", [[7], [2, 3, 5], [250, 7, 300, 16]])
def test_row_gather_bwd_fixed_on_the_sequence_index(lengths):
    """The index of the sequence assembly (repeated rows named twice, one -2 row per bag): bit-equal to the ascending float32
    sum on the CPU, twice, with and without dextra.  That sum IS the float32 restatement of the stage, so the float64 bound
    of the other stages holds here with ratio 0 and is not restated."""
    from mil_amd.model.dim1.TransMIL import seq_index
    idx, src_rows = seq_index(lengths), sum(lengths)
    assert F.max_naming(idx, src_rows) <= 2
    g = torch.Generator().manual_seed(len(idx))
    dd = torch.randn((len(idx), 512), generator=g)
    want_src, want_ex = F.gather_bwd_ordered(dd, idx, src_rows)
    for with_extra in (True, False):
        a_src, a_ex = _gather_bwd(dd, idx, src_rows, with_extra)
        b_src, b_ex = _gather_bwd(dd, idx, src_rows, with_extra)
        assert F.bits_equal(a_src, b_src) and F.bits_equal(a_src, want_src)
        if with_extra:
            assert F.bits_equal(a_ex, b_ex) and F.bits_equal(a_ex, want_ex)


@pytest.mark.parametrize("E", [1, 255, 512, 768])
def test_row_gather_bwd_fixed_any_index(E):
    """A hand-made index: row 3 named four times (the scan between its first and last row), row 5 twice, rows 1, 2, 4, 6, 7
    never (zeros), five -2 rows, two -1 rows, the matches spread over more than one 256-entry chunk of the scan."""
    idx = [-2, 0, 3, -1, 8, 3, -2, 5] + [-1] * 300 + [-2, 3, 5, -2] + [-1] * 290 + [3, -2, -1]
    assert idx.count(3) == 4 and idx.count(-2) == 5
    g = torch.Generator().manual_seed(90 + E)
    dd = torch.randn((len(idx), E), generator=g)
    want_src, want_ex = F.gather_bwd_ordered(dd, idx, 9)
    for with_extra in (True, False):
        a_src, a_ex = _gather_bwd(dd, idx, 9, with_extra)
        b_src, b_ex = _gather_bwd(dd, idx, 9, with_extra)
        assert F.bits_equal(a_src, want_src) and F.bits_equal(b_src, want_src)
        assert bool((a_src[[1, 2, 4, 6, 7]] == 0).all())
        if with_extra:
            assert F.bits_equal(a_ex, want_ex) and F.bits_equal(b_ex, want_ex)


# --------------------------------------------------------------------------- mil_tm_pinv_init_bwd_fixed
def _pinv_bwd(a2, dZ, dA0):
    ad = _dev(a2)
    scale = torch.empty(3 + 2 * R.H, device=DEV)
    arg = torch.empty(1 + R.H, device=DEV, dtype=torch.int32)
    Z = torch.empty((R.H, R.M, R.M), device=DEV)
    assert _lib().mil_tm_pinv_init(_p(ad), _p(scale), _p(arg), _p(Z), _st()) == 0
    dA = torch.cat([dA0.reshape(-1), torch.full((64,), SENT)]).to(DEV)
    n = _lib().mil_tm_pinv_ws_floats()
    assert n == F.ws_floats("mil_tm_pinv_ws_floats")
    ws = _ws(n)
    assert _lib().mil_tm_pinv_init_bwd_fixed(_p(_dev(dZ)), _p(Z), _p(scale), _p(arg), _p(dA), _p(ws), _st()) == 0
    assert _lib().mil_tm_softmax_rows_bwd(_p(ad), _p(dA), R.H * R.M, R.M, _st()) == 0
    torch.cuda.synchronize()
    assert bool((dA[-64:] == SENT).all()) and _ws_tail_ok(ws)
    assert bool(torch.isfinite(ws[:n]).all())                       # all 256 chunk sums were stored
    return dA[:-64].reshape(R.H, R.M, R.M).cpu()


def test_pinv_init_bwd_fixed():
    a2, dZ = R.pinv_case()
    dA0 = torch.randn((R.H, R.M, R.M), generator=torch.Generator().manual_seed(6))
    got, again = _pinv_bwd(a2, dZ, dA0), _pinv_bwd(a2, dZ, dA0)
    assert F.bits_equal(got, again)
    ref, r32 = R.pinv_run(a2, dZ), R.pinv_run(a2, dZ, torch.float32)
    want = {"dS2": ref["dS2"] + R.softmax_rows_bwd(a2, dA0.double())}
    w32 = {"dS2": r32["dS2"] + R.softmax_rows_bwd(a2.float(), dA0)}
    R.hold("pinv_init", "bwd fixed", {"dS2": got}, want, w32, {"dS2": R.whole()})


# --------------------------------------------------------------------------- mil_tm_resconv_bwd_fixed
def _resconv_bwd(c, n):
    qd, wd = _dev(c["qkv"]), _dev(c["w"])
    d0 = torch.cat([c["dqkv0"].float(), torch.full((1, 1536), SENT)])
    dq = d0.to(DEV)
    dw = torch.full((R.H * R.CONV + 8,), SENT, device=DEV)          # not zeroed: the fold overwrites [8, 33]
    nws = _lib().mil_tm_resconv_ws_floats(n)
    assert nws == F.ws_floats("mil_tm_resconv_ws_floats", n)
    ws = _ws(nws)
    assert _lib().mil_tm_resconv_bwd_fixed(_p(_dev(c["dout"])), _p(qd), _p(wd), n, _p(dq), _p(dw), _p(ws), _st()) == 0
    torch.cuda.synchronize()
    gq = dq.cpu()
    assert F.bits_equal(gq[n], d0[n]) and F.bits_equal(gq[:, :1024], d0[:, :1024]), "rows or columns outside dv moved"
    assert bool((dw[R.H * R.CONV:] == SENT).all()) and _ws_tail_ok(ws)
    return {"dv": gq[:n, 1024:], "dw": dw[:R.H * R.CONV].reshape(R.H, R.CONV).cpu()}


@pytest.mark.parametrize("n", [256, 512, 1280])
def test_resconv_bwd_fixed(n):
    """One chunk of 256 rows, two, five.  dw is overwritten, so the restatement starts it from zero."""
    c = R.resconv_case(n)
    c["dw0"] = torch.zeros_like(c["dw0"])
    got, again = _resconv_bwd(c, n), _resconv_bwd(c, n)
    assert F.bits_equal(got["dw"], again["dw"]) and F.bits_equal(got["dv"], again["dv"])
    blocks = {k: v for k, v in R.resconv_blocks(n).items() if k != "out"}
    R.hold("resconv", f"fixed n {n}", got, R.resconv_run(c), R.resconv_run(c, torch.float32), blocks)


# --------------------------------------------------------------------------- mil_tm_ppeg_bwd_fixed
def _ppeg_bwd(p, x, dy, s):
    rows = 1 + s * s
    W = [_dev(p["pos_layer." + n]) for n in R.PPEG_NAMES]
    dx = torch.full((rows + 1, 512), SENT, device=DEV)
    dWf = torch.full((512 * 49 + 8,), SENT, device=DEV)             # not zeroed: the folds overwrite both
    db = torch.full((512 + 8,), SENT, device=DEV)
    nws = _lib().mil_tm_ppeg_ws_floats(s)
    assert nws == F.ws_floats("mil_tm_ppeg_ws_floats", s)
    ws = _ws(nws)
    assert _lib().mil_tm_ppeg_bwd_fixed(_p(_dev(dy)), _p(_dev(x)), s, _p(W[0]), _p(W[2]), _p(W[4]), _p(dx), _p(dWf), _p(db), _p(ws),
                                        _st()) == 0
    torch.cuda.synchronize()
    assert bool((dx[rows] == SENT).all()) and bool((dWf[512 * 49:] == SENT).all()) and bool((db[512:] == SENT).all())
    assert _ws_tail_ok(ws)
    assert torch.equal(dx[0].cpu(), dy[0].float())                  # cls passes through
    return dx[:rows].cpu(), dWf[:512 * 49].reshape(512, 1, 7, 7).cpu(), db[:512].cpu()


@pytest.mark.parametrize("s", [1, 3, 8, 9, 18])
def test_ppeg_bwd_fixed(s):
    """One chunk of 8 grid rows (s 1, 3, 8), a chunk and a tail (9), two chunks and a tail (18)."""
    p, x, dy = R.ppeg_case(s)
    dx, dWf, db = _ppeg_bwd(p, x, dy, s)
    dx2, dWf2, db2 = _ppeg_bwd(p, x, dy, s)
    assert F.bits_equal(dx, dx2) and F.bits_equal(dWf, dWf2) and F.bits_equal(db, db2)
    cut = {"proj": slice(0, 7), "proj1": slice(1, 6), "proj2": slice(2, 5)}
    got = {"dx": dx}
    for name, sl in cut.items():                                    # dW7 is the whole map, dW5 / dW3 its centre; one db
        got[f"d{name}.weight"] = dWf[:, :, sl, sl]
        got[f"d{name}.bias"] = db
    blocks = {k: v for k, v in R.ppeg_all_blocks(s).items() if k != "y"}
    R.hold("ppeg", f"fixed s {s}", got, R.ppeg_run(p, x, dy, s), R.ppeg_run(p, x, dy, s, torch.float32), blocks)
