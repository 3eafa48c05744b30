"""GPU: every mil_tm_* entry of csrc/transmil.hip on its own against the float64 restatement of its stage
(tests/transmil_ref.py), per block: max|got - ref| / max|ref| over a block <= k x max(e32, 1e-7), e32 being what the float32
restatement loses on the CPU over the same block.  tests/test_transmil_sensitivity_host.py shows what these bounds see; the
k of each stage (transmil_ref.K_STAGE) comes from the measured ratios in docs/lab_notes.md.  Buffers carry a sentinel
wherever an entry must not write, compared bit for bit afterwards."""
import ctypes
import math

import pytest
import torch

import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -12345.678                    # the sentinel; the bit pattern is what is compared
EINVAL = -22


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _bits_equal(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# --------------------------------------------------------------------------- mil_tm_bgemm
def _layout(kind, b, r, c):
    """(numel, offset, (stride batch, stride row, stride col)) of a [b, r, c] operand; every index stays below numel."""
    if kind == "plain":
        lay = (b * r * c, 0, (r * c, c, 1))
    elif kind == "T":                       # each batch stored column-major
        lay = (b * r * c, 0, (r * c, 1, r))
    elif kind == "padded":                  # rows 5 floats apart, 3 floats in front: gaps the entry must leave alone
        lay = (3 + b * r * (c + 5), 3, (r * (c + 5), c + 5, 1))
    elif kind == "merged_rows":             # head b's 64 columns of row-major [r, 1536] rows (q of qkv): c <= 64
        lay = (r * 1536, 0, (64, 1536, 1))
    elif kind == "merged_kT":               # element (k, j) = row j, column 512 + 64 b + k of [c, 1536] (k of qkv, read transposed)
        lay = (c * 1536, 512, (64, 1, 1536))
    elif kind == "merged_v":                # element (k, j) = row k, column 1024 + 64 b + j of [r, 1536] (v of qkv)
        lay = (r * 1536, 1024, (64, 1536, 1))
    elif kind == "merged_out":              # head b's 64 columns of [r, 512] merged-head rows
        lay = (r * 512, 0, (64, 512, 1))
    else:
        raise KeyError(kind)
    numel, off, st = lay
    assert off + (b - 1) * st[0] + (r - 1) * st[1] + (c - 1) * st[2] < numel, (kind, b, r, c)
    if kind.startswith("merged"):
        assert b <= 8 and (r if kind == "merged_kT" else c) <= 64, (kind, b, r, c)
    return lay


def _place(T, kind, fill=0.0):
    """float32 CPU buffer holding T [b, r, c] in the layout, `fill` elsewhere; and a mask of the elements it owns."""
    b, r, c = T.shape
    numel, off, st = _layout(kind, b, r, c)
    buf = torch.full((numel,), fill, dtype=torch.float32)
    torch.as_strided(buf, (b, r, c), st, off).copy_(T)
    mask = torch.zeros(numel, dtype=torch.bool)
    torch.as_strided(mask, (b, r, c), st, off).fill_(True)
    return buf, mask, off, st


def _bgemm_case(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits):
    """One call of the entry; returns (got [b, M, N], reference operands) after the sentinel check."""
    b, Mr, K = A.shape
    Nc = B.shape[2]
    abuf, _, oa, sa = _place(A, la)
    bbuf, _, ob, sb = _place(B, lb)
    cbuf, cmask, oc, sc = _place(C0, lc, SENT)
    dbuf = None
    if D is not None:
        dbuf = _place(D, lc)[0].to(DEV)
    ad, bd, cd = abuf.to(DEV), bbuf.to(DEV), cbuf.to(DEV)
    rc = _lib().mil_tm_bgemm(_p(ad[oa:]), *sa, _p(bd[ob:]), *sb, _p(cd[oc:]), *sc, _p(dbuf[oc:]) if dbuf is not None else None,
                             b, Mr, Nc, K, alpha, beta, diag, splits, _st())
    assert rc == 0, (tag, rc)
    torch.cuda.synchronize()
    out = cd.cpu()
    assert _bits_equal(out[~cmask], cbuf[~cmask]), f"{tag}: wrote outside C"
    return torch.as_strided(out, (b, Mr, Nc), sc, oc).clone()


def _bgemm_hold(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits):
    got = _bgemm_case(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits)
    Dr = D if D is not None else C0
    ref = R.bgemm(A, B, alpha, beta, Dr, diag)
    r32 = R.bgemm(A.float(), B.float(), alpha, beta, Dr.float(), diag)
    R.hold("bgemm", tag, {"C": got}, {"C": ref}, {"C": r32}, {"C": R.bgemm_blocks(A.shape[1], B.shape[2])})


@pytest.mark.parametrize("K", [1, 7, 17, 64, 100, 7936])
def test_bgemm(K):
    """K tails, ragged M and N, transposed / strided C, every epilogue, explicit splits (one, three, one above the number of
    K slices so that some are empty, split-K with diag) - C's surroundings bit-identical."""
    slices = -(-K // 16)
    for Mr in (1, 63, 65, 130):
        for Nc in (1, 63, 65, 130):
            A, B, D = R.bgemm_case(2, Mr, Nc, K)
            C0 = (D * 0.5 + 1.0).float().double()
            t = f"{Mr}x{Nc}x{K}"
            _bgemm_hold(t + " plain->padded", A, B, None, C0, "plain", "plain", "padded", 0.5, 0.0, 0.0, 1)
            _bgemm_hold(t + " T,T->T beta D diag", A, B, D, C0, "T", "T", "T", -1.0, -7.0, 15.0, 1)
            _bgemm_hold(t + " D on padded C", A, B, D, C0, "plain", "T", "padded", 1.0, 0.5, 0.0, 1)
            _bgemm_hold(t + " beta in place ->T", A, B, None, C0, "T", "plain", "T", 2.0, 0.75, -3.0, 1)
            _bgemm_hold(t + " splits 3 diag", A, B, None, C0, "plain", "plain", "plain", 1.0, 1.0, 2.5, 3)
            _bgemm_hold(t + " splits slices+1", A, B, None, C0, "T", "T", "padded", -0.5, 1.0, 0.0, slices + 1)


@pytest.mark.parametrize("K", [1, 7, 17, 64])
def test_bgemm_reads_merged_qkv_rows(K):
    """A = q and B = k^T read in place from [n, 1536] rows (sAb = 64, sAi = 1536), as the A1 / A2 / A3 logits are."""
    for Mr in (1, 63, 65, 130):
        for Nc in (1, 63, 65, 130):
            A, B, D = R.bgemm_case(8, Mr, Nc, K, seed=1)
            _bgemm_hold(f"{Mr}x{Nc}x{K} merged q, k^T", A, B, None, D, "merged_rows", "merged_kT", "padded", 0.125, 0.0, 0.0, 1)


@pytest.mark.parametrize("K", [100, 7936])
def test_bgemm_writes_merged_head_rows(K):
    """B = v read from the merged rows, C written into merged-head [M, 512] rows (sCb = 64, sCi = 512), with and without
    split-K: the neighbouring heads' columns of a row are sentinel where batch < 8."""
    for Mr in (1, 65, 130):
        for Nc in (1, 63, 64):
            for batch in (3, 8):
                A, B, D = R.bgemm_case(batch, Mr, Nc, K, seed=2)
                t = f"{batch}x{Mr}x{Nc}x{K} v->merged"
                _bgemm_hold(t, A, B, None, D, "plain", "merged_v", "merged_out", 1.0, 0.0, 0.0, 1)
                _bgemm_hold(t + " splits 4", A, B, None, D, "T", "merged_v", "merged_out", 1.0, 1.0, 0.0, 4)


def test_bgemm_einval_rules_launch_nothing():
    A, B, D = R.bgemm_case(2, 65, 63, 100)
    ad, bd, dd = _dev(A), _dev(B), _dev(D)
    c = torch.full((2, 65, 63), SENT, device=DEV)
    before = c.clone()
    sa, sb, sc = (65 * 100, 100, 1), (100 * 63, 63, 1), (65 * 63, 63, 1)

    def call(batch, beta, Dp, splits):
        return _lib().mil_tm_bgemm(_p(ad), *sa, _p(bd), *sb, _p(c), *sc, _p(Dp), batch, 65, 63, 100, 1.0, beta, 0.0, splits, _st())
    assert call(2, 0.0, None, 2) == EINVAL            # split-K adds into C: beta must be 1
    assert call(2, 0.5, None, 2) == EINVAL
    assert call(2, 1.0, dd, 2) == EINVAL              # ... and D must be C
    assert call(2, 1.0, None, 32768) == EINVAL        # batch x splits > 65535
    assert call(2, 1.0, None, 0) == EINVAL
    torch.cuda.synchronize()
    assert _bits_equal(c, before)


# --------------------------------------------------------------------------- softmax rows
@pytest.mark.parametrize("rows", [1, 5, 2051])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 257, 7936])
def test_softmax_rows(rows, cols):
    x, dp = R.softmax_case(rows, cols)
    blocks = {"all": (Ellipsis,), "big": (slice(0, None, 4),), "const": (slice(1 % rows, 1 % rows + 1),)}
    buf = torch.full((rows + 3, cols), SENT)
    buf[:rows] = x.float()
    d = buf.to(DEV)
    assert _lib().mil_tm_softmax_rows(_p(d), rows, cols, _st()) == 0
    torch.cuda.synchronize()
    got = d.cpu()
    assert _bits_equal(got[rows:], buf[rows:]), "softmax wrote behind its rows"
    ref = R.softmax_rows(x)
    assert bool((got[:rows][torch.isinf(x)] == 0).all())                       # -inf logits: exactly 0
    assert bool(torch.isfinite(got[:rows]).all())
    R.hold("softmax", f"fwd {rows}x{cols}", {"p": got[:rows]}, {"p": ref}, {"p": R.softmax_rows(x.float())}, {"p": blocks})
    # backward, on the float32 rounding of the reference's p
    p = ref.float()
    dbuf = torch.full((rows + 3, cols), SENT)
    dbuf[:rows] = dp.float()
    pd, dd = p.to(DEV), dbuf.to(DEV)
    assert _lib().mil_tm_softmax_rows_bwd(_p(pd), _p(dd), rows, cols, _st()) == 0
    torch.cuda.synchronize()
    gd = dd.cpu()
    assert _bits_equal(gd[rows:], dbuf[rows:]), "softmax backward wrote behind its rows"
    R.hold("softmax", f"bwd {rows}x{cols}", {"dp": gd[:rows]}, {"dp": R.softmax_rows_bwd(p.double(), dp)},
           {"dp": R.softmax_rows_bwd(p, dp.float())}, {"dp": blocks})


# --------------------------------------------------------------------------- landmarks
@pytest.mark.parametrize("l", [1, 2, 31])
def test_landmarks(l):
    n = R.M * l
    g = torch.Generator().manual_seed(50 + l)
    qkv = torch.randn((n, 1536), generator=g).double()
    qs = R.DH ** -0.5
    qd = _dev(qkv)
    qL = torch.full((R.H * R.M * R.DH + 64,), SENT, device=DEV)
    kL = torch.full((R.H * R.M * R.DH + 64,), SENT, device=DEV)
    assert _lib().mil_tm_landmarks(_p(qd), n, qs, _p(qL), _p(kL), _st()) == 0
    torch.cuda.synchronize()
    assert bool((qL[-64:] == SENT).all()) and bool((kL[-64:] == SENT).all())
    rq, rk = R.landmarks(qkv, l)
    fq, fk = R.landmarks(qkv.float(), l)
    got = {"qL": qL[:-64].reshape(R.H, R.M, R.DH), "kL": kL[:-64].reshape(R.H, R.M, R.DH)}
    R.hold("landmarks", f"fwd l {l}", got, {"qL": rq, "kL": rk}, {"qL": fq, "kL": fk}, {"qL": R.whole(), "kL": R.whole()})
    # backward adds onto what dqkv holds and leaves the v columns alone
    dqL = torch.randn((R.H, R.M, R.DH), generator=g).double()
    dkL = torch.randn((R.H, R.M, R.DH), generator=g).double()
    d0 = torch.randn((n + 1, 1536), generator=g)
    d0[n] = SENT
    dd = d0.to(DEV)
    assert _lib().mil_tm_landmarks_bwd(_p(_dev(dqL)), _p(_dev(dkL)), n, qs, _p(dd), _st()) == 0
    torch.cuda.synchronize()
    gd = dd.cpu()
    assert _bits_equal(gd[:, 1024:], d0[:, 1024:]) and _bits_equal(gd[n], d0[n])
    ref = d0[:n, :1024].double() + R.landmarks_bwd(dqL, dkL, l)
    r32 = d0[:n, :1024] + R.landmarks_bwd(dqL.float(), dkL.float(), l)
    blocks = {k: v for k, v in R.qkv_blocks(n).items() if k[0] in "qk" and "pad" not in k}
    R.hold("landmarks", f"bwd l {l}", {"dqk": gd[:n, :1024]}, {"dqk": ref}, {"dqk": r32}, {"dqk": blocks})


# --------------------------------------------------------------------------- start of the pseudo-inverse
def _pinv_init(a2):
    ad = _dev(a2)
    scale = torch.full((3 + 2 * R.H + 4,), SENT, device=DEV)
    arg = torch.full((1 + R.H + 4,), -7, device=DEV, dtype=torch.int32)
    Z = torch.full((R.H * R.M * R.M + 64,), SENT, device=DEV)
    assert _lib().mil_tm_pinv_init(_p(ad), _p(scale), _p(arg), _p(Z), _st()) == 0
    torch.cuda.synchronize()
    assert bool((scale[-4:] == SENT).all()) and bool((arg[-4:] == -7).all()) and bool((Z[-64:] == SENT).all())
    return ad, scale[:-4], arg[:-4], Z[:-64].reshape(R.H, R.M, R.M)


def test_pinv_init():
    """Largest column sum in head 3, largest row sum in head 5: scale, the per-head maxima, arg and Z0; then the backward,
    through the row-softmax backward, against float64 autograd of A2^T / (max x max)."""
    a2, dZ = R.pinv_case(row_head=5)
    _, scale, arg, Z = _pinv_init(a2)
    ref, r32 = R.pinv_run(a2, dZ), R.pinv_run(a2, dZ, torch.float32)
    csum, rsum = a2.sum(-2), a2.sum(-1)
    assert int(rsum.amax(-1).argmax()) == 5 and int(csum.amax(-1).argmax()) == 3
    assert arg.cpu().tolist() == [3 * R.M + 77] + [h * R.M + int(csum[h].argmax()) for h in range(R.H)]
    got = {"scale": scale[:3], "row_max": scale[3:3 + R.H], "col_max": scale[3 + R.H:], "Z0": Z}
    R.hold("pinv_init", "fwd", got, ref, r32, {k: R.whole() for k in got})

    a2, dZ = R.pinv_case()                                    # rows exactly as the softmax leaves them
    ad, scale, arg, Z = _pinv_init(a2)
    assert int(arg[0]) == 3 * R.M + 77
    g = torch.Generator().manual_seed(6)
    dA0 = torch.randn((R.H, R.M, R.M), generator=g)           # dA2 comes in holding the six iterations' share
    dA = torch.cat([dA0.reshape(-1), torch.full((64,), SENT)]).to(DEV)
    ws = torch.zeros(1, device=DEV)
    assert _lib().mil_tm_pinv_init_bwd(_p(_dev(dZ)), _p(Z.contiguous()), _p(scale), _p(arg), _p(dA), _p(ws), _st()) == 0
    assert _lib().mil_tm_softmax_rows_bwd(_p(ad), _p(dA), R.H * R.M, R.M, _st()) == 0
    torch.cuda.synchronize()
    assert bool((dA[-64:] == SENT).all())
    ref, r32 = R.pinv_run(a2, dZ), R.pinv_run(a2, dZ, torch.float32)
    want = {"dS2": ref["dS2"] + R.softmax_rows_bwd(a2, dA0.double())}
    w32 = {"dS2": r32["dS2"] + R.softmax_rows_bwd(a2.float(), dA0)}
    R.hold("pinv_init", "bwd", {"dS2": dA[:-64].reshape(R.H, R.M, R.M)}, want, w32, {"dS2": R.whole()})


def test_pinv_init_first_on_ties():
    """Two exactly equal largest column sums inside head 2 (columns 17 and 200) and the same again in head 6: arg is the
    first.  Entries are multiples of 2^-13, so every sum is exact in float32 in any order."""
    g = torch.Generator().manual_seed(8)
    a2 = torch.randint(1, 8, (R.H, R.M, R.M), generator=g).double() / 8192
    a2[2, :, 17] += 1.0 / 1024
    a2[2, :, 200] = a2[2, :, 17]
    a2[6, :, 5] = a2[2, :, 17]
    _, scale, arg, Z = _pinv_init(a2)
    ref = R.z0(a2)
    assert ref["arg"] == 2 * R.M + 17
    assert int(arg[0]) == 2 * R.M + 17 and int(arg[1 + 2]) == 2 * R.M + 17 and int(arg[1 + 6]) == 6 * R.M + 5
    assert torch.equal(scale[3:3 + R.H].cpu().double(), ref["row_max"]) and torch.equal(scale[3 + R.H:].cpu().double(), ref["col_max"])
    assert torch.equal(scale[:3].cpu().double(), ref["scale"])
    r32 = R.z0(a2.float())
    R.hold("pinv_init", "ties fwd", {"Z0": Z}, ref, r32, {"Z0": R.whole()})


# --------------------------------------------------------------------------- residual conv
@pytest.mark.parametrize("n", [1, 16, 33, 255, 256, 257, 600, 7936])
def test_resconv(n):
    c = R.resconv_case(n)
    qd, wd = _dev(c["qkv"]), _dev(c["w"])
    out = torch.cat([c["out0"].float(), torch.full((1, 512), SENT)]).to(DEV)
    assert _lib().mil_tm_resconv(_p(qd), _p(wd), n, _p(out), _st()) == 0
    d0 = torch.cat([c["dqkv0"].float(), torch.full((1, 1536), SENT)])
    dq, dw = d0.to(DEV), _dev(c["dw0"])
    assert _lib().mil_tm_resconv_bwd(_p(_dev(c["dout"])), _p(qd), _p(wd), n, _p(dq), _p(dw), _st()) == 0
    torch.cuda.synchronize()
    gq = dq.cpu()
    assert bool((out[n] == SENT).all()) and _bits_equal(gq[n], d0[n])
    assert _bits_equal(gq[:, :1024], d0[:, :1024]), "the q / k columns of dqkv moved"
    got = {"out": out[:n], "dv": gq[:n, 1024:], "dw": dw}
    R.hold("resconv", f"n {n}", got, R.resconv_run(c), R.resconv_run(c, torch.float32), R.resconv_blocks(n))


# --------------------------------------------------------------------------- PPEG
@pytest.mark.parametrize("s", [1, 2, 3, 7, 8, 9, 16, 17, 125])
def test_ppeg(s):
    p, x, dy = R.ppeg_case(s)
    rows = 1 + s * s
    g = torch.Generator().manual_seed(70 + s)
    W = [_dev(p["pos_layer." + n]) for n in R.PPEG_NAMES]
    xd = _dev(x)
    y = torch.full((rows + 1, 512), SENT, device=DEV)
    assert _lib().mil_tm_ppeg_fwd(_p(xd), s, *[_p(t) for t in W], _p(y), _st()) == 0
    dx = torch.full((rows + 1, 512), SENT, device=DEV)
    dWf0 = torch.randn((512, 1, 7, 7), generator=g)            # the gradients add onto what the buffers hold
    db0 = torch.randn(512, generator=g)
    dWf, db = dWf0.to(DEV), db0.to(DEV)
    assert _lib().mil_tm_ppeg_bwd(_p(_dev(dy)), _p(xd), s, _p(W[0]), _p(W[2]), _p(W[4]), _p(dx), _p(dWf), _p(db), _st()) == 0
    torch.cuda.synchronize()
    assert bool((y[rows] == SENT).all()) and bool((dx[rows] == SENT).all())
    assert torch.equal(y[0].cpu(), x[0].float())                 # cls passes through, both ways
    assert torch.equal(dx[0].cpu(), dy[0].float())
    cut = {"proj": slice(0, 7), "proj1": slice(1, 6), "proj2": slice(2, 5)}
    got = {"y": y[:rows], "dx": dx[:rows]}
    ref, r32 = R.ppeg_run(p, x, dy, s), R.ppeg_run(p, x, dy, s, torch.float32)
    for name, sl in cut.items():                                 # dW7 is the whole map, dW5 / dW3 its centre; one db
        got[f"d{name}.weight"] = dWf[:, :, sl, sl]
        got[f"d{name}.bias"] = db
        for r, cast in ((ref, torch.float64), (r32, torch.float32)):
            r[f"d{name}.weight"] = r[f"d{name}.weight"] + dWf0[:, :, sl, sl].to(cast)
            r[f"d{name}.bias"] = r[f"d{name}.bias"] + db0.to(cast)
    R.hold("ppeg", f"s {s}", got, ref, r32, R.ppeg_all_blocks(s))


# --------------------------------------------------------------------------- row gather and the sequence index
@pytest.mark.parametrize("E", [1, 255, 512, 768])
def test_row_gather(E):
    g = torch.Generator().manual_seed(90 + E)
    src = torch.randn((9, E), generator=g)
    extra = torch.randn(E, generator=g)
    idx = [-2, 0, 3, -1, 8, 3, 3, -2, -1, 5]
    rows = len(idx)
    id_d = torch.tensor(idx, dtype=torch.int32, device=DEV)
    sd, ed = src.to(DEV), extra.to(DEV)
    for ex in (ed, None):                                        # a null `extra`: the -2 rows read as zeros, like -1
        dst = torch.full((rows + 1, E), SENT, device=DEV)
        assert _lib().mil_tm_row_gather(_p(sd), _p(ex), _p(id_d), rows, E, _p(dst), _st()) == 0
        torch.cuda.synchronize()
        zero = torch.zeros(E)
        want = torch.stack([src[i] if i >= 0 else (extra if i == -2 and ex is not None else zero) for i in idx])
        assert torch.equal(dst[:rows].cpu(), want) and bool((dst[rows] == SENT).all())
    # backward: integer-valued gradients, so the atomic sums are exact in any order
    dd = torch.randint(-8, 9, (rows, E), generator=g).float()
    want_src = torch.zeros((9, E))
    want_ex = torch.zeros(E)
    for r, i in enumerate(idx):
        if i >= 0:
            want_src[i] += dd[r]
        elif i == -2:
            want_ex += dd[r]
    for with_extra in (True, False):
        dsrc = torch.zeros((9 + 1, E), device=DEV)
        dsrc[9] = SENT
        dex = torch.zeros(E, device=DEV) if with_extra else None
        assert _lib().mil_tm_row_gather_bwd(_p(dd.to(DEV)), _p(id_d), rows, E, _p(dsrc), _p(dex), _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dsrc[:9].cpu(), want_src) and bool((dsrc[9] == SENT).all())      # rows 1, 2, 4, 6, 7: no gradient
        if with_extra:
            assert torch.equal(dex.cpu(), want_ex)


def test_seq_index_against_restatement():
    from mil_amd import ops
    for lengths, sides in (([7, 250, 1], [3, 16, 1]), ([256], [16]), ([257], [17]), ([3, 9], [3, 3])):
        want, rows, flag = R.seq_index(lengths, sides)
        idx = torch.full((len(want) + 4,), -9, dtype=torch.int32, device=DEV)
        rd = torch.zeros(1, dtype=torch.int32, device=DEV)
        fd = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.tm_seq_index(torch.tensor(lengths, dtype=torch.int32, device=DEV), sides, idx[:len(want)], rows_dev=rd, flag=fd)
        torch.cuda.synchronize()
        assert idx.cpu().tolist() == want + [-9] * 4 and int(rd) == rows and int(fd) == flag, (lengths, sides)


# --------------------------------------------------------------------------- the whole core
@pytest.mark.parametrize("n_pad,peak", [(256, 1.0), (512, 1.0), (2048, 1.0), (7936, 1.0), (512, R.PEAK), (7936, R.PEAK)])
def test_nystrom_core(n_pad, peak):
    """out, dqkv by q / k / v column group (each also over the pad rows and the conv halo) and dw.  The peaked input has
    q and k scaled by transmil_ref.PEAK."""
    from mil_amd import ops
    qkv, w, dO, pad = R.core_case(n_pad, peak)
    qd, wd = _dev(qkv).requires_grad_(True), _dev(w).requires_grad_(True)
    o, _ = ops.nystrom_core(qd, wd)
    o.backward(_dev(dO))
    torch.cuda.synchronize()
    got = {"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad.reshape(R.H, R.CONV)}
    assert bool(torch.isfinite(qd.grad).all())
    R.hold("core", f"n_pad {n_pad} peak {peak}", got, R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32),
           R.core_blocks(n_pad, pad))
