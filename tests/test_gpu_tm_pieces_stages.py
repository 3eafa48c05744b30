"""GPU: mil_tm_bgemm_pieces and mil_tm_bgemm_pieces_fixed (csrc/tm_bgemm_pieces.hip, three-piece split-bf16 MFMA) on their own
against the float64 restatement of the product (tests/transmil_ref.py), per block: max|got - ref| / max|ref| over a block
<= k x max(e32, 1e-7), e32 being what the float32 restatement loses on the CPU over the same block - the bound of mil_tm_bgemm,
k from tm_pieces_ref.K_STAGE (docs/lab_notes.md has the measured ratios).  Both tile forms (64 x 64 for M <= 256, 128 x 64
above) and their edges, every layout and epilogue of test_gpu_transmil_stages.test_bgemm, the merged-row operands, both split-K
forms; buffers carry a sentinel wherever an entry must not write, compared bit for bit afterwards.  Then the one place where
products feed products 24 deep: the pseudo-inverse chain and its backward sweep, per head."""
import pytest
import torch

import tm_pieces_ref as P
import transmil_ref as R
import test_gpu_transmil_stages as S

pytestmark = pytest.mark.gpu

DEV = S.DEV
SENT, EINVAL = S.SENT, S.EINVAL
SHAPES = [(64, 64), (65, 63), (200, 130), (257, 64)]          # 257 rows: the 128-row tile, its last tile one row deep
SLICE = 32                                                    # depth of a K slice of k_tm_bgemm_pieces: what split-K divides
_lib, _p, _st = S._lib, S._p, S._st


def _call(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits, fixed=False, pieces=3, want_rc=0):
    """One call of the entry on operands placed in their layouts; returns C [b, M, N] after the sentinel checks."""
    b, Mr, K = A.shape
    Nc = B.shape[2]
    abuf, _, oa, sa = S._place(A, la)
    bbuf, _, ob, sb = S._place(B, lb)
    cbuf, cmask, oc, sc = S._place(C0, lc, SENT)
    dbuf = S._place(D, lc)[0].to(DEV) if D is not None else None
    ad, bd, cd = abuf.to(DEV), bbuf.to(DEV), cbuf.to(DEV)
    args = (_p(ad[oa:]), *sa, _p(bd[ob:]), *sb, _p(cd[oc:]), *sc, _p(dbuf[oc:]) if dbuf is not None else None, b, Mr, Nc, K,
            alpha, beta, diag, splits, pieces)
    if fixed:
        n = _lib().mil_tm_bgemm_ws_floats(b, Mr, Nc, splits)
        assert n == (splits * b * Mr * Nc if splits > 1 else 0)
        ws = torch.full((n + 64,), SENT, device=DEV)
        rc = _lib().mil_tm_bgemm_pieces_fixed(*args, _p(ws), _st())
    else:
        rc = _lib().mil_tm_bgemm_pieces(*args, _st())
    assert rc == want_rc, (tag, rc)
    torch.cuda.synchronize()
    out = cd.cpu()
    if fixed:
        assert bool((ws[n:] == SENT).all()), f"{tag}: wrote behind the workspace"
    if want_rc != 0:
        assert S._bits_equal(out, cbuf), f"{tag}: a refused call wrote"
        return None
    assert S._bits_equal(out[~cmask], cbuf[~cmask]), f"{tag}: wrote outside C"
    return torch.as_strided(out, (b, Mr, Nc), sc, oc).clone()


def _hold(stage, tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits, fixed=False):
    got = _call(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits, fixed)
    if fixed:
        again = _call(tag, A, B, D, C0, la, lb, lc, alpha, beta, diag, splits, fixed)
        assert S._bits_equal(got, again), f"{tag}: two fixed-order calls differ"
    Dr = D if D is not None else C0
    ref = R.bgemm(A, B, alpha, beta, Dr, diag)
    r32 = R.bgemm(A.float(), B.float(), alpha, beta, Dr.float(), diag)
    P.hold(stage, tag, {"C": got}, {"C": ref}, {"C": r32}, {"C": R.bgemm_blocks(A.shape[1], B.shape[2])})


@pytest.mark.parametrize("K", [1, 7, 17, 64, 100, 7936])
def test_bgemm_pieces(K):
    """K tails (K = 1, K no multiple of 16 or 32), ragged M and N on both tile forms, transposed / strided C, every epilogue,
    explicit splits (three with diag, one above the number of K slices so that one is empty)."""
    slices = -(-K // SLICE)
    for Mr, Nc in SHAPES:
        A, B, D = R.bgemm_case(2, Mr, Nc, K)
        C0 = (D * 0.5 + 1.0).float().double()
        t = f"{Mr}x{Nc}x{K}"
        _hold("bgemm", t + " plain->padded", A, B, None, C0, "plain", "plain", "padded", 0.5, 0.0, 0.0, 1)
        _hold("bgemm", t + " T,T->T beta D diag", A, B, D, C0, "T", "T", "T", -1.0, -7.0, 15.0, 1)
        _hold("bgemm", t + " D on padded C", A, B, D, C0, "plain", "T", "padded", 1.0, 0.5, 0.0, 1)
        _hold("bgemm", t + " beta in place ->T", A, B, None, C0, "T", "plain", "T", 2.0, 0.75, -3.0, 1)
        _hold("bgemm", t + " splits 3 diag", A, B, None, C0, "plain", "plain", "plain", 1.0, 1.0, 2.5, 3)
        _hold("bgemm", t + " splits slices+1", A, B, None, C0, "T", "T", "padded", -0.5, 1.0, 0.0, slices + 1)


@pytest.mark.parametrize("K", [1, 7, 17, 64, 100, 7936])
def test_bgemm_pieces_fixed(K):
    """The same cases with splits > 1 on the fixed-order entry, which takes any beta, D and diag with any splits: same
    bound, two calls bit-equal, nothing behind the workspace size of mil_tm_bgemm_ws_floats written."""
    slices = -(-K // SLICE)
    for Mr, Nc in SHAPES:
        A, B, D = R.bgemm_case(2, Mr, Nc, K)
        C0 = (D * 0.5 + 1.0).float().double()
        t = f"{Mr}x{Nc}x{K} fixed"
        _hold("bgemm_fixed", t + " plain->padded", A, B, None, C0, "plain", "plain", "padded", 0.5, 0.0, 0.0, 2, True)
        _hold("bgemm_fixed", t + " T,T->T beta D diag", A, B, D, C0, "T", "T", "T", -1.0, -7.0, 15.0, 3, True)
        _hold("bgemm_fixed", t + " D on padded C", A, B, D, C0, "plain", "T", "padded", 1.0, 0.5, 0.0, 2, True)
        _hold("bgemm_fixed", t + " beta in place ->T", A, B, None, C0, "T", "plain", "T", 2.0, 0.75, -3.0, 4, True)
        _hold("bgemm_fixed", t + " splits 3 diag", A, B, None, C0, "plain", "plain", "plain", 1.0, 1.0, 2.5, 3, True)
        _hold("bgemm_fixed", t + " splits slices+1", A, B, None, C0, "T", "T", "padded", -0.5, 1.0, 0.0, slices + 1, True)
    A, B, D = R.bgemm_case(2, 65, 63, K)                       # splits == 1 falls through to the plain entry: ws may be null
    abuf, bbuf = A.float().to(DEV), B.float().to(DEV)
    c = [torch.zeros((2, 65, 63), device=DEV) for _ in range(2)]
    sa, sb, sc = (65 * K, K, 1), (K * 63, 63, 1), (65 * 63, 63, 1)
    assert _lib().mil_tm_bgemm_pieces_fixed(_p(abuf), *sa, _p(bbuf), *sb, _p(c[0]), *sc, None, 2, 65, 63, K, 1.0, 0.0, 0.0, 1, 3,
                                            None, _st()) == 0
    assert _lib().mil_tm_bgemm_pieces(_p(abuf), *sa, _p(bbuf), *sb, _p(c[1]), *sc, None, 2, 65, 63, K, 1.0, 0.0, 0.0, 1, 3, _st()) == 0
    torch.cuda.synchronize()
    assert S._bits_equal(c[0], c[1])


@pytest.mark.parametrize("K", [1, 7, 17, 64])
def test_bgemm_pieces_reads_merged_qkv_rows(K):
    """A = q and B = k^T read in place from [n, 1536] rows (sAb = 64, sAi = 1536), as the logits' operands lie."""
    for Mr, Nc in SHAPES:
        A, B, D = R.bgemm_case(8, Mr, Nc, K, seed=1)
        _hold("bgemm", f"{Mr}x{Nc}x{K} merged q, k^T", A, B, None, D, "merged_rows", "merged_kT", "padded", 0.125, 0.0, 0.0, 1)


@pytest.mark.parametrize("K", [100, 7936])
def test_bgemm_pieces_writes_merged_head_rows(K):
    """B = v read from the merged rows, C written into merged-head [M, 512] rows (sCb = 64, sCi = 512), with and without
    split-K in both forms: the neighbouring heads' columns of a row are sentinel where batch < 8."""
    for Mr, Nc in ((65, 63), (64, 64), (257, 64)):
        for batch in (3, 8):
            A, B, D = R.bgemm_case(batch, Mr, Nc, K, seed=2)
            t = f"{batch}x{Mr}x{Nc}x{K} v->merged"
            _hold("bgemm", t, A, B, None, D, "plain", "merged_v", "merged_out", 1.0, 0.0, 0.0, 1)
            _hold("bgemm", t + " splits 4", A, B, None, D, "T", "merged_v", "merged_out", 1.0, 1.0, 0.0, 4)
            _hold("bgemm_fixed", t + " splits 4 fixed", A, B, None, D, "T", "merged_v", "merged_out", 1.0, 1.0, 0.0, 4, True)


def test_bgemm_pieces_einval_rules_launch_nothing():
    A, B, D = R.bgemm_case(2, 65, 63, 100)
    C0 = (D * 0.5 + 1.0).float().double()
    for fixed in (False, True):
        for pieces in (0, 1, 2, 4):                            # only three pieces are built
            for splits in (1, 3):
                _call(f"pieces {pieces}", A, B, None, C0, "plain", "plain", "padded", 1.0, 1.0, 0.0, splits, fixed, pieces, EINVAL)
    _call("splits 2 beta 0", A, B, None, C0, "plain", "plain", "padded", 1.0, 0.0, 0.0, 2, want_rc=EINVAL)    # split-K adds into C
    _call("splits 2 beta .5", A, B, None, C0, "plain", "plain", "padded", 1.0, 0.5, 0.0, 2, want_rc=EINVAL)
    _call("splits 2 with D", A, B, D, C0, "plain", "plain", "padded", 1.0, 1.0, 0.0, 2, want_rc=EINVAL)      # ... and D must be C
    _call("splits 0", A, B, None, C0, "plain", "plain", "padded", 1.0, 1.0, 0.0, 0, want_rc=EINVAL)
    _call("batch x splits", A, B, None, C0, "plain", "plain", "padded", 1.0, 1.0, 0.0, 32768, want_rc=EINVAL)
    ad, bd = A.float().to(DEV), B.float().to(DEV)
    c = torch.full((2, 65, 63), SENT, device=DEV)
    sa, sb, sc = (65 * 100, 100, 1), (100 * 63, 63, 1), (65 * 63, 63, 1)
    assert _lib().mil_tm_bgemm_pieces_fixed(_p(ad), *sa, _p(bd), *sb, _p(c), *sc, None, 2, 65, 63, 100, 1.0, 0.0, 0.0, 2, 3, None,
                                            _st()) == EINVAL                                                  # no workspace
    torch.cuda.synchronize()
    assert bool((c == SENT).all())


# --------------------------------------------------------------------------- the pseudo-inverse chain, 24 products deep
@pytest.mark.parametrize("det", [False, True])
def test_pinv_chain_on_pieces(det):
    """ops._tm_pinv_fwd's six iterations with pieces=3 on pinv_case()'s A2: the last Z per head against transmil_ref.pinv in
    float64, and _tm_pinv_bwd's dA2 against float64 autograd of the same; e32 from the float32 restatement on the CPU."""
    from mil_amd import ops
    a2, dZ = R.pinv_case()
    zr, gr = P.pinv_grad(a2, dZ)
    z32, g32 = P.pinv_grad(a2, dZ, torch.float32)
    ad = a2.float().to(DEV)
    with S_recorded() as log:
        Z, pinv = ops._tm_pinv_fwd(ad, det, 3)
        dA2 = ops._tm_pinv_bwd(dZ.float().to(DEV), ad, *pinv, det=det, pieces=3)
    torch.cuda.synchronize()
    names = [n for n, _ in log]
    assert names.count("mil_tm_bgemm_pieces") == 24 + 48 and "mil_tm_bgemm" not in names
    blocks = {"Z": P.head_blocks(), "dA2": P.head_blocks()}
    P.hold("pinv_chain", f"det {det}", {"Z": Z, "dA2": dA2}, {"Z": zr, "dA2": gr}, {"Z": z32, "dA2": g32}, blocks)


def S_recorded():
    import tm_fixed_ref as F
    return F.recorded()
