"""GPU: the two entries behind `model.note_attn` through the C ABI - mil_absorbed_pool_attn (csrc/absorbed_attn.hip), the
softmax weights of the absorbed one-token pool, and mil_bag_softmax (csrc/attn_pool.hip) - against the float64 restatement of
tests/note_attn_ref.py, per (bag, 64-key tile, head): max|got - ref| / max|ref| over a block <= 16 x max(e32, 1e-7), e32 being
what the float32 restatement loses on the CPU over the same block (the scheme of tests/test_gpu_attn_stages.py; measured
ratios: docs/lab_notes.md).  The kernel is fed the float32 rounding of the float64 forward's Qp and lse, as are both
restatements: one entry under test.  Outputs carry a sentinel wherever the entry must not write."""
import ctypes

import pytest
import torch

import note_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -12345.678
SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
EINVAL = -22
H, E = R.H, R.E
GUARD = 3                            # sentinel rows in front of and behind attn


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return t.float().to(DEV).contiguous()


def _is_sent(t):
    return bool((t.contiguous().view(torch.int32) == SENT_BITS).all())


def _segs(lens):
    from mil_amd.segments import AttnSegs
    return AttnSegs([1] * len(lens), lens, DEV)


def _run(keys, pe, Qp, lse, segs, ntiles, B, C, rows):
    """The entry on device tensors -> attn [rows, H] (a view between GUARD sentinel rows on either side, checked)."""
    buf = torch.full((rows + 2 * GUARD, H), SENT, dtype=torch.float32, device=DEV)
    rc = _lib().mil_absorbed_pool_attn(_p(keys), _p(pe), _p(Qp), _p(lse), _p(segs.k_off), _p(segs.tile_map), ntiles, B, H, C, E,
                                       _p(buf, GUARD * H), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert _is_sent(buf[:GUARD]) and _is_sent(buf[GUARD + rows:]), "wrote outside attn"
    return buf[GUARD:GUARD + rows]


def _check(tag, c, lse_from_gpu=False):
    C, off = c["C"], c["k_off"]
    lens = [off[b + 1] - off[b] for b in range(len(off) - 1)]
    s = _segs(lens)
    Qp, lse = R.fed(c)
    keys, pe, Qd = _dev(c["keys"]), _dev(c["pe"]), _dev(Qp)
    if lse_from_gpu:                                     # the GPU forward's own normaliser
        pooled, lg = torch.empty_like(Qd), torch.empty((len(lens), H), device=DEV)
        ws = torch.empty(s.ntiles * H * (E + 2), device=DEV)
        assert _lib().mil_absorbed_pool_fwd(_p(keys), _p(pe), _p(Qd), _p(s.k_off), _p(s.tile_map), _p(s.bag_tile_off), s.ntiles,
                                            len(lens), H, C, E, _p(pooled), _p(lg), _p(ws), _st()) == 0
        torch.cuda.synchronize()
        lse, ld = lg.double().cpu(), lg
    else:
        ld = _dev(lse)
    got = _run(keys, pe, Qd, ld, s, s.ntiles, len(lens), C, off[-1])
    ref = R.absorbed_attention(c["keys"], c["pe"], Qp, lse, off, C)
    r32 = R.absorbed_attention(c["keys"].float(), c["pe"].float(), Qp.float(), lse.float(), off, C)
    R.hold("absorbed_attn", tag, got, ref, r32, R.attn_blocks(off))
    R.hold("absorbed_attn.sums", tag, R.head_sums(got.double().cpu(), off), R.head_sums(ref, off), R.head_sums(r32, off),
           R.sum_blocks(len(lens)))
    return got


@pytest.mark.parametrize("C", [32, 64])
def test_ragged_bags(C):
    """A one-key bag, a partial, an exact and a just-over 64-key tile, two tiles and a bit, in one call."""
    _check(f"ragged C {C}", R.absorbed_case([1, 63, 64, 65, 130], C))


def test_single_bag():
    _check("single 200", R.absorbed_case([200], 32, seed=1))


@pytest.mark.parametrize("C", [32, 64])
def test_peaked(C):
    """One key per bag scores about 30 above the rest: the other weights underflow towards 0, relative to the peak."""
    c = R.peak(R.absorbed_case([65, 130, 200], C, seed=2))
    got = _check(f"peaked C {C}", c)
    assert float(got.max()) > 0.9 and float(got.median()) < 1e-9


@pytest.mark.parametrize("C", [32, 64])
def test_with_the_gpu_forwards_lse(C):
    _check(f"gpu lse C {C}", R.absorbed_case([1, 63, 64, 65, 130], C, seed=3), lse_from_gpu=True)


def test_rejections_launch_nothing():
    c = R.absorbed_case([70], 32)
    s = _segs([70])
    Qp, lse = R.fed(c)
    keys, pe, Qd, ld = _dev(c["keys"]), _dev(c["pe"]), _dev(Qp), _dev(lse)
    out = torch.full((70, H), SENT, dtype=torch.float32, device=DEV)
    for Hh, C, Ee in ((8, 48, 512), (4, 32, 512), (8, 32, 256), (8, 16, 512)):
        assert _lib().mil_absorbed_pool_attn(_p(keys), _p(pe), _p(Qd), _p(ld), _p(s.k_off), _p(s.tile_map), s.ntiles, 1, Hh, C, Ee,
                                             _p(out), _st()) == EINVAL
    assert _lib().mil_absorbed_pool_attn(_p(keys), _p(pe), _p(Qd), None, _p(s.k_off), _p(s.tile_map), s.ntiles, 1, 8, 32, 512,
                                         _p(out), _st()) == EINVAL
    torch.cuda.synchronize()
    assert _is_sent(out)


# --------------------------------------------------------------------------- capacity bucket, device lengths, one graph
CAP = 256                            # two slots of 128 rows


def _bucket_inputs(lens, seed):
    c = R.absorbed_case(lens, 32, seed=seed)
    Qp, lse = R.fed(c)
    keys = torch.full((CAP, E), float("nan"), dtype=torch.float64)          # rows behind the bags are never read
    keys[:sum(lens)] = c["keys"]
    pe = torch.zeros((CAP, E), dtype=torch.float64)
    pe[:c["pe"].shape[0]] = c["pe"]
    ref = R.absorbed_attention(c["keys"], c["pe"], Qp, lse, c["k_off"], 32)
    r32 = R.absorbed_attention(c["keys"].float(), c["pe"].float(), Qp.float(), lse.float(), c["k_off"], 32)
    return c, dict(keys=_dev(keys), pe=_dev(pe), Qp=_dev(Qp), lse=_dev(lse)), ref, r32


def test_bucket_with_device_lengths_and_its_graph():
    """segments.FusionBucket (the tile map built on the device from len_dev, padding tiles behind the bags): rows behind the
    bags read exactly 0, nothing is written outside attn, and the same call captured into one graph (one stream) follows the
    device lengths when they change."""
    from mil_amd.bags import upload_lengths
    from mil_amd.segments import FusionBucket
    bucket = FusionBucket(CAP, 2, DEV)
    first, second = [65, 1], [1, 65]
    c1, d1, ref1, r321 = _bucket_inputs(first, 4)
    c2, d2, ref2, r322 = _bucket_inputs(second, 5)
    static = {n: t.clone() for n, t in d1.items()}
    buf = torch.full((CAP + 2 * GUARD, H), SENT, dtype=torch.float32, device=DEV)
    s = bucket.s_ti

    def call():
        bucket.refresh()
        assert _lib().mil_absorbed_pool_attn(_p(static["keys"]), _p(static["pe"]), _p(static["Qp"]), _p(static["lse"]), _p(s.k_off),
                                             _p(s.tile_map), s.ntiles, 2, H, 32, E, _p(buf, GUARD * H), _st()) == 0

    def verify(tag, lens, c, ref, r32):
        torch.cuda.synchronize()
        n = sum(lens)
        assert _is_sent(buf[:GUARD]) and _is_sent(buf[GUARD + CAP:]), tag
        got = buf[GUARD:GUARD + CAP]
        assert bool((got[n:] == 0).all()), f"{tag}: rows behind the bags must read 0"
        R.hold("absorbed_attn", tag, got[:n], ref, r32, R.attn_blocks(c["k_off"]))

    upload_lengths(bucket.len_dev, first)
    call()
    verify("bucket eager [65, 1]", first, c1, ref1, r321)
    buf.fill_(SENT)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    graph.replay()
    verify("bucket replay [65, 1]", first, c1, ref1, r321)
    buf.fill_(SENT)
    upload_lengths(bucket.len_dev, second)
    for n, t in d2.items():
        static[n].copy_(t)
    graph.replay()
    verify("bucket replay [1, 65]", second, c2, ref2, r322)


# --------------------------------------------------------------------------- mil_bag_softmax
SM_LENS = [1, 2, 1023, 1024, 1025]


@pytest.mark.parametrize("with_len", [False, True])
def test_bag_softmax(with_len):
    off = R.offsets(SM_LENS)
    true = [1, 1, 1000, 1024, 513] if with_len else None
    s = (3.0 * torch.randn(off[-1], generator=torch.Generator().manual_seed(7), dtype=torch.float64)).float().double()
    sd = _dev(s)
    buf = torch.full((off[-1] + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    row_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    len_dev = torch.tensor(true, dtype=torch.int32, device=DEV) if with_len else None
    assert _lib().mil_bag_softmax(_p(sd), _p(row_off), _p(len_dev), len(SM_LENS), _p(buf, GUARD), _st()) == 0
    torch.cuda.synchronize()
    assert _is_sent(buf[:GUARD]) and _is_sent(buf[GUARD + off[-1]:])
    got = buf[GUARD:GUARD + off[-1]]
    ref, r32 = R.bag_softmax(s, off, true), R.bag_softmax(s.float(), off, true)
    if with_len:
        for b, n in enumerate(true):
            assert bool((got[off[b] + n:off[b + 1]] == 0).all()), f"bag {b}: rows behind the device length must read 0"
    R.hold("bag_softmax", f"len_dev {with_len}", got, ref, r32, R.softmax_blocks(off))
    sums = lambda w: torch.stack([w[off[b]:off[b + 1]].sum() for b in range(len(SM_LENS))])      # noqa: E731
    R.hold("bag_softmax.sums", f"len_dev {with_len}", sums(got.double().cpu()), sums(ref), sums(r32),
           {f"bag{b}": (b,) for b in range(len(SM_LENS))})


def test_ops_reject_cpu_tensors_and_take_no_gradient():
    from mil_amd import _lib as L, ops
    from mil_amd.bags import BagLayout
    c = R.absorbed_case([70], 32)
    Qp, lse = R.fed(c)
    s = _segs([70])
    with pytest.raises(L.MilHipError):
        ops.absorbed_pool_attention(c["keys"].float(), _dev(c["pe"]), _dev(Qp), _dev(lse), s, 32)
    with pytest.raises(L.MilHipError):
        ops.bag_softmax(torch.zeros(70), BagLayout.make([70], DEV))
    keys = _dev(c["keys"]).requires_grad_(True)
    a = ops.absorbed_pool_attention(keys, _dev(c["pe"]), _dev(Qp), _dev(lse), s, 32)
    w = ops.bag_softmax(torch.zeros(70, device=DEV, requires_grad=True), BagLayout.make([70], DEV))
    assert not a.requires_grad and not w.requires_grad and a.shape == (70, H)
    assert float((w - 1 / 70).abs().max()) < 1e-8
