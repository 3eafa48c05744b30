"""GPU: mil_bag_softmax_rows (csrc/attn_pool.hip) through the C ABI on a segments.FusionBucket - the gated-attention pool's
softmax weights over a capacity bucket, bags scattered over [cap patch rows | B tail rows per segment], lengths on the device -
against the float64 per-bag softmax (tests/note_attn_bucket_ref.py, note_attn_ref.bag_softmax), per bag and per 256-row chunk
of a bag: max|got - ref| / max|ref| over a block <= 16 x max(e32, 1e-7), e32 being what the float32 restatement loses on the CPU
(the bar of tests/test_gpu_note_attn.py; measured ratios: docs/lab_notes.md).  The scores of the padding rows are NaN - they must
not be read - and the output carries a sentinel wherever the entry must not write."""
import ctypes

import pytest
import torch

import note_attn_bucket_ref as Q
import note_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -12345.678
SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
GUARD = 3


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def _bucket(cap, tail, lengths):
    from mil_amd.segments import FusionBucket
    bucket = FusionBucket(cap, len(lengths), DEV, P=tail[0], tail=tail)
    assert bucket.fits(lengths)
    return bucket.set_lengths(lengths)


def _launch(bucket, scores, buf, stream=None):
    from mil_amd import _lib
    lay = bucket.layout
    st = torch.cuda.current_stream() if stream is None else stream
    rc = _lib.lib().mil_bag_softmax_rows(_p(scores), _p(lay.tile_map), _p(lay.bag_tile_off), lay.T, _p(lay.row_bag()), lay.B, lay.R,
                                         _p(buf, GUARD), ctypes.c_void_p(st.cuda_stream))
    assert rc == 0


def _run(bucket, s):
    """refresh() + the entry on the float32 scores -> w [R] (a view between GUARD sentinels on either side, checked)."""
    R_ = bucket.layout.R
    buf = torch.full((R_ + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    bucket.refresh()
    _launch(bucket, s.float().to(DEV), buf)
    torch.cuda.synchronize()
    sent = lambda t: bool((t.contiguous().view(torch.int32) == SENT_BITS).all())      # noqa: E731
    assert sent(buf[:GUARD]) and sent(buf[GUARD + R_:]), "wrote outside w"
    return buf[GUARD:GUARD + R_]


def _hold(tag, got, s, rb, B):
    perm, off = Q.bag_order(rb, B)
    assert bool((got[(rb < 0).to(DEV)] == 0).all()), f"{tag}: the padding rows must read exactly 0"
    ref, r32 = Q.bag_softmax_rows(s, rb, B)[perm], Q.bag_softmax_rows(s.float(), rb, B)[perm]
    assert float((ref - R.bag_softmax(s[perm], off)).abs().max()) <= 1e-15        # the reference is the per-bag softmax
    g = got.double().cpu()[perm]
    R.hold("bag_softmax_rows", tag, g, ref, r32, R.softmax_blocks(off))
    sums = lambda w: torch.stack([w[off[b]:off[b + 1]].sum() for b in range(B)])      # noqa: E731
    R.hold("bag_softmax_rows.sums", tag, sums(g), sums(ref), sums(r32.double()), {f"bag{b}": (b,) for b in range(B)})


@pytest.mark.parametrize("kind", ["normal", "peak", "equal"])
@pytest.mark.parametrize("cap,tail,lengths", Q.CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_weights_against_float64(cap, tail, lengths, kind):
    B = len(lengths)
    bucket = _bucket(cap, tail, lengths)
    rb = Q.row_bag(cap, tail, lengths)
    s = Q.scores_for(kind, rb, B, 11)
    got = _run(bucket, s)
    assert torch.equal(bucket.row_bag_dev.cpu().long(), rb)                      # the host mirror is the device's map
    _hold(f"cap {cap} tail {tail} lengths {lengths} {kind}", got, s, rb, B)
    if kind == "peak":
        assert float(got.max()) > 0.9 and float(got[(rb >= 0).to(DEV)].median()) < 1e-9
    again = _run(bucket, s)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two launches differ in their bits"


def test_new_device_lengths_need_refresh_alone():
    """len_dev rewritten on the device and refresh(): the next launch gives the new bags' weights - nothing else comes from
    the host.  The stream argument is honoured: the launches go to a side stream and follow its order."""
    cap, tail = 512, [1, 4, 1]
    first, second = [130, 70, 200], [64, 257, 33]
    bucket = _bucket(cap, tail, first)
    assert bucket.fits(second)
    R_ = bucket.layout.R
    side = torch.cuda.Stream()
    for lengths in (first, second):
        rb = Q.row_bag(cap, tail, lengths)
        s = Q.scores_for("normal", rb, 3, 12)
        sd = s.float().to(DEV)
        buf = torch.full((R_ + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        bucket.len_dev.copy_(torch.tensor(lengths, dtype=torch.int32, device=DEV))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bucket.refresh()
            _launch(bucket, sd, buf, side)
        side.synchronize()
        _hold(f"device lengths {lengths}", buf[GUARD:GUARD + R_], s, rb, 3)


def test_ops_bag_softmax_takes_the_bucket_face():
    from mil_amd import ops
    cap, tail, lengths = Q.CASES[2]
    bucket = _bucket(cap, tail, lengths)
    bucket.refresh()
    rb = Q.row_bag(cap, tail, lengths)
    s = Q.scores_for("normal", rb, 3, 13)
    w = ops.bag_softmax(s.float().to(DEV).requires_grad_(True), bucket.layout)
    assert w.shape == (bucket.layout.R,) and not w.requires_grad
    _hold("ops.bag_softmax on the bucket", w, s, rb, 3)
    with pytest.raises(ValueError, match="rows"):
        ops.bag_softmax(torch.zeros(cap, device=DEV), bucket.layout)
