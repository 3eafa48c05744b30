"""GPU: every C entry of the fusion model's attention kernels (csrc/attention.hip: rows, general backward, pool, seq;
csrc/absorbed_attn.hip: the one-token absorbed path) on its own against the float64 restatement of tests/attn_ref.py, per
block: max|got - ref| / max|ref| over a block <= k x max(e32, 1e-7), e32 being what the float32 restatement loses on the CPU
over the same block.  tests/test_attn_sensitivity_host.py shows what these bounds see; the k of each stage
(attn_ref.K_STAGE) comes from the measured ratios in docs/lab_notes.md.  Every backward is fed the float32 rounding of the
float64 forward (o, lse; on the absorbed path every intermediate), as is the float32 restatement: one entry under test at a
time.  Buffers carry a sentinel wherever an entry must not write - guard rows behind the last bag, the tail of every
workspace past its documented size, the gap columns of strided outputs - compared bit for bit afterwards."""
import ctypes
import math

import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -12345.678                    # the sentinel; the bit pattern is what is compared
SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
EINVAL = -22
H, E = A.H, A.E
GUARD, TAIL = 3, 64                  # guard rows behind an output, sentinel floats behind a workspace


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV).contiguous()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=DEV)


def _is_sent(t):
    return bool((t.contiguous().view(torch.int32) == SENT_BITS).all())


def _segs(c):
    from mil_amd.segments import AttnSegs
    q, k = c["q_off"], c["k_off"]
    return AttnSegs([q[i + 1] - q[i] for i in range(len(q) - 1)], [k[i + 1] - k[i] for i in range(len(k) - 1)], DEV)


def _fed(ref_f):
    """The float32 rounding of the float64 forward, as the backward entries take it."""
    return _dev(ref_f["o"]), _dev(ref_f["lse"])


def _noise(stage, tag, c, got, causal=False):
    """The blocks that are zero by cancellation (attn_ref.bwd_blocks): rounding noise of the two terms, no more."""
    for name, rel in A.cancel_noise(c, got, causal).items():
        print(f"NOISE | {stage} | {tag} | {name} | {rel:.2e} of the cancelling terms | bound {A.noise_bound(c['C']):.2e}")
        assert rel <= A.noise_bound(c["C"]), (stage, tag, name, rel)


# --------------------------------------------------------------------------- rows form
def _rows_fwd(c, causal):
    C, I, Tq = c["C"], H * c["C"], c["q_off"][-1]
    s = _segs(c)
    o, lse = _sent(Tq + GUARD, I), _sent(Tq + GUARD, H)
    q, k, v = (_dev(c[n]) for n in "qkv")                   # held until the synchronize: a temporary's memory is reused
    rc = _lib().mil_attn_rows_fwd(_p(q), _p(k), _p(v), _p(s.q_off), _p(s.k_off), _p(s.q_bag),
                                  Tq, H, C, int(causal), _p(o), _p(lse), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert _is_sent(o[Tq:]) and _is_sent(lse[Tq:]), "rows forward wrote behind its rows"
    return {"o": o[:Tq], "lse": lse[:Tq]}


@pytest.mark.parametrize("C", [32, 64])
def test_rows_fwd(C):
    """(query rows, keys) = (1, 1) .. (70, 10), a bag without rows, a bag without keys: o = 0 and lse = -inf there."""
    c = A.attn_case(A.ROWS_BAGS, C)
    assert (c["q_off"][-1] * H) % 256 != 0
    got = _rows_fwd(c, False)
    rows = slice(c["q_off"][6], c["q_off"][7])
    assert bool((got["o"][rows] == 0).all()) and bool((got["lse"][rows] == -math.inf).all())
    A.hold("rows_fwd", f"C {C}", got, A.fwd_run(c), A.fwd_run(c, torch.float32), A.fwd_blocks(c))


@pytest.mark.parametrize("C", [32, 64])
def test_rows_fwd_causal(C):
    c = A.attn_case([(n, n) for n in A.CAUSAL_LENS], C, seed=1)
    got = _rows_fwd(c, True)
    A.hold("rows_fwd", f"causal C {C}", got, A.fwd_run(c, causal=True), A.fwd_run(c, torch.float32, causal=True), A.fwd_blocks(c))


@pytest.mark.parametrize("C", [32, 64])
def test_rows_bwd(C):
    """2, 15, 16 keys, partial 32-row blocks, a bag with keys and no rows (dk = dv = 0), the one-key bag (dq = dk = 0): the
    zeros exact, since block_err meets an all-zero reference exactly."""
    c = A.attn_case(A.ROWS_BWD_BAGS, C)
    I, Tq, Tk = H * C, c["q_off"][-1], c["k_off"][-1]
    assert (Tq * H) % 256 != 0
    s = _segs(c)
    ref_f = A.fwd_run(c)
    o, lse = _fed(ref_f)
    dq, dk, dv = _sent(Tq + GUARD, I), _sent(Tk + GUARD, I), _sent(Tk + GUARD, I)
    ws = _sent(s.nblk * 2 * 16 * I + TAIL)
    q, k, v, dO = (_dev(c[n]) for n in ("q", "k", "v", "dO"))
    rc = _lib().mil_attn_rows_bwd(_p(q), _p(k), _p(v), _p(o), _p(dO), _p(lse),
                                  _p(s.k_off), _p(s.blk_map), _p(s.bag_blk_off), s.nblk, s.B, H, C, _p(dq), _p(dk), _p(dv),
                                  _p(ws), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert _is_sent(dq[Tq:]) and _is_sent(dk[Tk:]) and _is_sent(dv[Tk:]) and _is_sent(ws[-TAIL:])
    got = {"dq": dq[:Tq], "dk": dk[:Tk], "dv": dv[:Tk]}
    A.hold("rows_bwd", f"C {C}", got, A.bwd_run(c), A.bwd_run(c, torch.float32, fwd=ref_f), A.bwd_blocks(c, exact=True))


# --------------------------------------------------------------------------- general backward
@pytest.mark.parametrize("C", [32, 64])
def test_rows_bwd_general(C):
    c = A.attn_case(A.GEN_BAGS, C)
    I, Tq, Tk = H * C, c["q_off"][-1], c["k_off"][-1]
    s = _segs(c)
    ref_f = A.fwd_run(c)
    o, lse = _fed(ref_f)
    dq, dk, dv = _sent(Tq + GUARD, I), _sent(Tk + GUARD, I), _sent(Tk + GUARD, I)
    ws = _sent(Tq * H + TAIL)
    q, k, v, dO = (_dev(c[n]) for n in ("q", "k", "v", "dO"))
    rc = _lib().mil_attn_rows_bwd_general(_p(q), _p(k), _p(v), _p(o), _p(dO), _p(lse),
                                          _p(s.q_off), _p(s.k_off), _p(s.q_bag), _p(s.k_bag), Tq, Tk, H, C, _p(dq), _p(dk),
                                          _p(dv), _p(ws), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert _is_sent(dq[Tq:]) and _is_sent(dk[Tk:]) and _is_sent(dv[Tk:]) and _is_sent(ws[-TAIL:])
    got = {"dq": dq[:Tq], "dk": dk[:Tk], "dv": dv[:Tk]}
    A.hold("gen_bwd", f"C {C}", got, A.bwd_run(c), A.bwd_run(c, torch.float32, fwd=ref_f), A.bwd_blocks(c))
    _noise("gen_bwd", f"C {C}", c, got)


# --------------------------------------------------------------------------- pool form
def _pool(tag, c, Tmax, tiles=None, k_src=None, v_src=None):
    """Forward, then the backward on the rounded float64 forward.  tiles: (tile_map rows, bag_tile_off) instead of the
    AttnSegs ones; k_src / v_src: device tensors to read k, v from.  Returns (fwd, bwd, forward workspace)."""
    C, I, Tq, Tk = c["C"], H * c["C"], c["q_off"][-1], c["k_off"][-1]
    s = _segs(c)
    tm, toff = (s.tile_map, s.bag_tile_off) if tiles is None else (_i32(tiles[0]), _i32(tiles[1]))
    nt = int(tm.shape[0])
    q, dO = _dev(c["q"]), _dev(c["dO"])
    k = _dev(c["k"]) if k_src is None else k_src
    v = _dev(c["v"]) if v_src is None else v_src
    o, lse = _sent(Tq + GUARD, I), _sent(Tq + GUARD, H)
    wf = _sent(nt * 16 * (I + 2 * H) + TAIL)
    rc = _lib().mil_attn_pool_fwd_mh(_p(q), _p(k), _p(v), _p(s.q_off), _p(tm), _p(toff), nt, s.B, Tmax, H, C, _p(o), _p(lse),
                                     _p(wf), _st())
    assert rc == 0, tag
    ref_f = A.fwd_run(c)
    of, lf = _fed(ref_f)
    dq, dk, dv = _sent(Tq + GUARD, I), _sent(Tk + GUARD, I), _sent(Tk + GUARD, I)
    wb = _sent(nt * 16 * I + TAIL)
    rc = _lib().mil_attn_pool_bwd_mh(_p(q), _p(k), _p(v), _p(of), _p(dO), _p(lf), _p(s.q_off), _p(tm), _p(toff), nt, s.B, Tmax,
                                     H, C, _p(dq), _p(dk), _p(dv), _p(wb), _st())
    assert rc == 0, tag
    torch.cuda.synchronize()
    assert _is_sent(o[Tq:]) and _is_sent(lse[Tq:]) and _is_sent(wf[-TAIL:]), f"{tag}: forward wrote outside"
    assert _is_sent(dq[Tq:]) and _is_sent(dk[Tk:]) and _is_sent(dv[Tk:]) and _is_sent(wb[-TAIL:]), f"{tag}: backward wrote outside"
    fwd, bwd = {"o": o[:Tq], "lse": lse[:Tq]}, {"dq": dq[:Tq], "dk": dk[:Tk], "dv": dv[:Tk]}
    A.hold("pool_fwd", tag, fwd, ref_f, A.fwd_run(c, torch.float32), A.fwd_blocks(c))
    A.hold("pool_bwd", tag, bwd, A.bwd_run(c), A.bwd_run(c, torch.float32, fwd=ref_f), A.bwd_blocks(c))
    _noise("pool_bwd", tag, c, bwd)
    return fwd, bwd, wf


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("name", ["ragged", "single", "peaked"])
def test_pool(name, C):
    """ragged: T in 1 .. 16 per bag over 1, 3, 63, 64, 65, 130, 200 keys; single: one bag (10, 200); peaked: scores near
    +-80 with the largest in another tile per head (the merge across tiles)."""
    bags = {"ragged": A.POOL_RAGGED, "single": A.POOL_SINGLE, "peaked": A.POOL_PEAKED}[name]
    _pool(f"{name} C {C}", A.attn_case(bags, C, peaked=name == "peaked"), max(t for t, _ in bags))


@pytest.mark.parametrize("C", [32, 64])
def test_pool_zero_key_tiles(C):
    """A tile of no keys - {bag, 0, 0}, what a capacity bucket pads its tile map with - in front of a bag's tiles, and one
    behind every bag's range: its partial is (m = -inf, l = 0, acc = 0) and the merge takes nothing from it.  k and v start
    one row into an allocation whose first row is NaN: the clamped row index of such a tile must not go below key0.  The
    second bag has queries and no tile at all: o = 0, lse = -inf, dq = 0."""
    c = A.attn_case([(3, 70), (2, 0)], C, seed=3)
    I = H * C
    nan_row = torch.full((1, I), math.nan, dtype=torch.float64)
    kb, vb = _dev(torch.cat([nan_row, c["k"]])), _dev(torch.cat([nan_row, c["v"]]))
    tiles = ([[0, 0, 0], [0, 0, 64], [0, 64, 6], [0, 0, 0]], [0, 3, 3])
    fwd, bwd, wf = _pool(f"zero-key tiles C {C}", c, 3, tiles, kb[1:], vb[1:])
    assert all(bool(torch.isfinite(t[:3]).all()) for t in (fwd["o"], fwd["lse"], bwd["dq"])) and bool(torch.isfinite(bwd["dk"]).all())
    assert bool((fwd["o"][3:] == 0).all()) and bool((fwd["lse"][3:] == -math.inf).all()) and bool((bwd["dq"][3:] == 0).all())
    pacc = wf[:4 * 16 * I].reshape(4, 16, I)
    pml = wf[4 * 16 * I:4 * 16 * (I + 2 * H)].reshape(4, 16, H, 2)
    for g in (0, 3):
        assert bool((pacc[g, :3] == 0).all()) and bool((pml[g, :3, :, 0] == -math.inf).all()) and bool((pml[g, :3, :, 1] == 0).all())


def test_pool_rejections_launch_nothing():
    c = A.attn_case(A.POOL_SINGLE, 32)
    s = _segs(c)
    Tq, Tk = c["q_off"][-1], c["k_off"][-1]
    q, k, v, dO = (_dev(c[n]) for n in ("q", "k", "v", "dO"))
    outs = [_sent(Tq, 512), _sent(Tq, H), _sent(Tq, 512), _sent(Tk, 512), _sent(Tk, 512), _sent(s.ntiles * 16 * (512 + 2 * H))]
    o, lse, dq, dk, dv, ws = outs
    for Tmax, C in ((17, 32), (10, 48), (0, 32)):
        assert _lib().mil_attn_pool_fwd_mh(_p(q), _p(k), _p(v), _p(s.q_off), _p(s.tile_map), _p(s.bag_tile_off), s.ntiles, 1, Tmax,
                                           H, C, _p(o), _p(lse), _p(ws), _st()) == EINVAL
        assert _lib().mil_attn_pool_bwd_mh(_p(q), _p(k), _p(v), _p(o), _p(dO), _p(lse), _p(s.q_off), _p(s.tile_map),
                                           _p(s.bag_tile_off), s.ntiles, 1, Tmax, H, C, _p(dq), _p(dk), _p(dv), _p(ws), _st()) == EINVAL
    torch.cuda.synchronize()
    assert all(_is_sent(t) for t in outs)


# --------------------------------------------------------------------------- seq form
def _seq_buffers(c, layout):
    """(q, k, v pointers, ld, [dq, dk, dv views], ldd, whole output buffers) for one layout; input gaps hold NaN."""
    I, T = H * c["C"], c["q_off"][-1]
    if layout == "packed":                                   # q | k | v the column blocks of one [T, 3 I] buffer
        src = _dev(torch.cat([c["q"], c["k"], c["v"]], 1))
        dst = _sent(T + GUARD, 3 * I)
        return [_p(src, I * i) for i in range(3)], 3 * I, [dst[:, I * i:I * (i + 1)] for i in range(3)], 3 * I, [dst], [src]
    ld = I + (4 if layout == "gapped" else 0)
    srcs, dsts = [], []
    for n in ("q", "k", "v"):
        t = torch.full((T, ld), math.nan, dtype=torch.float32)
        t[:, :I] = c[n].float()
        srcs.append(t.to(DEV))
        dsts.append(_sent(T + GUARD, ld))
    return [_p(t) for t in srcs], ld, [t[:, :I] for t in dsts], ld, dsts, srcs


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("layout", ["dense", "packed", "gapped"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_seq(causal, layout, C):
    """Lengths 1 .. 96 in one call.  dense: ld = ldd = H C; packed: ld = ldd = 3 H C; gapped: ld = ldd = H C + 4, the input
    gaps NaN, the gaps of dq, dk, dv sentinel afterwards."""
    c = A.seq_case(A.SEQ_LENS, C)
    I, T, B = H * C, c["q_off"][-1], len(A.SEQ_LENS)
    tag = f"{'causal' if causal else 'full'} {layout} C {C}"
    qoff = _i32(c["q_off"])
    ptr, ld, views, ldd, dsts, keep = _seq_buffers(c, layout)
    o, lse = _sent(T + GUARD, I), _sent(T + GUARD, H)
    rc = _lib().mil_attn_seq_fwd(*ptr, ld, _p(qoff), B, max(A.SEQ_LENS), H, C, int(causal), _p(o), _p(lse), _st())
    assert rc == 0
    ref_f = A.fwd_run(c, causal=causal)
    of, lf = _fed(ref_f)
    dptr = [_p(dsts[0], I * i) for i in range(3)] if layout == "packed" else [_p(t) for t in dsts]
    dO = _dev(c["dO"])
    rc = _lib().mil_attn_seq_bwd(*ptr, ld, _p(of), _p(dO), _p(lf), _p(qoff), B, max(A.SEQ_LENS), H, C, int(causal),
                                 *dptr, ldd, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert _is_sent(o[T:]) and _is_sent(lse[T:]), f"{tag}: forward wrote behind its rows"
    for t in dsts:
        assert _is_sent(t[T:]), f"{tag}: backward wrote behind its rows"
        if layout == "gapped":
            assert _is_sent(t[:, I:]), f"{tag}: backward wrote into the gap columns"
    fwd = {"o": o[:T], "lse": lse[:T]}
    bwd = {n: v[:T].contiguous() for n, v in zip(("dq", "dk", "dv"), views)}
    A.hold("seq_fwd", tag, fwd, ref_f, A.fwd_run(c, torch.float32, causal=causal), A.fwd_blocks(c))
    A.hold("seq_bwd", tag, bwd, A.bwd_run(c, causal=causal), A.bwd_run(c, torch.float32, causal=causal, fwd=ref_f),
           A.bwd_blocks(c, causal))
    _noise("seq_bwd", tag, c, bwd, causal)


def test_seq_rejections_launch_nothing():
    c = A.seq_case([5, 9], 32)
    I, T = 256, 14
    q, k, v, dO = (_dev(c[n]) for n in ("q", "k", "v", "dO"))
    qoff = _i32(c["q_off"])
    outs = [_sent(T, I) for _ in range(4)] + [_sent(T, H)]
    o, dq, dk, dv, lse = outs
    for Tmax, ld, ldd in ((97, I, I), (9, I - 4, I), (9, I + 2, I + 4), (9, I, I - 4)):
        if ldd == I or ld != I:
            assert _lib().mil_attn_seq_fwd(_p(q), _p(k), _p(v), ld, _p(qoff), 2, Tmax, H, 32, 0, _p(o), _p(lse), _st()) == EINVAL
        assert _lib().mil_attn_seq_bwd(_p(q), _p(k), _p(v), ld, _p(o), _p(dO), _p(lse), _p(qoff), 2, Tmax, H, 32, 0, _p(dq),
                                       _p(dk), _p(dv), ldd, _st()) == EINVAL
    torch.cuda.synchronize()
    assert all(_is_sent(t) for t in outs)


# --------------------------------------------------------------------------- the one-token absorbed path
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("lens", [A.ABS_BAGS, A.ABS_SINGLE], ids=["ragged", "single"])
def test_absorbed_path(lens, C):
    """mil_absorb_query (+ _bwd: both halves, each alone), mil_absorbed_pool_fwd, mil_absorbed_pool_value_fwd (its pooled, lse
    and o by the same bound; bit identity with the plain forward: the last test), mil_value_proj (+ _bwd with and without dbv), mil_absorbed_pool_bwd with and
    without dkeys_acc - each on the rounded float64 intermediates.  pe is a table longer than the longest bag."""
    from mil_amd.segments import AttnSegs
    L = _lib()
    c = A.absorbed_case(lens, C)
    B, N, I = len(lens), sum(lens), H * C
    tag = f"{B} bags C {C}"
    ref, blocks = A.absorbed_ref(c), A.absorbed_blocks(c)
    r32 = A.absorbed(c, torch.float32, given=ref)
    s = AttnSegs([1] * B, lens, DEV)
    nt = s.ntiles
    d = {n: _dev(c[n]) for n in ("keys", "pe", "qp", "Wk", "Wv", "bv", "dO", "dkeys_acc")}
    fed = {n: _dev(ref[n]) for n in ("Qp", "pooled", "lse", "dpooled", "dQp")}
    geo = (_p(s.k_off), _p(s.tile_map), _p(s.bag_tile_off), nt)

    # absorb_query and its backward
    Qp = _sent(B * H * E + TAIL)
    assert L.mil_absorb_query(_p(d["qp"]), _p(d["Wk"]), B, H, C, E, _p(Qp), _st()) == 0
    dqp, dWk, dqp1, dWk1 = _sent(B + 1, I), _sent(I + 1, E), _sent(B + 1, I), _sent(I + 1, E)
    assert L.mil_absorb_query_bwd(_p(d["qp"]), _p(d["Wk"]), _p(fed["dQp"]), B, H, C, E, _p(dqp), _p(dWk), _st()) == 0
    assert L.mil_absorb_query_bwd(_p(d["qp"]), _p(d["Wk"]), _p(fed["dQp"]), B, H, C, E, _p(dqp1), None, _st()) == 0
    assert L.mil_absorb_query_bwd(_p(d["qp"]), _p(d["Wk"]), _p(fed["dQp"]), B, H, C, E, None, _p(dWk1), _st()) == 0
    # the pool's forward, plain and with the value projection in its merge launch
    pooled, lse, wf = _sent(B + 1, H, E), _sent(B * H + 8), _sent(nt * H * (E + 2) + TAIL)
    assert L.mil_absorbed_pool_fwd(_p(d["keys"]), _p(d["pe"]), _p(fed["Qp"]), *geo, B, H, C, E, _p(pooled), _p(lse), _p(wf), _st()) == 0
    pooled2, lse2, o2, wf2 = _sent(B + 1, H, E), _sent(B * H + 8), _sent(B + 1, I), _sent(nt * H * (E + 2) + TAIL)
    assert L.mil_absorbed_pool_value_fwd(_p(d["keys"]), _p(d["pe"]), _p(fed["Qp"]), *geo, B, H, C, E, _p(d["Wv"]), _p(d["bv"]),
                                         _p(pooled2), _p(lse2), _p(o2), _p(wf2), _st()) == 0
    # value projection and its backward
    o = _sent(B + 1, I)
    assert L.mil_value_proj(_p(fed["pooled"]), _p(d["Wv"]), _p(d["bv"]), B, H, C, E, _p(o), _st()) == 0
    dpooled, dWv, dbv, dpooled1, dWv1 = _sent(B + 1, H, E), _sent(I + 1, E), _sent(I + 8), _sent(B + 1, H, E), _sent(I + 1, E)
    assert L.mil_value_proj_bwd(_p(d["dO"]), _p(d["Wv"]), _p(fed["pooled"]), B, H, C, E, _p(dpooled), _p(dWv), _p(dbv), _st()) == 0
    assert L.mil_value_proj_bwd(_p(d["dO"]), _p(d["Wv"]), _p(fed["pooled"]), B, H, C, E, _p(dpooled1), _p(dWv1), None, _st()) == 0
    # the pool's backward, with and without the addend
    bwd = {}
    for acc in (True, False):
        dkeys, dQp, wb = _sent(N + GUARD, E), _sent(B + 1, H, E), _sent(nt * H * E + 16 * N + TAIL)
        assert L.mil_absorbed_pool_bwd(_p(d["keys"]), _p(d["pe"]), _p(fed["Qp"]), _p(fed["lse"]), _p(fed["dpooled"]),
                                       _p(fed["pooled"]), *geo, N, B, H, C, E, _p(d["dkeys_acc"]) if acc else None, _p(dkeys),
                                       _p(dQp), _p(wb), _st()) == 0
        bwd[acc] = (dkeys, dQp, wb)
    torch.cuda.synchronize()

    assert _is_sent(Qp[-TAIL:]) and all(_is_sent(t[B:]) for t in (dqp, dqp1, pooled, pooled2, o, o2, dpooled, dpooled1))
    assert all(_is_sent(t[I:]) for t in (dWk, dWk1, dWv, dWv1, dbv)) and _is_sent(lse[B * H:]) and _is_sent(lse2[B * H:])
    assert _is_sent(wf[-TAIL:]) and _is_sent(wf2[-TAIL:])
    for dkeys, dQp, wb in bwd.values():
        assert _is_sent(dkeys[N:]) and _is_sent(dQp[B:]) and _is_sent(wb[-TAIL:]), "pool backward wrote outside"

    def hold(stage, what, got):
        A.hold(stage, f"{tag} {what}", got, ref, r32, blocks)
    hold("absorb", "query", {"Qp": Qp[:-TAIL].reshape(B, H, E)})
    hold("absorb", "query_bwd both", {"dqp": dqp[:B], "dWk": dWk[:I]})
    hold("absorb", "query_bwd alone", {"dqp": dqp1[:B], "dWk": dWk1[:I]})
    hold("absorbed_pool", "fwd", {"pooled": pooled[:B], "lse": lse[:B * H].reshape(B, H)})
    hold("absorbed_pool", "fwd, value in merge", {"pooled": pooled2[:B], "lse": lse2[:B * H].reshape(B, H), "o": o2[:B]})
    hold("absorb", "value_proj", {"o": o[:B]})
    hold("absorb", "value_proj_bwd", {"dpooled": dpooled[:B], "dWv": dWv[:I], "dbv": dbv[:I]})
    hold("absorb", "value_proj_bwd no dbv", {"dpooled": dpooled1[:B], "dWv": dWv1[:I]})
    hold("absorbed_pool", "bwd acc", {"dkeys": bwd[True][0][:N], "dQp": bwd[True][1][:B]})
    ref_noacc = dict(ref, dkeys=A.absorbed_ref(c, acc=False)["dkeys"])
    r32_noacc = A.absorbed(c, torch.float32, given=ref, acc=False)
    A.hold("absorbed_pool", f"{tag} bwd no acc", {"dkeys": bwd[False][0][:N], "dQp": bwd[False][1][:B]}, ref_noacc, r32_noacc, blocks)
    # the one-key bag: dQp is the rounding noise of two equal dot products, and dqp of the (near-)zero dQp fed in is bounded
    # by E max|Wk| max|dQp|
    for acc in (True, False):
        for b, rel in A.onekey_noise(c, ref, {"dQp": bwd[acc][1][:B]}).items():
            print(f"NOISE | absorbed_pool | {tag} | dQp.bag{b} | {rel:.2e} of the cancelling terms")
            assert rel <= A.NOISE_K * 2.0 ** -23 * math.sqrt(E)
    for b in [i for i, n in enumerate(lens) if n == 1]:
        top = E * float(c["Wk"].abs().max()) * float(fed["dQp"][b].abs().max())
        assert float(dqp[b].abs().max()) <= top and float(dqp1[b].abs().max()) <= top


@pytest.mark.parametrize("C", [32, 64])
def test_absorbed_value_fwd_bitwise_equals_plain_forward(C):
    """pooled and lse of mil_absorbed_pool_value_fwd against mil_absorbed_pool_fwd, bit for bit, on the ragged bags (1 to 11
    tiles): both entries merge a bag's tile partials with the same kernel, in eight interleaved groups folded in group
    order.  (A merge in tile order on the plain side differed from two tiles on: up to 1.8e-07 of max|pooled| at 700 keys,
    docs/lab_notes.md.)"""
    from mil_amd.segments import AttnSegs
    L = _lib()
    lens = A.ABS_BAGS
    c = A.absorbed_case(lens, C)
    B = len(lens)
    s = AttnSegs([1] * B, lens, DEV)
    d = {n: _dev(c[n]) for n in ("keys", "pe", "Wv", "bv")}
    Qp = _dev(A.absorbed(c)["Qp"])
    geo = (_p(s.k_off), _p(s.tile_map), _p(s.bag_tile_off), s.ntiles)
    out = []
    for value in (False, True):
        pooled, lse, o, ws = _sent(B, H, E), _sent(B, H), _sent(B, H * C), _sent(s.ntiles * H * (E + 2))
        if value:
            rc = L.mil_absorbed_pool_value_fwd(_p(d["keys"]), _p(d["pe"]), _p(Qp), *geo, B, H, C, E, _p(d["Wv"]), _p(d["bv"]),
                                               _p(pooled), _p(lse), _p(o), _p(ws), _st())
        else:
            rc = L.mil_absorbed_pool_fwd(_p(d["keys"]), _p(d["pe"]), _p(Qp), *geo, B, H, C, E, _p(pooled), _p(lse), _p(ws), _st())
        assert rc == 0
        out.append((pooled, lse))
    torch.cuda.synchronize()
    (p0, l0), (p1, l1) = out
    for b, n in enumerate(lens):
        dp = float((p1[b] - p0[b]).abs().max() / p0[b].abs().max())
        print(f"BITS | C {C} | bag {b} ({n} keys, {-(-n // 64)} tiles) | pooled differs in {int((p1[b] != p0[b]).sum())} of {H * E} "
              f"values, max |diff| / max|pooled| {dp:.2e} | lse differs in {int((l1[b] != l0[b]).sum())} of {H}")
    assert torch.equal(p1, p0) and torch.equal(l1, l0), "the value forward's pooled / lse differ from the plain forward's"
