"""GPU: every mil_tm_*_packed entry on its own, through the C ABI, and ops.nystrom_core_packed.  The inputs are random in ALL
rows, the pad rows included, so that a leak across a bag boundary shows; block counts [1, 2, 1, 3] (a first bag, a one-block bag
between larger ones, 1, 2 and 3 forward chunks, 2, 4 and 6 backward chunks) and [2] alone.  Every per-bag output of every packed
entry - qL, kL, W, lse3, O, lse1, the conv's addend, the dqkv rows, dqL, dU, dkL - is BIT-equal to the single-bag entry on that
bag's rows and slices: the order of every per-bag sum is unchanged.  The one sum across bags, the conv's dw (atomic and fixed),
is held to the float64 sum of the per-bag references at the bound tests/test_gpu_tm_fixed_stages.py holds
mil_tm_resconv_bwd_fixed to (transmil_ref.hold, stage "resconv").  tests/test_tm_packed_host.py shows in float64 that these
cases see a conv window across a boundary, a neighbour's landmark group and a merge over all chunks."""
import ctypes
import functools

import pytest
import torch

import tm_fixed_ref as F
import tm_packed_ref as P
import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = F.SENT
QS = R.DH ** -0.5


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(n):
    return torch.full((int(n) + 64,), float("nan"), device=DEV)


def _tab(blocks):
    return torch.tensor(P.table(blocks), dtype=torch.int32, device=DEV), len(blocks), sum(blocks)


def _case(blocks):
    return {k: v.to(DEV).contiguous() for k, v in P.stage_case(blocks).items()}


def _same(tag, got, want):
    assert F.bits_equal(got, want), f"{tag}: not bit-equal, max |diff| {float((got.cpu() - want.cpu()).abs().max()):.3e}"


def _ok(rc):
    assert rc == 0, rc


@functools.lru_cache(maxsize=None)
def _dw_refs(blocks):
    """The conv's dw [8, 33] of the stage case as the sum of the per-bag references, in float64 and in float32: computed once,
    shared by the stage test and the core tests (dw depends on dO and the v columns alone)."""
    cpu = P.stage_case(blocks)
    out = []
    for dt in (torch.float64, torch.float32):
        acc = torch.zeros((R.H, R.CONV), dtype=dt)
        for b in range(len(blocks)):
            rows = P.bag_rows(blocks, b)
            acc = acc + R.resconv_bwd(cpu["dO"][rows].to(dt), cpu["qkv"][rows].to(dt), cpu["w"].to(dt))[2]
        out.append({"dw": acc})
    return out


def _hold_dw(tag, dw, blocks):
    ref, r32 = _dw_refs(blocks)
    R.hold("resconv", tag, {"dw": dw.reshape(R.H, R.CONV).cpu()}, ref, r32, {"dw": R.whole()})


@pytest.mark.parametrize("blocks", P.BLOCKS)
def test_landmarks_and_their_backward(blocks):
    L, c = _lib(), _case(blocks)
    tab, nb, tb = _tab(blocks)
    qL = torch.full((nb, R.H, R.M, R.DH), SENT, device=DEV)
    kL = torch.full_like(qL, SENT)
    _ok(L.mil_tm_landmarks_packed(_p(c["qkv"]), QS, _p(qL), _p(kL), _p(tab), nb, tb, _st()))
    dq = c["dqkv0"].clone()
    _ok(L.mil_tm_landmarks_bwd_packed(_p(c["dqL"]), _p(c["dkL"]), QS, _p(dq), _p(tab), nb, tb, _st()))
    for b in range(nb):
        rows = P.bag_rows(blocks, b)
        n = rows.stop - rows.start
        q1, k1 = torch.empty((R.H, R.M, R.DH), device=DEV), torch.empty((R.H, R.M, R.DH), device=DEV)
        _ok(L.mil_tm_landmarks(_p(c["qkv"][rows].contiguous()), n, QS, _p(q1), _p(k1), _st()))
        _same(f"qL bag {b}", qL[b], q1)
        _same(f"kL bag {b}", kL[b], k1)
        d1 = c["dqkv0"][rows].clone()
        _ok(L.mil_tm_landmarks_bwd(_p(c["dqL"][b]), _p(c["dkL"][b]), n, QS, _p(d1), _st()))
        _same(f"dqkv bag {b}", dq[rows], d1)


@pytest.mark.parametrize("blocks", P.BLOCKS)
def test_lmk_attn_forward_and_backward(blocks):
    L, c = _lib(), _case(blocks)
    tab, nb, tb = _tab(blocks)
    W = torch.full((nb, R.H, R.M, R.DH), SENT, device=DEV)
    lse = torch.full((nb, R.H, R.M), SENT, device=DEV)
    ws = _ws(L.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 0))
    _ok(L.mil_tm_lmk_attn_fwd_packed(_p(c["qkv"]), _p(c["qL"]), _p(W), _p(lse), _p(ws), _p(tab), nb, tb, _st()))
    dq = c["dqkv0"].clone()
    dqL = torch.full((nb, R.H, R.M, R.DH), SENT, device=DEV)
    wsb = _ws(L.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 1))
    _ok(L.mil_tm_lmk_attn_bwd_packed(_p(c["qkv"]), _p(c["qL"]), _p(W), _p(lse), _p(c["dW"]), _p(dq), _p(dqL), _p(wsb), _p(tab), nb, tb,
                                     _st()))
    assert bool(torch.isnan(ws[-64:]).all()) and bool(torch.isnan(wsb[-64:]).all()), "written behind the workspace"
    _same("dqkv q columns untouched", dq[:, :512], c["dqkv0"][:, :512])
    for b in range(nb):
        rows = P.bag_rows(blocks, b)
        n = rows.stop - rows.start
        qkv1 = c["qkv"][rows].contiguous()
        W1, l1 = torch.empty((R.H, R.M, R.DH), device=DEV), torch.empty((R.H, R.M), device=DEV)
        _ok(L.mil_tm_lmk_attn_fwd(_p(qkv1), _p(c["qL"][b]), n, _p(W1), _p(l1), _p(_ws(L.mil_tm_lmk_attn_ws_floats(n, 0))), _st()))
        _same(f"W bag {b}", W[b], W1)
        _same(f"lse3 bag {b}", lse[b], l1)
        d1, g1 = c["dqkv0"][rows].clone(), torch.empty((R.H, R.M, R.DH), device=DEV)
        _ok(L.mil_tm_lmk_attn_bwd(_p(qkv1), _p(c["qL"][b]), _p(W1), _p(l1), _p(c["dW"][b]), n, _p(d1), _p(g1),
                                  _p(_ws(L.mil_tm_lmk_attn_ws_floats(n, 1))), _st()))
        _same(f"dk|dv bag {b}", dq[rows], d1)
        _same(f"dqL bag {b}", dqL[b], g1)


@pytest.mark.parametrize("blocks", P.BLOCKS)
def test_tok_attn_forward_and_backward(blocks):
    L, c = _lib(), _case(blocks)
    tab, nb, tb = _tab(blocks)
    rows_all = 256 * tb
    O = torch.full((rows_all, 512), SENT, device=DEV)
    lse = torch.full((R.H, rows_all), SENT, device=DEV)
    _ok(L.mil_tm_tok_attn_fwd_packed(_p(c["qkv"]), _p(c["kL"]), _p(c["U"]), _p(O), _p(lse), None, _p(tab), nb, tb, _st()))
    dq = c["dqkv0"].clone()
    dU = torch.full((nb, R.H, R.M, R.DH), SENT, device=DEV)
    dkL = torch.full_like(dU, SENT)
    wsb = _ws(L.mil_tm_tok_attn_packed_ws_floats(tb, nb, 1))
    _ok(L.mil_tm_tok_attn_bwd_packed(_p(c["qkv"]), _p(c["kL"]), _p(c["U"]), _p(lse), _p(c["dO"]), _p(dq), _p(dU), _p(dkL), _p(wsb),
                                     _p(tab), nb, tb, _st()))
    assert bool(torch.isnan(wsb[-64:]).all()), "written behind the workspace"
    _same("dqkv k|v columns untouched", dq[:, 512:], c["dqkv0"][:, 512:])
    for b in range(nb):
        rows = P.bag_rows(blocks, b)
        n = rows.stop - rows.start
        qkv1, dO1 = c["qkv"][rows].contiguous(), c["dO"][rows].contiguous()
        O1, l1 = torch.empty((n, 512), device=DEV), torch.empty((R.H, n), device=DEV)
        _ok(L.mil_tm_tok_attn_fwd(_p(qkv1), _p(c["kL"][b]), _p(c["U"][b]), n, _p(O1), _p(l1), None, _st()))
        _same(f"O bag {b}", O[rows], O1)
        _same(f"lse1 bag {b}", lse[:, rows], l1)
        d1 = c["dqkv0"][rows].clone()
        u1, k1 = torch.empty((R.H, R.M, R.DH), device=DEV), torch.empty((R.H, R.M, R.DH), device=DEV)
        _ok(L.mil_tm_tok_attn_bwd(_p(qkv1), _p(c["kL"][b]), _p(c["U"][b]), _p(l1), _p(dO1), n, _p(d1), _p(u1), _p(k1),
                                  _p(_ws(L.mil_tm_tok_attn_ws_floats(n, 1))), _st()))
        _same(f"dq bag {b}", dq[rows], d1)
        _same(f"dU bag {b}", dU[b], u1)
        _same(f"dkL bag {b}", dkL[b], k1)


@pytest.mark.parametrize("blocks", P.BLOCKS)
def test_resconv_forward_and_backward(blocks):
    L, c = _lib(), _case(blocks)
    tab, nb, tb = _tab(blocks)
    w = c["w"].contiguous()
    out = c["out0"].clone()
    _ok(L.mil_tm_resconv_packed(_p(c["qkv"]), _p(w), _p(out), _p(tab), nb, tb, _st()))
    dq_a, dq_f = c["dqkv0"].clone(), c["dqkv0"].clone()
    dw_a = torch.zeros(R.H * R.CONV, device=DEV)
    dw_f = torch.full((R.H * R.CONV + 8,), SENT, device=DEV)                # not zeroed: the fold overwrites [8, 33]
    _ok(L.mil_tm_resconv_bwd_packed(_p(c["dO"]), _p(c["qkv"]), _p(w), _p(dq_a), _p(dw_a), _p(tab), nb, tb, _st()))
    wsf = _ws(L.mil_tm_resconv_packed_ws_floats(tb, nb, 1))
    _ok(L.mil_tm_resconv_bwd_packed_fixed(_p(c["dO"]), _p(c["qkv"]), _p(w), _p(dq_f), _p(dw_f), _p(wsf), _p(tab), nb, tb, _st()))
    dw_f2 = torch.full_like(dw_f, SENT)
    _ok(L.mil_tm_resconv_bwd_packed_fixed(_p(c["dO"]), _p(c["qkv"]), _p(w), _p(c["dqkv0"].clone()), _p(dw_f2), _p(_ws(tb * 264)), _p(tab),
                                          nb, tb, _st()))
    assert bool(torch.isnan(wsf[-64:]).all()) and bool((dw_f[R.H * R.CONV:] == SENT).all())
    _same("dw fixed, two runs", dw_f, dw_f2)
    _same("dv: fixed and atomic entries", dq_f, dq_a)
    _same("dqkv q|k columns untouched", dq_a[:, :1024], c["dqkv0"][:, :1024])
    for b in range(nb):
        rows = P.bag_rows(blocks, b)
        n = rows.stop - rows.start
        qkv1, dO1 = c["qkv"][rows].contiguous(), c["dO"][rows].contiguous()
        o1 = c["out0"][rows].clone()
        _ok(L.mil_tm_resconv(_p(qkv1), _p(w), n, _p(o1), _st()))
        _same(f"conv addend bag {b}", out[rows], o1)
        d1, dw1 = c["dqkv0"][rows].clone(), torch.zeros(R.H * R.CONV, device=DEV)
        _ok(L.mil_tm_resconv_bwd(_p(dO1), _p(qkv1), _p(w), n, _p(d1), _p(dw1), _st()))
        _same(f"dv bag {b}", dq_a[rows], d1)
    for tag, got in (("atomic", dw_a), ("fixed", dw_f[:R.H * R.CONV])):
        _hold_dw(f"packed {tag} blocks {blocks}", got, blocks)


def _core(fn, qkv, w, dO):
    q, wr = qkv.clone().requires_grad_(True), w.clone().requires_grad_(True)
    outs = fn(q, wr)
    O = outs if isinstance(outs, torch.Tensor) else torch.cat(list(outs), 0)
    O.backward(dO)
    return {"O": O.detach(), "dqkv": q.grad, "dw": wr.grad}


@pytest.mark.parametrize("pieces", [0, 3])
@pytest.mark.parametrize("blocks", P.BLOCKS)
def test_core_packed_against_core_bags(blocks, pieces):
    """ops.nystrom_core_packed forward and backward under deterministic: O and dqkv bit-equal per bag to ops.nystrom_core_bags
    with both fused switches on; two packed runs give the same bits in everything, dw included; dw - one fold over all
    chunks - is held to the float64 sum of the per-bag references at the conv stage's bound."""
    from mil_amd import ops
    c = _case(blocks)
    w = c["w"].reshape(R.H, 1, R.CONV, 1).contiguous()
    nb = len(blocks)
    split = lambda t: [t[P.bag_rows(blocks, b)] for b in range(nb)]        # noqa: E731
    bags = _core(lambda q, wr: ops.nystrom_core_bags(split(q), wr, fused_a3=True, fused_a1=True, deterministic=True, pieces=pieces),
                 c["qkv"], w, c["dO"])
    with F.recorded() as log:
        packed = _core(lambda q, wr: ops.nystrom_core_packed(q, list(blocks), wr, deterministic=True, pieces=pieces), c["qkv"], w, c["dO"])
    names = [n for n, _ in log]
    assert not set(names) & set(P.SINGLE), set(names) & set(P.SINGLE)
    assert {n for n in P.STATUS if n != "mil_tm_resconv_bwd_packed"} <= set(names)
    assert names.count("mil_tm_pinv_init_bags") == 1
    again = _core(lambda q, wr: ops.nystrom_core_packed(q, ops.tm_packed_table(blocks, DEV), wr, deterministic=True, pieces=pieces),
                  c["qkv"], w, c["dO"])
    for k in ("O", "dqkv", "dw"):
        _same(f"two packed runs, {k}", packed[k], again[k])
    for b in range(nb):
        rows = P.bag_rows(blocks, b)
        _same(f"O bag {b}", packed["O"][rows], bags["O"][rows])
        _same(f"dqkv bag {b}", packed["dqkv"][rows], bags["dqkv"][rows])
    _hold_dw(f"core packed blocks {blocks} pieces {pieces}", packed["dw"], blocks)


def test_core_packed_atomic_route_runs():
    """Without deterministic the conv's dw takes the atomic entry; O is still bit-equal to the bags route."""
    from mil_amd import ops
    blocks = P.BLOCKS[0]
    c = _case(blocks)
    w = c["w"].reshape(R.H, 1, R.CONV, 1).contiguous()
    with F.recorded() as log:
        packed = _core(lambda q, wr: ops.nystrom_core_packed(q, list(blocks), wr, deterministic=False, pieces=0), c["qkv"], w, c["dO"])
    assert "mil_tm_resconv_bwd_packed" in [n for n, _ in log]
    det = _core(lambda q, wr: ops.nystrom_core_packed(q, list(blocks), wr, deterministic=True, pieces=0), c["qkv"], w, c["dO"])
    _same("O", packed["O"], det["O"])
    _hold_dw("core packed atomic", packed["dw"], blocks)
