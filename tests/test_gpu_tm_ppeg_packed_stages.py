"""GPU: the mil_tm_ppeg_*_packed entries on their own, through the C ABI, for bags of sides (3, 9, 1, 8, 17) - a grid narrower than
the 7 x 7 window, a one-cell bag between larger ones, exactly one 8-grid-row chunk, a chunk and a tail, two chunks and a tail, a
first and a last bag - and for (9,) alone.  Random data in ALL rows, the cls rows included, one weight set, a sentinel row behind the
R rows and sentinel floats behind dWf and db.  Every bag's rows of y and dx are BIT-equal to the single-bag entry on that bag's
slice; the sums that cross bags, dWf and db, are held with transmil_ref.hold("ppeg", ..) to the float64 sum over the bags of
transmil_ref.ppeg_run, the float32 CPU sum giving the noise; the fixed-order entry overwrites, reads nothing it has not written,
gives the same bits twice and, with one bag, the bits of mil_tm_ppeg_bwd_fixed.  (tests/test_tm_ppeg_packed_host.py shows in
float64 that the three silent mistakes - a neighbour's side, a window across a bag boundary, the cls row's + 1 lost - would break
these checks by orders of magnitude.)  No test hands the kernels a bad table."""
import ctypes
import functools

import pytest
import torch

import tm_fixed_ref as F
import tm_ppeg_packed_ref as Q
import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = F.SENT
TAIL = 64                            # sentinel floats behind the workspace's extent
PAD = 8                              # sentinel floats behind dWf and db


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return t.to(torch.float32).to(DEV).contiguous()


def _is_sent(t):
    return bool((t.cpu().view(torch.int32) == torch.tensor(SENT).view(torch.int32)).all())


def _tab(sides):
    from mil_amd import ops
    t = ops.tm_ppeg_table(sides, DEV)
    assert t.dev.tolist() == Q.table(sides) and t.rows == Q.row_off(sides)[-1]
    return t


@functools.lru_cache(maxsize=None)
def _inputs(sides):
    """The stage case on the device: x and dy with the sentinel row behind them, the six parameters."""
    p, x, dy = Q.stage_case(sides)
    rows = x.shape[0]
    xd, dyd = torch.full((rows + 1, 512), SENT, device=DEV), torch.full((rows + 1, 512), SENT, device=DEV)
    xd[:rows], dyd[:rows] = _dev(x), _dev(dy)
    return xd, dyd, [_dev(p["pos_layer." + n]) for n in R.PPEG_NAMES]


@functools.lru_cache(maxsize=None)
def _single(sides):
    """Per bag (y, dx) of mil_tm_ppeg_fwd / mil_tm_ppeg_bwd on the bag's slice: what every packed row is held to, bit for bit."""
    xd, dyd, W = _inputs(sides)
    out = []
    for b, s in enumerate(sides):
        rows = Q.bag_rows(sides, b)
        xb, dyb = xd[rows].clone(), dyd[rows].clone()
        y, dx = torch.empty_like(xb), torch.empty_like(xb)
        dWf, db = torch.zeros(512 * 49, device=DEV), torch.zeros(512, device=DEV)
        assert _lib().mil_tm_ppeg_fwd(_p(xb), s, *[_p(t) for t in W], _p(y), _st()) == 0
        assert _lib().mil_tm_ppeg_bwd(_p(dyb), _p(xb), s, _p(W[0]), _p(W[2]), _p(W[4]), _p(dx), _p(dWf), _p(db), _st()) == 0
        torch.cuda.synchronize()
        out.append((y.cpu(), dx.cpu()))
    return tuple(out)


def _per_bag_bits(tag, sides, got, which):
    x_or_dy = Q.stage_case(sides)[1 + which]
    for b in range(len(sides)):
        rows = Q.bag_rows(sides, b)
        assert F.bits_equal(got[rows], _single(sides)[b][which]), f"{tag}: bag {b} differs from the single-bag entry"
        assert torch.equal(got[rows.start], x_or_dy[rows.start].float()), f"{tag}: cls row of bag {b}"


def _hold_grads(tag, sides, dWf, db, dWf0=None, db0=None):
    """dWf, db against the float64 sum over the bags (+ what the buffers held), the float32 CPU sum as the noise reference."""
    ref, r32 = Q.grad_sums(sides), Q.grad_sums(sides, torch.float32)
    if dWf0 is not None:
        for name, sl in Q.CUT.items():
            for r, cast in ((ref, torch.float64), (r32, torch.float32)):
                r[f"d{name}.weight"] = r[f"d{name}.weight"] + dWf0[:, :, sl, sl].to(cast)
                r[f"d{name}.bias"] = r[f"d{name}.bias"] + db0.to(cast)
    R.hold("ppeg", tag, Q.got_grads(dWf, db), ref, r32, Q.grad_blocks())


@pytest.mark.parametrize("sides", Q.SIDES)
def test_forward(sides):
    xd, _, W = _inputs(sides)
    tab = _tab(sides)
    rows = tab.rows
    y = torch.full((rows + 1, 512), SENT, device=DEV)
    assert _lib().mil_tm_ppeg_fwd_packed(_p(xd), *[_p(t) for t in W], _p(y), *tab.args(), _st()) == 0
    torch.cuda.synchronize()
    assert _is_sent(y[rows]) and _is_sent(xd[rows])
    _per_bag_bits(f"fwd {sides}", sides, y[:rows].cpu(), 0)


def _bwd_atomic(sides, seed):
    xd, dyd, W = _inputs(sides)
    tab = _tab(sides)
    rows = tab.rows
    g = torch.Generator().manual_seed(seed)
    dWf0, db0 = torch.randn((512, 1, 7, 7), generator=g), torch.randn(512, generator=g)      # the gradients add onto these
    dWf, db = torch.full((512 * 49 + PAD,), SENT, device=DEV), torch.full((512 + PAD,), SENT, device=DEV)
    dWf[:512 * 49], db[:512] = dWf0.reshape(-1).to(DEV), db0.to(DEV)
    dx = torch.full((rows + 1, 512), SENT, device=DEV)
    assert _lib().mil_tm_ppeg_bwd_packed(_p(dyd), _p(xd), _p(W[0]), _p(W[2]), _p(W[4]), _p(dx), _p(dWf), _p(db), *tab.args(),
                                         _st()) == 0
    torch.cuda.synchronize()
    assert _is_sent(dx[rows]) and _is_sent(dWf[512 * 49:]) and _is_sent(db[512:])
    return dx[:rows].cpu(), dWf[:512 * 49].reshape(512, 1, 7, 7).cpu(), db[:512].cpu(), dWf0, db0


@pytest.mark.parametrize("sides", Q.SIDES)
def test_backward_atomic(sides):
    dx, dWf, db, dWf0, db0 = _bwd_atomic(sides, 71)
    _per_bag_bits(f"bwd {sides}", sides, dx, 1)
    _hold_grads(f"packed atomic {sides}", sides, dWf, db, dWf0, db0)


def _bwd_fixed(sides):
    xd, dyd, W = _inputs(sides)
    tab = _tab(sides)
    rows = tab.rows
    nws = _lib().mil_tm_ppeg_packed_ws_floats(tab.chunks)
    assert nws == Q.chunks(sides) * 50 * 512
    # everything pre-filled with the sentinel: a partial read before it is written, or a gradient added onto, would show
    ws = torch.full((nws + TAIL,), SENT, device=DEV)
    dWf, db = torch.full((512 * 49 + PAD,), SENT, device=DEV), torch.full((512 + PAD,), SENT, device=DEV)
    dx = torch.full((rows + 1, 512), SENT, device=DEV)
    assert _lib().mil_tm_ppeg_bwd_packed_fixed(_p(dyd), _p(xd), _p(W[0]), _p(W[2]), _p(W[4]), _p(dx), _p(dWf), _p(db), _p(ws),
                                               *tab.args(), _st()) == 0
    torch.cuda.synchronize()
    assert _is_sent(dx[rows]) and _is_sent(dWf[512 * 49:]) and _is_sent(db[512:]) and _is_sent(ws[nws:])
    assert not bool((ws[:nws] == SENT).any()), "a partial of the workspace was not written"
    return dx[:rows].cpu(), dWf[:512 * 49].reshape(512, 1, 7, 7).cpu(), db[:512].cpu()


@pytest.mark.parametrize("sides", Q.SIDES)
def test_backward_fixed(sides):
    dx, dWf, db = _bwd_fixed(sides)
    dx2, dWf2, db2 = _bwd_fixed(sides)
    assert F.bits_equal(dx, dx2) and F.bits_equal(dWf, dWf2) and F.bits_equal(db, db2)
    assert F.bits_equal(dx, _bwd_atomic(sides, 72)[0]), "dx of the fixed entry differs from the atomic one"
    _per_bag_bits(f"bwd fixed {sides}", sides, dx, 1)
    if len(sides) == 1:                                         # one bag: the bits of the single-bag fixed entry
        xd, dyd, W = _inputs(sides)
        s = sides[0]
        ws = torch.full((_lib().mil_tm_ppeg_ws_floats(s),), SENT, device=DEV)
        dWf1, db1, dx1 = torch.full((512 * 49,), SENT, device=DEV), torch.full((512,), SENT, device=DEV), torch.empty_like(xd)
        assert _lib().mil_tm_ppeg_bwd_fixed(_p(dyd), _p(xd), s, _p(W[0]), _p(W[2]), _p(W[4]), _p(dx1), _p(dWf1), _p(db1), _p(ws),
                                            _st()) == 0
        torch.cuda.synchronize()
        assert F.bits_equal(dWf.reshape(-1), dWf1) and F.bits_equal(db, db1)
    _hold_grads(f"packed fixed {sides}", sides, dWf, db)


def test_ops_function_against_per_bag_tm_ppeg():
    """ops.tm_ppeg_packed through autograd, deterministic and not: y and dx bit-equal per bag to ops.tm_ppeg, the six parameter
    gradients within the float64 bound of the sums; deterministic twice gives the same bits."""
    from mil_amd import ops
    sides = Q.SIDES[0]
    p, x, dy = Q.stage_case(sides)
    tab = _tab(sides)

    def run(fn, det):
        W = [_dev(p["pos_layer." + n]).requires_grad_(True) for n in R.PPEG_NAMES]
        xd = _dev(x).requires_grad_(True)
        y = fn(xd, W, det)
        y.backward(_dev(dy))
        torch.cuda.synchronize()
        return y.detach().cpu(), xd.grad.cpu(), {"d" + n: w.grad.cpu() for n, w in zip(R.PPEG_NAMES, W)}

    def packed(xd, W, det):
        return ops.tm_ppeg_packed(xd, tab, *W, deterministic=det)

    def bag_by_bag(xd, W, det):
        return torch.cat([ops.tm_ppeg(xd[Q.bag_rows(sides, b)], s, *W, deterministic=det) for b, s in enumerate(sides)], 0)

    y0, dx0, _ = run(bag_by_bag, True)
    for det in (True, False):
        y, dx, gr = run(packed, det)
        assert F.bits_equal(y, y0) and F.bits_equal(dx, dx0), det
        R.hold("ppeg", f"ops det {det}", gr, Q.grad_sums(sides), Q.grad_sums(sides, torch.float32), Q.grad_blocks())
        if det:
            _, _, again = run(packed, True)
            assert all(F.bits_equal(gr[k], again[k]) for k in gr)
