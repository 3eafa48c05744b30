"""GPU: the grouped start of the pseudo-inverse (mil_tm_pinv_init_bags, mil_tm_pinv_init_bwd_bags and its _fixed twin) alone, on
nb = 1, 2, 3 bags whose scales differ by more than 1 % (tests/test_tm_bags_host.py): every bag against the float64
restatement of ONE bag (tests/transmil_ref.py: pinv_run) at the single-bag stage's bound, bit-equal to the single-bag entry on
the bag's slices, and with sentinel rows in front of bag 0 and behind bag nb - 1 of every output."""
import ctypes

import pytest
import torch

import tm_bags_ref as G
import tm_fixed_ref as F
import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, M = R.H, R.M


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(nb, width, dtype=torch.float32, fill=F.SENT, inner=None):
    """[nb + 2, width] on the device: a sentinel row, the nb rows the entry owns (`inner`: their contents), a sentinel row."""
    buf = torch.full((nb + 2, width), fill, dtype=dtype)
    if inner is not None:
        buf[1:-1] = inner.reshape(nb, width)
    return buf.to(DEV)


def _guards_intact(buf, fill=F.SENT):
    ref = torch.full((buf.shape[1],), fill, dtype=buf.dtype)
    return F.bits_equal(buf[0], ref) and F.bits_equal(buf[-1], ref) if buf.dtype == torch.float32 else (
        bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all()))


def _init_bags(a2s):
    """The grouped forward on the stacked bags -> (A2 on the device [nb, 8, 256, 256], scale [nb, 19], arg [nb, 9], Z0)."""
    nb = len(a2s)
    ad = torch.stack([a.float() for a in a2s]).to(DEV).contiguous()
    scale, arg = _guarded(nb, G.SCALE_WORDS), _guarded(nb, G.ARG_WORDS, torch.int32, -7)
    Z = _guarded(nb, G.BAG)
    assert _lib().mil_tm_pinv_init_bags(_p(ad), nb, _p(scale[1:]), _p(arg[1:]), _p(Z[1:]), _st()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(scale) and _guards_intact(arg, -7) and _guards_intact(Z)
    return ad, scale[1:-1], arg[1:-1], Z[1:-1].reshape(nb, H, M, M)


def _init_one(a2):
    ad = a2.float().to(DEV).contiguous()
    scale = torch.empty(G.SCALE_WORDS, device=DEV)
    arg = torch.empty(G.ARG_WORDS, device=DEV, dtype=torch.int32)
    Z = torch.empty((H, M, M), device=DEV)
    assert _lib().mil_tm_pinv_init(_p(ad), _p(scale), _p(arg), _p(Z), _st()) == 0
    torch.cuda.synchronize()
    return ad, scale, arg, Z


@pytest.mark.parametrize("nb", [1, 2, 3])
def test_forward_per_bag(nb):
    cases = [G.stage_case(i) for i in range(nb)]
    _, scale, arg, Z = _init_bags([c[0] for c in cases])
    for b, (a2, _, ref, r32) in enumerate(cases):
        csum = a2.sum(-2)
        want = [ref["arg"]] + [h * M + int(csum[h].argmax()) for h in range(H)]     # local to the bag
        assert arg[b].cpu().tolist() == want and want[0] == G.STAGE_ARGS[b], (nb, b)
        got = {"scale": scale[b, :3], "row_max": scale[b, 3:3 + H], "col_max": scale[b, 3 + H:], "Z0": Z[b]}
        R.hold("pinv_init", f"bags {nb} bag {b} fwd", got, ref, r32, {k: R.whole() for k in got})
        _, s1, a1, Z1 = _init_one(a2)                                              # the single-bag entry on the bag's slices
        assert F.bits_equal(scale[b], s1) and torch.equal(arg[b], a1) and F.bits_equal(Z[b], Z1), (nb, b)


def _dA0(nb):
    g = torch.Generator().manual_seed(60 + nb)
    return torch.randn((nb, H, M, M), generator=g)                   # dA2 comes in holding the six iterations' share


def _bwd_bags(cases, ad, scale, arg, Z, fixed, dA0):
    nb = len(cases)
    dZ = torch.stack([c[1].float() for c in cases]).to(DEV).contiguous()
    dA = _guarded(nb, G.BAG, inner=dA0)
    Zc, sc, ac = Z.contiguous(), scale.contiguous(), arg.contiguous()
    if fixed:
        assert _lib().mil_tm_pinv_ws_floats_bags(nb) == 256 * nb
        ws = _guarded(nb, 256)
        assert _lib().mil_tm_pinv_init_bwd_bags_fixed(_p(dZ), _p(Zc), _p(sc), _p(ac), nb, _p(dA[1:]), _p(ws[1:]), _st()) == 0
    else:
        ws = _guarded(nb, 1, inner=torch.zeros(nb))
        assert _lib().mil_tm_pinv_init_bwd_bags(_p(dZ), _p(Zc), _p(sc), _p(ac), nb, _p(dA[1:]), _p(ws[1:]), _st()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(dA) and _guards_intact(ws)
    return dA[1:-1].reshape(nb, H, M, M).clone()


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_backward_per_bag(nb, fixed):
    """dS2 per bag through the row-softmax backward, as test_gpu_transmil_stages.test_pinv_init takes it."""
    cases = [G.stage_case(i) for i in range(nb)]
    ad, scale, arg, Z = _init_bags([c[0] for c in cases])
    dA0 = _dA0(nb)
    dA = _bwd_bags(cases, ad, scale, arg, Z, fixed, dA0)
    if fixed:
        again = _bwd_bags(cases, ad, scale, arg, Z, True, dA0)
        assert F.bits_equal(dA, again), "the fixed-order entry gave two answers"
    for b, (a2, dZ, ref, r32) in enumerate(cases):
        if fixed:                                                  # bit-equal to the single-bag entry on the bag's slices
            a1, s1, g1, Z1 = _init_one(a2)
            d1 = dA0[b].to(DEV).contiguous()
            ws = torch.empty(_lib().mil_tm_pinv_ws_floats(), device=DEV)
            assert _lib().mil_tm_pinv_init_bwd_fixed(_p(dZ.float().to(DEV).contiguous()), _p(Z1), _p(s1), _p(g1), _p(d1), _p(ws),
                                                     _st()) == 0
            torch.cuda.synchronize()
            assert F.bits_equal(dA[b], d1), (nb, b)
        dS = dA[b].contiguous()
        assert _lib().mil_tm_softmax_rows_bwd(_p(ad[b]), _p(dS), H * M, M, _st()) == 0
        torch.cuda.synchronize()
        want = {"dS2": ref["dS2"] + R.softmax_rows_bwd(a2, dA0[b].double())}
        w32 = {"dS2": r32["dS2"] + R.softmax_rows_bwd(a2.float(), dA0[b])}
        R.hold("pinv_init", f"bags {nb} bag {b} bwd fixed {fixed}", {"dS2": dS}, want, w32, {"dS2": R.whole()})


def test_first_on_ties_inside_one_bag_of_two():
    """Bag 1 is the construction of test_gpu_transmil_stages.test_pinv_init_first_on_ties: two exactly equal largest column
    sums inside head 2 (columns 17 and 200) and the same again in head 6 - arg is the first, local to the bag.  Bag 0 in front
    of it has larger column sums than any of bag 1's; they must not reach bag 1's maxima."""
    g = torch.Generator().manual_seed(8)
    a2 = torch.randint(1, 8, (H, M, M), generator=g).double() / 8192
    a2[2, :, 17] += 1.0 / 1024
    a2[2, :, 200] = a2[2, :, 17]
    a2[6, :, 5] = a2[2, :, 17]
    first = G.stage_case(0)[0]
    ref = R.z0(a2)
    assert float(R.z0(first)["scale"][2]) > float(ref["scale"][2]) and ref["arg"] == 2 * M + 17
    _, scale, arg, Z = _init_bags([first, a2])
    assert int(arg[1, 0]) == 2 * M + 17 and int(arg[1, 1 + 2]) == 2 * M + 17 and int(arg[1, 1 + 6]) == 6 * M + 5
    assert torch.equal(scale[1, 3:3 + H].cpu().double(), ref["row_max"]) and torch.equal(scale[1, 3 + H:].cpu().double(), ref["col_max"])
    assert torch.equal(scale[1, :3].cpu().double(), ref["scale"])
    R.hold("pinv_init", "bags ties fwd", {"Z0": Z[1]}, ref, R.z0(a2.float()), {"Z0": R.whole()})
    assert int(arg[0, 0]) == G.STAGE_ARGS[0]
