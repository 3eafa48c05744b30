"""GPU: ops.nystrom_core_bags - the Nystrom cores of a step's bags with the landmark-side chain as one set of launches - on
three bags (n_pad 256, 512 and a peaked 256, whose pseudo-inverse scales are 1.77, 1.20 and 7.32: tests/test_tm_bags_host.py
shows that one scale for the batch would break the bound on bags 0 and 1 by more than 10^4 x) against ops.nystrom_core per bag
and against the float64 restatement of one bag per call (tests/transmil_ref.py)."""
import functools

import pytest
import torch

import tm_bags_ref as G
import tm_fixed_ref as F
import tm_pieces_ref as P
import transmil_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROUTES = {"maps": dict(), "fused": dict(fused_a1=True, fused_a3=True), "pieces": dict(pieces=3)}


def _ops():
    from mil_amd import ops
    return ops


def _inputs(bags):
    qs = [G.core_ref(i)[0].float().to(DEV).requires_grad_(True) for i in bags]
    w = G.core_ref(0)[1].float().to(DEV).requires_grad_(True)
    dOs = [G.core_ref(i)[2].float().to(DEV) for i in bags]
    return qs, w, dOs


def _run_bags(bags, **kw):
    """One nystrom_core_bags call over the bags, forward + backward -> ([{out, dqkv}], dw, launch log)."""
    qs, w, dOs = _inputs(bags)
    with G.recorded() as log:
        outs = _ops().nystrom_core_bags(qs, w, **kw)
        torch.autograd.backward(outs, dOs)
    torch.cuda.synchronize()
    return [{"out": o.detach(), "dqkv": q.grad} for o, q in zip(outs, qs)], w.grad.reshape(R.H, R.CONV), log


def _run_each(bags, **kw):
    """The same bags through nystrom_core one after another, dw accumulated by autograd in bag order."""
    qs, w, dOs = _inputs(bags)
    got = []
    with G.recorded() as log:
        for q, dO in zip(qs, dOs):
            o, attn = _ops().nystrom_core(q, w, **kw)
            assert attn is None
            o.backward(dO)
            got.append({"out": o.detach(), "dqkv": q.grad})
    torch.cuda.synchronize()
    return got, w.grad.reshape(R.H, R.CONV), log


@functools.lru_cache(maxsize=None)
def _dw_ref(bags):
    """(float64, float32) sum of the bags' dw, the float32 one added in bag order."""
    d64 = sum(G.core_ref(i)[4]["dw"] for i in bags)
    d32 = functools.reduce(lambda a, b: a + b, [G.core_ref(i)[5]["dw"] for i in bags])
    return d64, d32


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_deterministic_bits_equal_the_bag_by_bag_route(route):
    kw = dict(deterministic=True, **ROUTES[route])
    got, dw, _ = _run_bags((0, 1, 2), **kw)
    each, _, _ = _run_each((0, 1, 2), **kw)
    for b in range(3):
        for k in ("out", "dqkv"):
            assert F.bits_equal(got[b][k], each[b][k]), (route, b, k)
    d64, d32 = _dw_ref((0, 1, 2))
    hold = P.hold if route == "pieces" else R.hold
    hold("core", f"bags dw {route}", {"dw": dw}, {"dw": d64}, {"dw": d32}, {"dw": R.whole()})
    got2, dw2, _ = _run_bags((0, 1), **kw)                           # a two-term sum is order-free: dw is bit-equal too
    each2, dwe2, _ = _run_each((0, 1), **kw)
    assert F.bits_equal(dw2, dwe2), route
    for b in range(2):
        for k in ("out", "dqkv"):
            assert F.bits_equal(got2[b][k], each2[b][k]), (route, b, k)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_bag_holds_the_float64_bound(route):
    got, dw, _ = _run_bags((0, 1, 2), **ROUTES[route])
    hold = P.hold if route == "pieces" else R.hold
    for b in range(3):
        qkv, _, _, pad, ref, r32 = G.core_ref(b)
        blocks = R.core_blocks(qkv.shape[0], pad)
        blocks.pop("dw")
        hold("core", f"bags {route} bag {b}", got[b], ref, r32, blocks)
    d64, d32 = _dw_ref((0, 1, 2))
    hold("core", f"bags {route} dw", {"dw": dw}, {"dw": d64}, {"dw": d32}, {"dw": R.whole()})


def test_launch_log_of_three_bags():
    """One call with three bags, forward + backward: the 24 + 48 chain products once, at batch 24; the grouped start and its
    backward once each; no single-bag start.  The same bags through nystrom_core: today's entry list, three times."""
    for det in (False, True):
        _, _, log = _run_bags((0, 1, 2), deterministic=det)
        names = [e[0] for e in log]
        cube = [e for e in log if e[0] in G.PRODUCTS and e[3] == (256, 256, 256)]
        assert len(cube) == 24 + 48 and all(e[2] == 24 and e[1] == 1 for e in cube), (det, len(cube))
        assert names.count("mil_tm_pinv_init_bags") == 1
        assert names.count("mil_tm_pinv_init_bwd_bags_fixed" if det else "mil_tm_pinv_init_bwd_bags") == 1
        assert names.count("mil_tm_pinv_init_bwd_bags" if det else "mil_tm_pinv_init_bwd_bags_fixed") == 0
        assert not set(names) & set(G.SINGLE)
        small = [e for e in log if e[0] in G.PRODUCTS and e[2] == 24 and e[3] != (256, 256, 256)]
        assert sorted(e[3] for e in small) == sorted([(256, 256, 64)] * 2 + [(256, 64, 256)] * 4)    # A2 dZ | U dW dkL dqL
        assert names.count("mil_tm_landmarks") == 3 and names.count("mil_tm_landmarks_bwd") == 3
        assert names.count("mil_tm_resconv") == 3

        _, _, each = _run_each((0, 1, 2), deterministic=det)
        enames = [e[0] for e in each]
        assert not set(enames) & set(G.NAMES)
        assert enames.count("mil_tm_pinv_init") == 3
        assert enames.count("mil_tm_pinv_init_bwd_fixed" if det else "mil_tm_pinv_init_bwd") == 3
        ecube = [e for e in each if e[0] in G.PRODUCTS and e[3] == (256, 256, 256)]
        assert len(ecube) == 3 * 72 and all(e[2] == 8 for e in ecube)
        # per bag, the bag-by-bag route launches what the batched one does, plus the chain: the products differ by the
        # 2 x 78 launches that the two other bags no longer issue (72 chain products and A2, U, dZ, dW, dkL, dqL)
        prod = lambda lg: sum(e[0] in G.PRODUCTS for e in lg)      # noqa: E731
        assert prod(each) - prod(log) == 2 * 78


def test_the_single_bag_core_keeps_its_entry_list():
    """nystrom_core on the n_pad = 512 bag: the entries, in order, that the phases of one bag state (maps route, atomic sums)."""
    _, _, log = _run_each((1,))
    names = [e[0] for e in log]
    bg, sm, smb = "mil_tm_bgemm", "mil_tm_softmax_rows", "mil_tm_softmax_rows_bwd"
    fwd = (["mil_tm_landmarks", bg, bg, bg, sm, sm, sm, bg, "mil_tm_pinv_init"] + [bg] * 24 + [bg, bg, "mil_tm_resconv"])
    bwd = ([bg] * 4 + [bg, bg, "mil_tm_resconv_bwd", smb, smb] + [bg] * 48 + ["mil_tm_pinv_init_bwd", smb]
           + [bg] * 6 + ["mil_tm_landmarks_bwd"])
    assert names == fwd + bwd, names


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_one_bag_equals_nystrom_core(route):
    kw = dict(deterministic=True, **ROUTES[route])
    got, dw, log = _run_bags((1,), **kw)
    each, dwe, _ = _run_each((1,), **kw)
    assert F.bits_equal(got[0]["out"], each[0]["out"]) and F.bits_equal(got[0]["dqkv"], each[0]["dqkv"]) and F.bits_equal(dw, dwe)
    assert [e[0] for e in log].count("mil_tm_pinv_init_bags") == 1
