"""GPU: the Nystrom core and the TransMIL module with the core's K >= 256 products on split-bf16 MFMA (pieces=3 /
TransMIL.gemm_pieces = 3 / MIL_TM_PIECES=3).  The route is held to the references and bounds of the fp32 route: the float64
restatement per block at k x max(e32, 1e-7) (tm_pieces_ref.K_STAGE), the reference-made goldens at the tolerances of
tests/test_gpu_transmil.py, the replayed step at the tolerance of tests/test_gpu_transmil_graph.py.  It goes with the fused
passes and with the fixed-order sums (two runs bit-equal), and leaves the default route's bits alone."""
import functools

import pytest
import torch

import tm_fixed_ref as F
import tm_pieces_ref as P
import transmil_ref as R
import test_gpu_transmil as T
from test_gpu_transmil_graph import _feed, _model as _graph_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
rel = T.rel
PIECES = ("mil_tm_bgemm_pieces", "mil_tm_bgemm_pieces_fixed")


def _ops():
    from mil_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _core_ref(n_pad, peak):
    """The case and its float64 / float32 restatements, computed once and shared (never modified) by the tests below."""
    qkv, w, dO, pad = R.core_case(n_pad, peak)
    return qkv, w, dO, pad, R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32)


def _core_gpu(qkv, w, dO, **kw):
    qd = qkv.float().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    with F.recorded() as log:
        o, attn = _ops().nystrom_core(qd, wd, **kw)
        assert attn is None
        o.backward(dO.float().to(DEV))
    torch.cuda.synchronize()
    return {"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad.reshape(R.H, R.CONV)}, [n for n, _ in log]


def _core_hold(n_pad, peak, tag, **kw):
    qkv, w, dO, pad, ref, r32 = _core_ref(n_pad, peak)
    got, names = _core_gpu(qkv, w, dO, pieces=3, **kw)
    assert set(names) & set(PIECES), "the split-bf16 entries did not run"
    P.hold("core", f"n_pad {n_pad} peak {peak} {tag}", got, ref, r32, R.core_blocks(n_pad, pad))
    return got


@pytest.mark.parametrize("peak", [1.0, R.PEAK])
@pytest.mark.parametrize("n_pad", [256, 512])                  # the 64-row tile alone; the 128-row tile and the smallest split-K
def test_nystrom_core_pieces(n_pad, peak):
    _core_hold(n_pad, peak, "maps")


def test_nystrom_core_pieces_n2048():
    _core_hold(2048, 1.0, "maps")


@pytest.mark.parametrize("peak", [1.0, R.PEAK])
@pytest.mark.parametrize("n_pad", [256, 512])
def test_nystrom_core_pieces_with_the_fused_passes(n_pad, peak):
    _core_hold(n_pad, peak, "fused a1 a3", fused_a1=True, fused_a3=True)


@pytest.mark.parametrize("fused", [dict(), dict(fused_a1=True, fused_a3=True)])
@pytest.mark.parametrize("n_pad", [256, 512])
def test_nystrom_core_pieces_deterministic_twice(n_pad, fused):
    got = _core_hold(n_pad, 1.0, f"deterministic {sorted(fused)}", deterministic=True, **fused)
    again = _core_hold(n_pad, 1.0, f"deterministic again {sorted(fused)}", deterministic=True, **fused)
    for k in got:
        assert F.bits_equal(got[k], again[k]), (n_pad, fused, k)


def test_the_route_names_the_products():
    """What one core call launches at n_pad = 512: with pieces=3 every product with K >= 256 on the split-bf16 entries and
    the K = 64 products on mil_tm_bgemm; with pieces=0 nothing on them."""
    qkv, w, dO, _, _, _ = _core_ref(512, 1.0)
    _, off = _core_gpu(qkv, w, dO, pieces=0)
    _, on = _core_gpu(qkv, w, dO, pieces=3)
    _, det = _core_gpu(qkv, w, dO, pieces=3, deterministic=True)
    assert not set(off) & set(PIECES)
    n_all = sum(n in ("mil_tm_bgemm", "mil_tm_bgemm_fixed") for n in off)
    assert on.count("mil_tm_bgemm") == 6 and on.count("mil_tm_bgemm_pieces") == n_all - 6      # A1, A2, A3, dA1, dZ, dA3
    assert det.count("mil_tm_bgemm") == 6 and "mil_tm_bgemm_pieces_fixed" in det and "mil_tm_bgemm_fixed" not in det
    assert sum(n in PIECES for n in det) == n_all - 6


def test_default_route_keeps_its_bits(monkeypatch):
    """Switch unset: the same bits as pieces=0 passed explicitly, and as the fixed-order fp32 route's second run."""
    monkeypatch.delenv("MIL_TM_PIECES", raising=False)
    qkv, w, dO, _, _, _ = _core_ref(512, 1.0)
    a, names = _core_gpu(qkv, w, dO, deterministic=True)
    b, _ = _core_gpu(qkv, w, dO, deterministic=True, pieces=0)
    assert not set(names) & set(PIECES)
    for k in a:
        assert F.bits_equal(a[k], b[k]), k
    with torch.no_grad():                                       # no split-K at n_pad 256: the atomic route is order-free too
        q2, w2, _, _, _, _ = _core_ref(256, 1.0)
        o0, _ = _ops().nystrom_core(q2.float().to(DEV), w2.float().to(DEV))
        o1, _ = _ops().nystrom_core(q2.float().to(DEV), w2.float().to(DEV), pieces=0)
        o3, _ = _ops().nystrom_core(q2.float().to(DEV), w2.float().to(DEV), pieces=3)
    assert F.bits_equal(o0, o1) and not F.bits_equal(o0, o3)


# --------------------------------------------------------------------------- the module
@pytest.mark.parametrize("tag", ["transmil_N7", "transmil_N250"])
def test_module_with_the_attribute_holds_the_reference_goldens(tag, golden, monkeypatch):
    """test_gpu_transmil.test_module_eval_against_reference_goldens (eval forward, BCE, backward, its tolerances) with
    gemm_pieces = 3 on the TransMIL module the test builds."""
    from mil_amd.model.dim1.TransMIL import TransMIL
    init = TransMIL.__init__

    def with_pieces(self, *a, **kw):
        init(self, *a, **kw)
        self.gemm_pieces = 3
    monkeypatch.setattr(TransMIL, "__init__", with_pieces)
    monkeypatch.delenv("MIL_TM_PIECES", raising=False)
    with F.recorded() as log:
        T.test_module_eval_against_reference_goldens(tag, golden)
    assert "mil_tm_bgemm_pieces" in {n for n, _ in log}


@pytest.mark.parametrize("N", [7, 250])
def test_module_bag_against_restatement(N):
    """test_gpu_transmil._check_bag: one bag forward and backward against the float64 restatement at its tolerances."""
    net, p = T._model()
    net.eval()
    net.gemm_pieces = 3
    x = torch.randn((N, 768), generator=torch.Generator().manual_seed(N))
    with F.recorded() as log:
        T._check_bag(net, p, x)
    assert "mil_tm_bgemm_pieces" in {n for n, _ in log}


def test_module_cls_attention_n250():
    """need_attn="cls" at N = 250 with gemm_pieces = 3: both layers' per-patch attention against the float64 restatement, per
    block, at the bound test_gpu_transmil_cls_attn holds the fp32 route to (its reference, its blocks, its k)."""
    import test_gpu_transmil_cls_attn as C
    N = 250
    x, _, ref, r32 = C._bag(N)
    net, _ = C._model()
    net.eval()
    net.gemm_pieces = 3
    with torch.no_grad(), F.recorded() as log:
        h, (a0, a1) = net(x.float().to(DEV), [N], need_attn="cls")
    assert "mil_tm_bgemm_pieces" in {n for n, _ in log}
    for layer, a in enumerate((a0[0], a1[0])):
        assert a.shape == (R.H, N)
        C.hold(f"pieces module N {N} layer {layer}", a, ref[layer], r32[layer], N, R.geometry(N)["s"])


def test_replayed_step_follows_the_flag():
    """N = 250: the stepper's graph key carries the flag (a graph captured on one arithmetic is not replayed for the other),
    and with the flag set the replayed loss equals the eager module's loss of the same seed within the 1e-4 of
    test_gpu_transmil_graph.test_replayed_training_equals_the_eager_module."""
    from mil_amd import ops, synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    N = 250
    m_r, m_e = _graph_model(21, train=True), _graph_model(21, train=True)
    m_r.extractor_pathology.gemm_pieces = m_e.extractor_pathology.gemm_pieces = 3
    m_e.extractor_pathology._drop_seed = 4321
    st = RaggedTransMILStepper(m_r, None, B=1, backward=True, drop_seed=4321)
    bce = torch.nn.BCELoss()
    x = torch.randn((N, 768), generator=torch.Generator().manual_seed(900)).to(DEV)
    y = syn.make_labels(70, 1, 2).to(DEV)
    slot = st.slot([N])
    _feed(slot, x, y)
    for i in range(3):                                          # eager visit, capture with its first replay, replay
        loss_r, _ = st.step(slot, [N])
        m_e.zero_grad(set_to_none=True)
        _, prob = m_e([x], [N])
        loss_e = bce(prob, y)
        ops.backward(loss_e)
        d = abs(st.read_loss(loss_r) - float(loss_e.detach())) / abs(float(loss_e.detach()))
        assert d <= 1e-4, (i, d)
    assert st.n_graphs == 1 and st.replays == 2 and st.eager_steps == 1
    keys = list(st.graph_bytes)
    assert len(keys) == 1 and ("gemm_pieces", 3) in keys[0]
    m_r.extractor_pathology.gemm_pieces = 0                     # the flag leaves: a new key, eager first, then its own graph
    st.step(slot, [N])
    st.step(slot, [N])
    assert st.n_graphs == 2
    keys = [k for k in st.graph_bytes if k[1] == slot.sides]
    assert len(keys) == 2 and sum(("gemm_pieces", 3) in k for k in keys) == 1
