"""GPU: the TransMIL module with a step's bags as one packed sequence (TransMIL.packed / MIL_TM_PACKED=1 / --tm_packed 1).  The
route is held to the reference-made golden at the tolerances of tests/test_gpu_transmil.py and launches the packed entries
only; in train mode (bags of 250, 7 and 1500 patches, forced keep bits, deterministic) it is compared with the bag-by-bag route
- the dense layers run over other row counts there and may take another kernel, so the bound is twice what the golden test
allows either route against float64, not bit-equality - and is bit-reproducible; it draws the bag-by-bag route's masks, leaves a
one-bag step and a request for attention outputs on today's launches, and is part of the stepper's graph key."""
import pytest
import torch

import tm_fixed_ref as F
import tm_packed_ref as P
import test_gpu_transmil as T
from test_gpu_transmil_graph import _feed, _model as _graph_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# test_module_eval_against_reference_goldens allows a route 1e-4 on h and 2e-3 on every gradient against float64; two routes
# may each sit that far from the truth, on opposite sides
TOL_H, TOL_G = 2 * 1e-4, 2 * 2e-3
PACKED_EVAL = tuple(n for n in P.STATUS if n != "mil_tm_resconv_bwd_packed_fixed")      # what a step on the atomic sums launches
PACKED_DET = tuple(n for n in P.STATUS if n != "mil_tm_resconv_bwd_packed")


def test_ragged_golden_on_the_packed_route(golden, monkeypatch):
    """test_gpu_transmil.test_module_eval_against_reference_goldens on transmil_ragged (bags of 7, 1000, 2000: eval forward,
    BCE, backward, its tolerances) with packed set on the TransMIL module the test builds: the packed entries ran, no
    single-bag token-side entry did, and the grouped pseudo-inverse start ran once per layer."""
    from mil_amd.model.dim1.TransMIL import TransMIL
    init = TransMIL.__init__

    def with_switch(self, *a, **kw):
        init(self, *a, **kw)
        self.packed = True
    monkeypatch.setattr(TransMIL, "__init__", with_switch)
    monkeypatch.setenv("MIL_TM_PACKED", "0")                            # the attribute wins over the environment
    with F.recorded() as log:
        T.test_module_eval_against_reference_goldens("transmil_ragged", golden)
    names = [n for n, _ in log]
    assert all(names.count(n) == 2 for n in PACKED_EVAL), {n: names.count(n) for n in PACKED_EVAL}
    assert not set(names) & set(P.SINGLE), set(names) & set(P.SINGLE)
    assert names.count("mil_tm_pinv_init_bags") == 2 and names.count("mil_tm_pinv_init_bwd_bags") == 2
    assert "mil_tm_pinv_init" not in names


def _grads(net, run, x):
    net.zero_grad(set_to_none=True)
    xd = x.clone().requires_grad_(True)
    with F.recorded() as log:
        h, attn = run(xd)
        gw = torch.randn(h.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
        (h * gw).sum().backward()
    torch.cuda.synchronize()
    out = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    out["dx"], out["h"] = xd.grad.clone(), h.detach().clone()
    return out, [n for n, _ in log], attn


def _close(tag, on, off):
    assert set(on) == set(off)
    bad = []
    for k in sorted(off):
        e = T.rel(on[k], off[k])
        print(f"RATIO | packed module | {tag} | {k} | rel {e:.2e} | bound {TOL_H if k == 'h' else TOL_G:.0e}")
        if not e <= (TOL_H if k == "h" else TOL_G):
            bad.append((k, e))
    assert not bad, (tag, bad)


def test_train_mode_against_the_bag_by_bag_route():
    """Bags of 250, 7 and 1500 patches: 1500 gives side 39 and a front pad of 14 rows, fewer than the conv's 16, so a window that
    crossed into the neighbour would reach kept rows.  Train mode, deterministic, the keep bits forced from a bag-by-bag pass."""
    lengths = [250, 7, 1500]
    net, _ = T._model(seed=13)
    net.train()
    net._drop_seed = 1234
    net.deterministic = True
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    net.packed = False
    with torch.no_grad():
        net(x, lengths)
    net.force_bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    off, names_off, _ = _grads(net, lambda xd: net(xd, lengths), x)
    net.packed = True
    on, names_on, _ = _grads(net, lambda xd: net(xd, lengths), x)
    again, _, _ = _grads(net, lambda xd: net(xd, lengths), x)
    assert all(names_on.count(n) == 2 for n in PACKED_DET) and not set(names_on) & set(P.SINGLE)
    assert not set(names_off) & set(P.NAMES) and "mil_tm_landmarks" in names_off
    assert len(off) > 20
    _close("train [250, 7, 1500]", on, off)
    for k in on:
        assert F.bits_equal(on[k], again[k]), k
    # the keep bits the packed pass reports are the forced ones, bag by bag and layer by layer
    assert all(a is b for pa, pb in zip(net.last_bits, net.force_bits) for a, b in zip(pa, pb))


def test_keep_bits_and_pass_counter_follow_the_bag_by_bag_route():
    """Train mode without forced bits: from the same seed and counter the packed pass draws the masks the bag-by-bag pass draws
    for every (bag, layer) - into the bag's rows of one buffer per layer -, and the counter advances once per pass."""
    lengths = [7, 250]
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    bits = {}
    for on in (False, True):
        net, _ = T._model(seed=13)
        net.train()
        net._drop_seed = 1234
        net.packed = on
        with torch.no_grad():
            net(x, lengths)
            first = [tuple(b.clone() for b in pair) for pair in net.last_bits]
            net(x, lengths)
        assert int(net._drop_ctr) == 2
        assert [tuple(b.shape for b in pair) for pair in net.last_bits] == [((10, 16),) * 2, ((257, 16),) * 2]
        bits[on] = (first, [tuple(b.clone() for b in pair) for pair in net.last_bits])
    for p in range(2):
        for b in range(2):
            for layer in range(2):
                assert torch.equal(bits[True][p][b][layer], bits[False][p][b][layer]), (p, b, layer)
    assert not torch.equal(bits[True][0][1][0], bits[True][1][1][0])


def test_one_bag_and_attention_outputs_keep_their_launches():
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x1 = torch.randn((250, 768), generator=torch.Generator().manual_seed(6)).to(DEV)
    x2 = torch.randn((257, 768), generator=torch.Generator().manual_seed(7)).to(DEV)
    runs = {"one bag": (x1, lambda xd: net(xd, [250])), "cls": (x2, lambda xd: net(xd, [7, 250], need_attn="cls")),
            "maps": (x2, lambda xd: net(xd, [7, 250], need_attn=True))}
    for tag, (x, run) in runs.items():
        net.packed = False
        off, names_off, _ = _grads(net, run, x)
        net.packed = True
        on, names_on, attn_on = _grads(net, run, x)
        assert names_on == names_off and not set(names_on) & set(P.NAMES), tag
        for k in off:
            assert F.bits_equal(on[k], off[k]), (tag, k)
    assert attn_on[0][1].shape == (8, 512, 512)


def test_flat_segments_against_the_bag_by_bag_route():
    """Two small bags whose rows lie in pieces, out of order in memory (the bags of tests/test_gpu_tm_bags_module.py)."""
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x = torch.randn((60, 768), generator=torch.Generator().manual_seed(8)).to(DEV)
    segs = [[(40, 9), (0, 12)], [(12, 28), (49, 11)]]
    net.packed = False
    off, _, _ = _grads(net, lambda xd: net.flat_segments(xd, segs), x)
    net.packed = True
    on, names, _ = _grads(net, lambda xd: net.flat_segments(xd, segs), x)
    assert all(names.count(n) == 2 for n in PACKED_DET) and not set(names) & set(P.SINGLE)
    _close("flat_segments", on, off)


def test_stepper_with_two_bags_per_slot():
    """RaggedTransMILStepper, B = 2, lengths [40, 250], eval-mode model with backward, deterministic: the key ends in
    ("packed",); the eager visit, the capture's replay and a further replay give the same bits (loss, h, every gradient); with
    the switch off the stepper captures a second graph for the slot instead of replaying the first."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    lengths = [40, 250]
    model = _graph_model(21)
    ex = model.extractor_pathology
    ex.deterministic, ex.packed = True, True
    st = RaggedTransMILStepper(model, None, B=2, backward=True)
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(900)).to(DEV)
    y = syn.make_labels(70, 2, 2).to(DEV)
    slot = st.slot(lengths)
    _feed(slot, x, y)
    seen = []
    for i in range(3):                                          # eager visit, capture with its first replay, replay
        with F.recorded() as log:
            loss, _ = st.step(slot, lengths)
        torch.cuda.synchronize()
        if i == 0:
            assert set(PACKED_DET) <= {n for n, _ in log} and not {n for n, _ in log} & set(P.SINGLE)
        got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
        got["loss"], got["h"] = loss.detach().clone(), slot.last["h"].clone()
        seen.append(got)
    assert st.n_graphs == 1 and st.replays == 2 and st.eager_steps == 1
    assert len(seen[0]) > 20 and bool(torch.isfinite(seen[0]["loss"]))
    for k in seen[0]:
        assert F.bits_equal(seen[0][k], seen[1][k]) and F.bits_equal(seen[0][k], seen[2][k]), k
    keys = list(st.graph_bytes)
    assert len(keys) == 1 and ("packed",) == keys[0][-1:]
    ex.packed = False                                           # the switch leaves: a new key, eager first, then its own graph
    with F.recorded() as log:
        st.step(slot, lengths)
    assert not {n for n, _ in log} & set(P.NAMES)
    st.step(slot, lengths)
    assert st.n_graphs == 2
    keys = [k for k in st.graph_bytes if k[1] == slot.sides]
    assert len(keys) == 2 and sum("packed" in k for k in keys) == 1


@pytest.mark.parametrize("branch", ["pathology", "CT-pathology"])
def test_fusion_stepper_two_bags_in_a_512_row_bucket(branch):
    """RaggedFusionTransMILStepper, B = 2, eval (the bags of test_gpu_fusion_transmil_graph's two-bag case) with `packed` set on
    the TransMIL aggregator: the packed tables come from BucketGeometry, the key ends in ("packed",), the eager visit and the
    replays launch the packed entries and agree with the host-lengths module on the bag-by-bag route at that test's bars."""
    import test_gpu_fusion_transmil_graph as G
    c = G.BRANCH[branch]
    model = G.make_model(branch).eval()
    agg = model.aggregator
    st = G.make_stepper(model, branch, B=2, backward=False)
    for i, lengths in enumerate([[c["key_a"][0], c["key_b"][0]]] * 2 + [[c["key_a"][1], c["key_b"][2]]]):
        xs, ct, t, y = G.inputs(branch, lengths, 200 + i)
        slot = st.slot(sum(lengths))
        G.feed(slot, xs, ct, t, y)
        agg.packed = True
        assert st.key(slot.cap, lengths)[-1:] == ("packed",)
        with F.recorded() as log:
            loss, prob = st.step(slot, lengths)
        st.read_loss(loss)
        names = {n for n, _ in log}
        if i == 0:                                              # the eager visit; replays launch nothing through the handle
            assert {n for n in PACKED_EVAL if "bwd" not in n} <= names and not names & set(P.SINGLE)
        prob, h = prob.clone(), st.last["h"].clone()
        agg.packed = False
        with torch.no_grad():
            p0 = G.eager_forward(model, xs, ct, t)
        e_p, e_h = G.rel(prob, p0), G.rel(h, model.last_pooled)
        print(f"RATIO | packed fusion stepper | {branch} | {lengths} | prob {e_p:.2e} | h {e_h:.2e} | bound {G.TOL_H:.0e}")
        assert e_p <= G.TOL_H and e_h <= G.TOL_H, (lengths, e_p, e_h)
    assert st.n_graphs == 1 and st.replays == 2
