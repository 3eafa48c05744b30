"""GPU: the TransMIL module with PPEG of a step's bags as one launch set (TransMIL.packed_ppeg / MIL_TM_PACKED_PPEG=1 /
--tm_packed_ppeg 1 on top of the packed route).  Against the packed route alone everything but the PPEG parameters' gradients is
bit-equal - every bag's PPEG rows are, forwards and backwards -, those gradients (one sum over all bags, where autograd adds per-bag
totals) stay within the bound of tests/test_gpu_tm_packed_module.py against the bag-by-bag route, and the step is bit-reproducible;
the packed entries are launched once per step and no single-bag PPEG entry is; one bag, a request for attention outputs and a
module without the packed route keep their launches and bits; both steppers key, capture and replay the route."""
import pytest
import torch

import tm_fixed_ref as F
import tm_packed_ref as P
import tm_ppeg_packed_ref as Q
import test_gpu_transmil as T
from test_gpu_tm_packed_module import TOL_G, TOL_H, _close, _grads
from test_gpu_transmil_graph import _feed, _model as _graph_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _count(names, n):
    return names.count(n)


def test_train_mode_against_the_packed_and_the_bag_by_bag_route():
    """Bags of 60, 7, 70 and 250 patches: sides 8, 3, 9 and 16 - one chunk, a grid narrower than the window, a chunk and a tail,
    two chunks.  Train mode, deterministic, the keep bits forced from a bag-by-bag pass."""
    lengths = [60, 7, 70, 250]
    net, _ = T._model(seed=13)
    net.train()
    net._drop_seed = 1234
    net.deterministic = True
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    net.packed, net.packed_ppeg = False, False
    with torch.no_grad():
        net(x, lengths)
    net.force_bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    bag, names_bag, _ = _grads(net, lambda xd: net(xd, lengths), x)
    net.packed = True
    pk, names_pk, _ = _grads(net, lambda xd: net(xd, lengths), x)
    net.packed_ppeg = True
    on, names_on, _ = _grads(net, lambda xd: net(xd, lengths), x)
    again, _, _ = _grads(net, lambda xd: net(xd, lengths), x)
    assert not set(names_bag) & set(Q.NAMES) and not set(names_pk) & set(Q.NAMES)          # switch off: no new entry
    assert _count(names_pk, "mil_tm_ppeg_fwd") == 4 and _count(names_pk, "mil_tm_ppeg_bwd_fixed") == 4
    assert _count(names_on, "mil_tm_ppeg_fwd_packed") == 1 and _count(names_on, "mil_tm_ppeg_bwd_packed_fixed") == 1
    assert "mil_tm_ppeg_bwd_packed" not in names_on and not set(names_on) & set(Q.SINGLE)
    assert [n for n in names_on if n not in Q.NAMES] == [n for n in names_pk if n not in Q.SINGLE]     # nothing else moved
    assert set(on) == set(pk) == set(bag) and len(on) > 20
    pos = sorted(k for k in on if k.startswith("pos_layer."))
    assert len(pos) == 6
    for k in on:
        if k not in pos:
            assert F.bits_equal(on[k], pk[k]), k
        assert F.bits_equal(on[k], again[k]), k
    _close("train [60, 7, 70, 250], pos_layer", {k: on[k] for k in pos}, {k: bag[k] for k in pos})
    _close("train [60, 7, 70, 250]", on, bag)


def test_eval_mode_on_the_atomic_sums():
    lengths = [60, 7, 70, 250]
    net, _ = T._model(seed=13)
    net.eval()
    net.deterministic = False
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    net.packed, net.packed_ppeg = False, True
    bag, names_bag, _ = _grads(net, lambda xd: net(xd, lengths), x)
    net.packed = True
    on, names_on, _ = _grads(net, lambda xd: net(xd, lengths), x)
    assert not set(names_bag) & set(Q.NAMES)
    assert _count(names_on, "mil_tm_ppeg_fwd_packed") == 1 and _count(names_on, "mil_tm_ppeg_bwd_packed") == 1
    assert "mil_tm_ppeg_bwd_packed_fixed" not in names_on and not set(names_on) & set(Q.SINGLE)
    _close("eval [60, 7, 70, 250]", on, bag)


def test_routes_the_switch_must_not_touch():
    """One bag, the attention outputs, and a module with `packed` off: launches and bits as with the switch off."""
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x1 = torch.randn((250, 768), generator=torch.Generator().manual_seed(6)).to(DEV)
    x2 = torch.randn((257, 768), generator=torch.Generator().manual_seed(7)).to(DEV)
    runs = {"one bag": (True, x1, lambda xd: net(xd, [250])),
            "cls": (True, x2, lambda xd: net(xd, [7, 250], need_attn="cls")),
            "maps": (True, x2, lambda xd: net(xd, [7, 250], need_attn=True)),
            "packed off": (False, x2, lambda xd: net(xd, [7, 250])),
            "packed off, batched": (False, x2, lambda xd: net(xd, [7, 250]))}
    for tag, (packed, x, run) in runs.items():
        net.packed, net.batch_bags = packed, tag.endswith("batched")
        net.packed_ppeg = False
        off, names_off, _ = _grads(net, run, x)
        net.packed_ppeg = True
        on, names_on, _ = _grads(net, run, x)
        assert names_on == names_off and not set(names_on) & set(Q.NAMES + P.NAMES), tag
        for k in off:
            assert F.bits_equal(on[k], off[k]), (tag, k)


def test_the_environment_switch(monkeypatch):
    """MIL_TM_PACKED=1 alone launches what it launched; with MIL_TM_PACKED_PPEG=1 beside it the packed PPEG runs."""
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x = torch.randn((257, 768), generator=torch.Generator().manual_seed(7)).to(DEV)
    monkeypatch.setenv("MIL_TM_PACKED", "1")
    monkeypatch.delenv("MIL_TM_PACKED_PPEG", raising=False)
    alone, names_alone, _ = _grads(net, lambda xd: net(xd, [7, 250]), x)
    monkeypatch.setenv("MIL_TM_PACKED_PPEG", "1")
    both, names_both, _ = _grads(net, lambda xd: net(xd, [7, 250]), x)
    assert not set(names_alone) & set(Q.NAMES) and _count(names_alone, "mil_tm_ppeg_fwd") == 2
    assert _count(names_both, "mil_tm_ppeg_fwd_packed") == 1 and not set(names_both) & set(Q.SINGLE)
    assert F.bits_equal(alone["h"], both["h"]) and F.bits_equal(alone["dx"], both["dx"])


def test_stepper_with_two_bags_per_slot():
    """RaggedTransMILStepper, B = 2, lengths [40, 250], eval-mode model with backward, deterministic: the key ends in
    ("packed", "ppeg"); the eager visit launches the packed PPEG entries; the eager visit, the capture's replay and a further
    replay give the same bits (loss, h, every gradient); with packed_ppeg off the stepper captures a second graph."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    lengths = [40, 250]
    model = _graph_model(21)
    ex = model.extractor_pathology
    ex.deterministic, ex.packed, ex.packed_ppeg = True, True, True
    st = RaggedTransMILStepper(model, None, B=2, backward=True)
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(900)).to(DEV)
    y = syn.make_labels(70, 2, 2).to(DEV)
    slot = st.slot(lengths)
    _feed(slot, x, y)
    assert st.key(slot.sides)[-2:] == ("packed", "ppeg")
    seen = []
    for i in range(3):                                          # eager visit, capture with its first replay, replay
        with F.recorded() as log:
            loss, _ = st.step(slot, lengths)
        torch.cuda.synchronize()
        if i == 0:
            names = {n for n, _ in log}
            assert {"mil_tm_ppeg_fwd_packed", "mil_tm_ppeg_bwd_packed_fixed"} <= names and not names & set(Q.SINGLE)
        got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
        got["loss"], got["h"] = loss.detach().clone(), slot.last["h"].clone()
        seen.append(got)
    assert st.n_graphs == 1 and st.replays == 2 and st.eager_steps == 1
    assert len(seen[0]) > 20 and bool(torch.isfinite(seen[0]["loss"]))
    for k in seen[0]:
        assert F.bits_equal(seen[0][k], seen[1][k]) and F.bits_equal(seen[0][k], seen[2][k]), k
    keys = list(st.graph_bytes)
    assert len(keys) == 1 and ("packed", "ppeg") == keys[0][-2:]
    ex.packed_ppeg = False                                      # the switch leaves: a new key, eager first, then its own graph
    with F.recorded() as log:
        st.step(slot, lengths)
    names = {n for n, _ in log}
    assert not names & set(Q.NAMES) and "mil_tm_ppeg_fwd" in names
    st.step(slot, lengths)
    assert st.n_graphs == 2
    keys = [k for k in st.graph_bytes if k[1] == slot.sides]
    assert len(keys) == 2 and sum("ppeg" in k for k in keys) == 1 and all("packed" in k for k in keys)


def test_fusion_stepper_two_bags_in_a_512_row_bucket():
    """RaggedFusionTransMILStepper, B = 2, eval forward (the pathology branch of test_gpu_fusion_transmil_graph's two-bag case)
    with both switches on the TransMIL aggregator: the PPEG table comes from BucketGeometry, the key ends ("packed", "ppeg"), the
    eager visit launches the packed PPEG forward, and the results agree with the host-lengths module on the bag-by-bag route at
    that test's bar."""
    import test_gpu_fusion_transmil_graph as G
    branch = "pathology"
    c = G.BRANCH[branch]
    model = G.make_model(branch).eval()
    agg = model.aggregator
    st = G.make_stepper(model, branch, B=2, backward=False)
    for i, lengths in enumerate([[c["key_a"][0], c["key_b"][0]]] * 2 + [[c["key_a"][1], c["key_b"][2]]]):
        xs, ct, t, y = G.inputs(branch, lengths, 200 + i)
        slot = st.slot(sum(lengths))
        G.feed(slot, xs, ct, t, y)
        agg.packed, agg.packed_ppeg = True, True
        assert st.key(slot.cap, lengths)[-2:] == ("packed", "ppeg")
        with F.recorded() as log:
            loss, prob = st.step(slot, lengths)
        st.read_loss(loss)
        names = [n for n, _ in log]
        if i == 0:                                              # the eager visit; replays launch nothing through the handle
            assert _count(names, "mil_tm_ppeg_fwd_packed") == 1 and not set(names) & set(Q.SINGLE)
        prob, h = prob.clone(), st.last["h"].clone()
        agg.packed, agg.packed_ppeg = False, False
        with torch.no_grad():
            p0 = G.eager_forward(model, xs, ct, t)
        e_p, e_h = G.rel(prob, p0), G.rel(h, model.last_pooled)
        print(f"RATIO | packed ppeg fusion stepper | {branch} | {lengths} | prob {e_p:.2e} | h {e_h:.2e} | bound {G.TOL_H:.0e}")
        assert e_p <= G.TOL_H and e_h <= G.TOL_H, (lengths, e_p, e_h)
    assert st.n_graphs == 1 and st.replays == 2
