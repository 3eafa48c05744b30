"""GPU: the TransMIL module with a step's bags on the batched landmark-side chain (TransMIL.batch_bags / MIL_TM_BATCH_BAGS=1 /
--tm_batch_bags 1).  The route is held to the reference-made golden at the tolerances of tests/test_gpu_transmil.py, is
bit-equal to the bag-by-bag route under the fixed-order sums (forward, flat_segments, train mode with forced keep bits),
leaves a one-bag step and a request for attention outputs on today's launches, and is part of the stepper's graph key."""
import pytest
import torch

import tm_bags_ref as G
import tm_fixed_ref as F
import test_gpu_transmil as T
from test_gpu_transmil_graph import _feed, _model as _graph_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.mark.parametrize("on", [True, False])
def test_ragged_golden_on_either_route(on, golden, monkeypatch):
    """test_gpu_transmil.test_module_eval_against_reference_goldens on transmil_ragged (bags of 7, 1000, 2000: eval forward,
    BCE, backward, its tolerances) with batch_bags set on the TransMIL module the test builds.  Each route against the golden."""
    from mil_amd.model.dim1.TransMIL import TransMIL
    init = TransMIL.__init__

    def with_switch(self, *a, **kw):
        init(self, *a, **kw)
        self.batch_bags = on
    monkeypatch.setattr(TransMIL, "__init__", with_switch)
    monkeypatch.setenv("MIL_TM_BATCH_BAGS", "0" if on else "1")        # the attribute wins over the environment
    with F.recorded() as log:
        T.test_module_eval_against_reference_goldens("transmil_ragged", golden)
    names = [n for n, _ in log]
    if on:                                                              # two layers: the grouped start and its backward twice
        assert names.count("mil_tm_pinv_init_bags") == 2 and names.count("mil_tm_pinv_init_bwd_bags") == 2
        assert not set(names) & set(G.SINGLE)
    else:
        assert names.count("mil_tm_pinv_init") == 6 and not set(names) & set(G.NAMES)


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


@pytest.mark.parametrize("fused", ["maps", "fused"])
def test_train_mode_bits_equal_the_bag_by_bag_route(fused, monkeypatch):
    """Bags of 7 and 250, train mode, deterministic, the keep bits forced: h and the input gradient are bit-equal between the
    routes, and so are the two res_conv weight gradients (a sum of two bags' terms, order-free)."""
    if fused == "fused":
        monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
        monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    lengths = [7, 250]
    net, _ = T._model(seed=13)
    net.train()
    net._drop_seed = 1234
    net.deterministic = True
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    net.batch_bags = False
    net(x, lengths)
    net.force_bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    off, names_off, _ = _grads(net, lambda xd: net(xd, lengths), x)
    net.batch_bags = True
    on, names_on, _ = _grads(net, lambda xd: net(xd, lengths), x)
    assert "mil_tm_pinv_init_bags" in names_on and not set(names_on) & set(G.SINGLE)
    assert "mil_tm_pinv_init" in names_off and not set(names_off) & set(G.NAMES)
    assert F.bits_equal(on["h"], off["h"]) and F.bits_equal(on["dx"], off["dx"])
    for k in ("layer1.attn.res_conv.weight", "layer2.attn.res_conv.weight"):        # dw_0 + dw_1 in either order
        assert F.bits_equal(on[k], off[k]), k
    # the keep bits the batched pass reports are the forced ones, bag by bag and layer by layer
    assert all(a is b for pa, pb in zip(net.last_bits, net.force_bits) for a, b in zip(pa, pb))


def test_keep_bits_and_pass_counter_follow_the_bag_by_bag_route():
    """Train mode without forced bits: from the same seed and counter the batched pass draws the masks the bag-by-bag pass
    draws for every (bag, layer), and the counter advances once per pass."""
    lengths = [7, 250]
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    bits = {}
    for on in (False, True):
        net, _ = T._model(seed=13)
        net.train()
        net._drop_seed = 1234
        net.batch_bags = on
        with torch.no_grad():
            net(x, lengths)
            first = [tuple(b.clone() for b in pair) for pair in net.last_bits]
            net(x, lengths)
        assert int(net._drop_ctr) == 2
        bits[on] = (first, [tuple(b.clone() for b in pair) for pair in net.last_bits])
    for p in range(2):
        for b in range(2):
            for layer in range(2):
                assert torch.equal(bits[True][p][b][layer], bits[False][p][b][layer]), (p, b, layer)
    assert not torch.equal(bits[True][0][1][0], bits[True][1][1][0])


def test_one_bag_and_cls_attention_keep_their_launches():
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x1 = torch.randn((250, 768), generator=torch.Generator().manual_seed(6)).to(DEV)
    x2 = torch.randn((257, 768), generator=torch.Generator().manual_seed(7)).to(DEV)
    runs = {"one bag": (x1, lambda xd: net(xd, [250])), "cls": (x2, lambda xd: net(xd, [7, 250], need_attn="cls"))}
    for tag, (x, run) in runs.items():
        net.batch_bags = False
        off, names_off, attn_off = _grads(net, run, x)
        net.batch_bags = True
        on, names_on, attn_on = _grads(net, run, x)
        assert names_on == names_off and not set(names_on) & set(G.NAMES), tag
        for k in off:
            assert F.bits_equal(on[k], off[k]), (tag, k)
    assert attn_on[0][1].shape == (8, 250)


def test_flat_segments_bits_equal_the_bag_by_bag_route():
    """Two small bags whose rows lie in pieces, out of order in memory."""
    net, _ = T._model()
    net.eval()
    net.deterministic = True
    x = torch.randn((60, 768), generator=torch.Generator().manual_seed(8)).to(DEV)
    segs = [[(40, 9), (0, 12)], [(12, 28), (49, 11)]]
    net.batch_bags = False
    off, _, _ = _grads(net, lambda xd: net.flat_segments(xd, segs), x)
    net.batch_bags = True
    on, names, _ = _grads(net, lambda xd: net.flat_segments(xd, segs), x)
    assert names.count("mil_tm_pinv_init_bags") == 2
    assert F.bits_equal(on["h"], off["h"]) and F.bits_equal(on["dx"], off["dx"])


def test_stepper_with_two_bags_per_slot():
    """RaggedTransMILStepper, B = 2, eval-mode model with backward, deterministic: the key carries ("batch_bags",); the eager
    visit, the capture's replay and a further replay give the same bits (loss, h, every gradient); with the switch off the
    stepper captures a second graph for the slot instead of replaying the first."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    lengths = [40, 250]
    model = _graph_model(21)
    ex = model.extractor_pathology
    ex.deterministic, ex.batch_bags = True, True
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
            assert "mil_tm_pinv_init_bags" in {n for n, _ in log}
        got = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
        got["loss"], got["h"] = loss.detach().clone(), slot.last["h"].clone()
        seen.append(got)
    assert st.n_graphs == 1 and st.replays == 2 and st.eager_steps == 1
    assert len(seen[0]) > 20 and bool(torch.isfinite(seen[0]["loss"]))
    for k in seen[0]:
        assert F.bits_equal(seen[0][k], seen[1][k]) and F.bits_equal(seen[0][k], seen[2][k]), k
    keys = list(st.graph_bytes)
    assert len(keys) == 1 and ("batch_bags",) == keys[0][-1:]
    ex.batch_bags = False                                       # the switch leaves: a new key, eager first, then its own graph
    with F.recorded() as log:
        loss_off, _ = st.step(slot, lengths)
    assert not {n for n, _ in log} & set(G.NAMES)
    st.step(slot, lengths)
    assert st.n_graphs == 2
    keys = [k for k in st.graph_bytes if k[1] == slot.sides]
    assert len(keys) == 2 and sum("batch_bags" in k for k in keys) == 1
    assert F.bits_equal(loss_off.detach(), seen[0]["loss"])     # and under the fixed-order sums the two routes agree to the bit
