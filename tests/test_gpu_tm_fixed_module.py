"""GPU: the TransMIL step with every cross-workgroup sum in a fixed order (deterministic=True / MIL_TM_DETERMINISTIC=1 /
--deterministic 1).  The mode is held to the same references and tolerances as the atomic path (the float64 restatement, the
reference-made goldens), and two runs from the same state give the same bits: the Nystrom core, three ragged bags in train
mode, nine replayed training steps, the fusion model's aggregator.  What a step launches is read off _lib.checked().
No test here asserts that the atomic path differs between runs."""
import pytest
import torch

import tm_fixed_ref as F
import transmil_ref as R
import test_gpu_fusion_transmil as FT
import test_gpu_transmil as T
from test_gpu_transmil_graph import _feed, _model as _graph_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
rel = T.rel
FUSED = [dict(), dict(fused_a1=True), dict(fused_a3=True), dict(fused_a1=True, fused_a3=True)]     # maps, A1, A3, both


def _ops():
    from mil_amd import ops
    return ops


# --------------------------------------------------------------------------- the Nystrom core
@pytest.mark.parametrize("n_pad", [256, 512, 1280])            # no split, the smallest split (2), 5 splits
def test_nystrom_core_fixed(n_pad):
    ops = _ops()
    assert [ops._tm_splits(256, 64, 8, n) for n in (256, 512, 1280)] == [1, 2, 5]
    qkv, w, dO, pad = R.core_case(n_pad)
    ref, r32 = R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32)
    for fused in FUSED:
        runs = []
        for _ in range(2):
            qd = qkv.float().to(DEV).requires_grad_(True)
            wd = w.float().to(DEV).requires_grad_(True)
            o, attn = ops.nystrom_core(qd, wd, deterministic=True, **fused)
            assert attn is None
            o.backward(dO.float().to(DEV))
            runs.append({"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad.reshape(R.H, R.CONV)})
        got, again = runs
        for k in got:
            assert F.bits_equal(got[k], again[k]), (n_pad, fused, k)
        assert rel(got["out"], ref["out"]) < 1e-4
        assert rel(got["dqkv"], ref["dqkv"]) < 2e-3 and rel(got["dqkv"][:pad], ref["dqkv"][:pad]) < 2e-3
        assert rel(got["dw"], ref["dw"]) < 2e-3
        R.hold("core", f"fixed n_pad {n_pad} {sorted(fused)}", got, ref, r32, R.core_blocks(n_pad, pad))


def test_nystrom_core_fixed_attention_outputs():
    """need_attn True and "cls" (from the maps and from the fused passes) go with the mode: same values as with it off."""
    ops = _ops()
    N = 300
    g = R.geometry(N)
    qkv, w, _, _ = R.core_case(g["n_pad"])
    qd, wd = qkv.float().to(DEV), w.float().to(DEV)
    with torch.no_grad():
        for kw in (dict(need_attn=True), dict(need_attn="cls", pad=g["pad"], s=g["s"], n=N),
                   dict(need_attn="cls", pad=g["pad"], s=g["s"], n=N, fused_cls=True)):
            o0, a0 = ops.nystrom_core(qd, wd, deterministic=False, **kw)
            o1, a1 = ops.nystrom_core(qd, wd, deterministic=True, **kw)
            o2, a2 = ops.nystrom_core(qd, wd, deterministic=True, **kw)
            assert F.bits_equal(o1, o2) and F.bits_equal(a1, a2)
            assert rel(o1, o0) < 1e-5 and rel(a1, a0) < 1e-5, kw


# --------------------------------------------------------------------------- one bag through the module
def _check_bag(net, p, x, tol_h=1e-4, tol_g=2e-3, keeps=None):
    """test_gpu_transmil._check_bag: fwd + bwd of one bag through the module against the restatement - h, the x gradient,
    every parameter gradient, to_qkv.weight.grad by its q / k / v blocks against the float32 restatement's loss."""
    xr = x.double().clone().requires_grad_(True)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    h_ref, _ = R.transmil(xr, pr, keeps)
    gw = torch.randn(512, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (h_ref * gw).sum().backward()
    net.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    h, _ = net(xd, [x.shape[0]])
    (h[0] * gw.float().to(DEV)).sum().backward()
    assert rel(h[0], h_ref) < tol_h
    assert rel(xd.grad, xr.grad) < tol_g
    for k, prm in net.named_parameters():
        if k.startswith("_fc2"):
            assert prm.grad is None
            continue
        assert rel(prm.grad, pr[k].grad) < tol_g, (k, rel(prm.grad, pr[k].grad))
    x32 = x.float().clone().requires_grad_(True)
    p32 = {k: v.float().clone().requires_grad_(True) for k, v in p.items()}
    h32, _ = R.transmil(x32, p32, None if keeps is None else [k.float() for k in keeps])
    (h32 * gw.float()).sum().backward()
    grads = dict(net.named_parameters())
    for layer in ("layer1", "layer2"):
        k = f"{layer}.attn.to_qkv.weight"
        R.hold("module", f"fixed N {x.shape[0]} {k}", {"g": grads[k].grad}, {"g": pr[k].grad}, {"g": p32[k].grad}, {"g": R.wqkv_blocks()})


@pytest.mark.parametrize("N", [7, 300, 1000])                  # n_pad 256, 512, 1280
@pytest.mark.parametrize("fused", ["maps", "fused"])
def test_module_bag_fixed(N, fused, monkeypatch):
    if fused == "fused":
        monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
        monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    net, p = T._model()
    net.eval()
    net.deterministic = True
    x = torch.randn((N, 768), generator=torch.Generator().manual_seed(N))
    _check_bag(net, p, x)


# --------------------------------------------------------------------------- three ragged bags, train mode, twice
LENGTHS = [7, 300, 250]


def _ragged_train_grads(net, x, bits):
    net.zero_grad(set_to_none=True)
    net.force_bits = bits
    xd = x.clone().requires_grad_(True)
    h, _ = net(xd, LENGTHS)
    gw = torch.randn(h.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (h * gw).sum().backward()
    out = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    out["dx"], out["h"] = xd.grad.clone(), h.detach().clone()
    return out


@pytest.mark.parametrize("fused", ["maps", "fused"])
def test_three_ragged_bags_train_twice(fused, monkeypatch):
    """Three cls contributions, repeated rows in every bag, train mode with the keep bits forced: the whole forward and
    backward twice from the same parameters - h, the input gradient and every parameter gradient have equal bits."""
    if fused == "fused":
        monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
        monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    net, _ = T._model(seed=13)
    net.train()
    net._drop_seed = 1234
    net.deterministic = True
    x = torch.randn((sum(LENGTHS), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    net(x, LENGTHS)
    bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    a, b = _ragged_train_grads(net, x, bits), _ragged_train_grads(net, x, bits)
    assert set(a) == set(b) and len(a) > 20
    for k in a:
        assert F.bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("tag", ["transmil_ragged", "transmil_N250", "transmil_N1000"])
@pytest.mark.parametrize("fused", ["maps", "fused"])
def test_fixed_mode_holds_the_reference_goldens(tag, fused, golden, monkeypatch):
    """test_gpu_transmil.test_module_eval_against_reference_goldens with the mode on (environment switch), same tolerances."""
    monkeypatch.setenv("MIL_TM_DETERMINISTIC", "1")
    if fused == "fused":
        monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
        monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    with F.recorded() as log:
        T.test_module_eval_against_reference_goldens(tag, golden)
    names = {n for n, _ in log}
    assert "mil_tm_row_gather_bwd_fixed" in names and not names & set(F.ATOMIC)


# --------------------------------------------------------------------------- what a step launches
def _step_log(net, x, lengths):
    net.zero_grad(set_to_none=True)
    with F.recorded() as log:
        h, _ = net(x.clone().requires_grad_(True), lengths)
        h.sum().backward()
    torch.cuda.synchronize()
    return log


def test_launched_entries_follow_the_switch(monkeypatch):
    """Keyword (the module's attribute), then the environment; off: no `_fixed` entry; on: none of the atomic entries and no
    split-K mil_tm_bgemm."""
    monkeypatch.delenv("MIL_TM_DETERMINISTIC", raising=False)
    net, _ = T._model()
    net.eval()
    lengths = [300, 7]                                          # N = 300: n_pad 512, split-K products
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(2)).to(DEV)

    def is_on(log):
        names = [n for n, _ in log]
        fixed = [n for n in names if n.endswith("_fixed")]
        atomic = [n for n in names if n in F.ATOMIC] + [n for n, s in log if n == "mil_tm_bgemm" and s > 1]
        assert not (fixed and atomic), (sorted(set(fixed)), sorted(set(atomic)))
        if fixed:
            assert set(F.FIXED) <= set(names)
            assert any(n == "mil_tm_bgemm_fixed" and s > 1 for n, s in log)
        else:
            assert set(F.ATOMIC) <= set(names) and any(n == "mil_tm_bgemm" and s > 1 for n, s in log)
        return bool(fixed)

    assert net.deterministic is None
    assert is_on(_step_log(net, x, lengths)) is False           # attribute None, environment unset
    monkeypatch.setenv("MIL_TM_DETERMINISTIC", "1")
    assert is_on(_step_log(net, x, lengths)) is True            # attribute None: the environment
    net.deterministic = False
    assert is_on(_step_log(net, x, lengths)) is False           # the attribute wins over the environment
    monkeypatch.setenv("MIL_TM_DETERMINISTIC", "0")
    net.deterministic = True
    assert is_on(_step_log(net, x, lengths)) is True


# --------------------------------------------------------------------------- replayed training
SEQ = [40, 55, 70, 45, 60, 75, 49, 64, 80]                      # sides 7, 8, 9: three visits each (eager, capture, replay)


def _replayed_run():
    from mil_amd import synthetic as syn
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    model = _graph_model(21, train=True)
    model.extractor_pathology.deterministic = True
    opt = FlatAdam([p for p in model.parameters()], lr=1e-4, counted=True)
    st = RaggedTransMILStepper(model, opt, B=1, drop_seed=4321)
    losses = []
    for i, n in enumerate(SEQ):
        slot = st.slot([n])
        _feed(slot, torch.randn((n, 768), generator=torch.Generator().manual_seed(900 + i)).to(DEV), syn.make_labels(70 + i, 1, 2).to(DEV))
        loss, _ = st.step(slot, [n])
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    assert st.n_graphs == 3 and st.eager_steps == 3 and st.replays == len(SEQ) - 3    # a capture is followed by its replay
    assert all("deterministic" in k for k in st.graph_bytes)
    return torch.stack(losses), opt.flat.clone(), st, model


def test_replayed_training_twice_gives_the_same_bits():
    """Two fresh models and steppers from one seed and one drop_seed: nine steps over three sides, each side eager, captured
    and replayed.  Losses and all parameters after step 9 are equal bit for bit.  Then the flag leaves the model: the stepper
    captures a second graph for the side instead of replaying the first."""
    l1, p1, st, model = _replayed_run()
    l2, p2, _, _ = _replayed_run()
    assert bool(torch.isfinite(l1).all()) and torch.equal(l1, l2)
    assert torch.equal(p1, p2)
    from mil_amd import synthetic as syn
    model.extractor_pathology.deterministic = False
    n = SEQ[-1]
    slot = st.slot([n])
    _feed(slot, torch.randn((n, 768), generator=torch.Generator().manual_seed(7)).to(DEV), syn.make_labels(3, 1, 2).to(DEV))
    before = (st.n_graphs, st.replays, st.eager_steps)
    st.step(slot, [n])
    assert (st.n_graphs, st.replays, st.eager_steps) == (before[0], before[1], before[2] + 1)      # a new key: eager first
    st.step(slot, [n])
    assert st.n_graphs == before[0] + 1 and st.replays == before[1] + 1                            # ... then its own graph
    keys = [k for k in st.graph_bytes if k[1] == slot.sides]
    assert len(keys) == 2 and sum("deterministic" in k for k in keys) == 1


# --------------------------------------------------------------------------- the fusion model's aggregator
def _fusion_train_grads():
    from mil_amd import synthetic as syn
    g = FT.load_golden("fusion_transmil_small")
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    clip = dict(clip_layers=2, clip_width=512, clip_vocab=49408)
    torch.manual_seed(3)
    model = FT._load(FT.get_model(FT.make_args(clip_heads=8, **clip)), FT._fusion_params(seed, "TwoWayTransformer_Pth", **clip))
    for m in model.modules():                                    # what train_ddp.build_model does for --deterministic 1
        if type(m).__name__ == "TransMIL":
            m.deterministic = True
            m._drop_seed = 77
    model.train()
    B = len(lengths)
    x = syn.make_bags(seed + 3, B, max(lengths), 768).to(DEV).requires_grad_(True)
    ids = syn.make_token_ids(seed + 4, B, 1).to(DEV)
    y = syn.make_labels(seed + 5, B).to(DEV)
    with F.recorded() as log:
        prob, _ = model([x], ids, lengths=lengths)
        loss = torch.nn.BCELoss()(prob, y)
        loss.backward()
    torch.cuda.synchronize()
    out = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    out["dx"], out["loss"] = x.grad.clone(), loss.detach().clone()
    return out, log


def test_fusion_transmil_train_step_twice():
    """--fusion_transmil 1 with the model of the fusion_transmil_small fixture: one train step twice from the same state
    (fresh model, same seeds) - all gradients have equal bits, and the aggregator ran on the fixed-order entries."""
    (a, log), (b, _) = _fusion_train_grads(), _fusion_train_grads()
    names = {n for n, _ in log}
    assert "mil_tm_row_gather_bwd_fixed" in names and "mil_tm_ppeg_bwd_fixed" in names and not names & set(F.ATOMIC)
    assert set(a) == set(b) and len(a) > 20 and bool(torch.isfinite(a["loss"]))
    for k in a:
        assert F.bits_equal(a[k], b[k]), k

