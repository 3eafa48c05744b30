"""GPU: the TransMIL step replayed from hipGraphs with the bag geometry on the device (transmil_step.RaggedTransMILStepper,
csrc/transmil.hip: mil_tm_seq_index) - the index kernel against the host list, a replay on a bag length the graph was NOT
captured with against the reference's float64 goldens, replay against the eager module in train mode, stale slot rows, the
graph cap and the two entry points.  Bounds: the project's TransMIL bounds against float64 (1e-4 on h / logits / loss, 2e-3 on
gradients, test_gpu_transmil.py)."""
import argparse
import json
import os
import subprocess
import sys

import pytest
import torch

from test_transmil_host import golden_bags

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _host_list(lengths):
    import math
    idx, off = [], 0
    for n in lengths:
        s = int(math.ceil(math.sqrt(n)))
        idx += [-2] + list(range(off, off + n)) + list(range(off, off + s * s - n))
        off += n
    return idx


def _run_index(lengths, sides, guard=64):
    from mil_amd import ops
    total = sum(1 + s * s for s in sides)
    buf = torch.full((total + guard,), GUARD, device=DEV, dtype=torch.int32)
    rows = torch.full((1,), -1, device=DEV, dtype=torch.int32)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    len_dev = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    ops.tm_seq_index(len_dev, sides, buf[:total], rows, flag)
    torch.cuda.synchronize()
    return buf.cpu(), int(rows), int(flag), total


@pytest.mark.parametrize("lengths", [[1], [7], [250], [1000], [1937], [2025], [15592], [7, 1000, 250]])
def test_index_kernel_equals_the_host_list(lengths):
    from mil_amd.model.dim1.TransMIL import bucket_side
    sides = [bucket_side(n) for n in lengths]
    buf, rows, flag, total = _run_index(lengths, sides)
    assert buf[:total].tolist() == _host_list(lengths)
    assert rows == sum(lengths) and flag == 0
    assert bool((buf[total:] == GUARD).all())


@pytest.mark.parametrize("length", [3000, 5])
def test_index_kernel_clamps_an_out_of_bucket_length_and_raises_the_flag(length):
    s = 45                                                            # bucket (1936, 2025]
    buf, rows, flag, total = _run_index([length], [s])
    assert flag == 1
    assert bool((buf[total:] == GUARD).all())                         # nothing behind idx_out's extent
    body = buf[:total]
    assert int(body[0]) == -2 and int(body[1:].min()) >= 0 and int(body[1:].max()) < s * s
    assert rows == min(max(length, (s - 1) ** 2 + 1), s * s)


def test_index_entry_refuses_an_extent_that_is_too_short():
    from mil_amd import _lib, ops
    idx = torch.zeros(100, device=DEV, dtype=torch.int32)
    with pytest.raises(_lib.MilHipError):
        ops.tm_seq_index(torch.tensor([250], dtype=torch.int32, device=DEV), [16], idx)


def _model(seed, train=False):
    from mil_amd import synthetic as syn
    from mil_amd.model.utils_clip import get_model
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    model = get_model(args)
    sd = {"extractor_pathology." + k: v for k, v in syn.transmil_params(seed, 768, 2).items()}
    sd.update(syn.head_params(seed + 1, 512, 2))
    model.load_state_dict(sd)
    model = model.to(DEV)
    return model.train() if train else model.eval()


def _feed(slot, x, y=None):
    slot.x[:x.shape[0]].copy_(x)
    if y is not None:
        slot.y.copy_(y)


@pytest.mark.parametrize("tag,others", [("transmil_N2000", [1990, 1990]), ("transmil_N1000", [990, 990])])
def test_replay_on_another_length_of_the_side_matches_the_reference_goldens(tag, others, golden):
    """The graph of a side is captured on N = 1990 (990) and replayed on the golden bag of N = 2000 (1000): h, logits, loss
    and every parameter gradient of that REPLAYED step against tests/golden/transmil_*.npz (the reference's own TransMIL.py
    in float64), so the index, the true row count and the row offset really come from the length on the device."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    g = golden(tag)
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    model = _model(seed)
    st = RaggedTransMILStepper(model, None, B=1, backward=True)
    y = syn.make_labels(seed + 7, 1, 2).to(DEV)
    for i, n in enumerate(others):
        slot = st.slot([n])
        _feed(slot, torch.randn((n, 768), generator=torch.Generator().manual_seed(50 + i)).to(DEV), y)
        st.step(slot, [n])
    assert st.n_graphs == 1 and st.replays == 1 and st.eager_steps == 1
    N = lengths[0]
    slot2 = st.slot([N])
    assert slot2 is slot
    _feed(slot, golden_bags(seed, lengths)[0].float().to(DEV), y)
    loss, prob = st.step(slot, [N])
    assert st.replays == 2 and st.eager_steps == 1 and st.n_graphs == 1
    value = st.read_loss(loss)
    err = {"h": rel(slot.last["h"], g["h"]), "logits": rel(slot.last["logits"], g["logits"]),
           "loss": abs(value - float(g["loss"])) / abs(float(g["loss"]))}
    print(f"replayed golden {tag}: {err}")
    assert err["h"] <= 1e-4 and err["logits"] <= 1e-4 and err["loss"] <= 1e-4, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    worst = 0.0
    for k, v in model.named_parameters():
        if k.startswith("extractor_pathology._fc2"):
            assert v.grad is None
            continue
        k = "g." + k
        e = max(abs(float(v.grad.norm()) - float(g[k + ".norm"])) / float(g[k + ".norm"]),
                rel(v.grad.flatten()[::97], g[k + ".sample"]))
        assert e <= 2e-3, (k, e)
        worst = max(worst, e)
    print(f"replayed golden {tag}: worst grad {worst:.2e}")


SEQ = [250, 390, 1000, 240, 400, 990, 256, 380, 1024, 230, 362, 962]          # sides 16, 20, 32: four visits each

# Parameter update after the 12 steps, replayed run against eager run, ||d_replay - d_eager|| / ||d_eager||: measured once on
# the MI355X at 1.52e-5 (split-K products and the gather's atomics reorder sums; Adam's normalised step carries a gradient's
# rounding into the update).  The bound is 4 x that, 6.1e-5, capped at the 2e-3 gradient bound.
MEASURED_UPDATE_DIFF = 1.52e-5
UPDATE_BOUND = 2e-3 if MEASURED_UPDATE_DIFF is None else min(4 * MEASURED_UPDATE_DIFF, 2e-3)


def test_replayed_training_equals_the_eager_module():
    """Train mode, fixed dropout seed: the same ragged sequence (3 sides, 4 visits each) through the stepper (Adam inside the
    graphs) and through the eager module with the same counted FlatAdam.  Per step: loss within 1e-4, keep bits bit-equal.
    At the end: the parameter update p_end - p_start of the two runs, relative to its norm, within UPDATE_BOUND (measured 1.52e-5 on
    the MI355X, asserted at 4 x = 6.1e-5)."""
    from mil_amd import ops, synthetic as syn
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    m_r, m_e = _model(21, train=True), _model(21, train=True)
    m_e.extractor_pathology._drop_seed = 4321
    o_r = FlatAdam([p for p in m_r.parameters()], lr=1e-4, counted=True)
    o_e = FlatAdam([p for p in m_e.parameters()], lr=1e-4, counted=True)
    start = o_r.flat.clone()
    assert torch.equal(start, o_e.flat)
    st = RaggedTransMILStepper(m_r, o_r, B=1, drop_seed=4321)
    bce = torch.nn.BCELoss()
    worst = 0.0
    for i, n in enumerate(SEQ):
        x = torch.randn((n, 768), generator=torch.Generator().manual_seed(900 + i)).to(DEV)
        y = syn.make_labels(70 + i, 1, 2).to(DEV)
        slot = st.slot([n])
        _feed(slot, x, y)
        loss_r, _ = st.step(slot, [n])
        o_e.zero_grad()
        _, prob = m_e([x], [n])
        loss_e = bce(prob, y)
        ops.backward(loss_e)
        o_e.step()
        d = abs(st.read_loss(loss_r) - float(loss_e.detach())) / abs(float(loss_e.detach()))
        worst = max(worst, d)
        assert d <= 1e-4, (i, n, d)
        bits_e = list(m_e.extractor_pathology.last_bits[0]) + [m_e.last_mbits]
        assert len(slot.last["bits"]) == 3
        for a, b in zip(slot.last["bits"], bits_e):
            assert torch.equal(a, b), (i, n)
    assert st.n_graphs == 3 and st.eager_steps == 3 and st.replays == len(SEQ) - 3
    assert int(o_r.step_counter) == len(SEQ) == int(o_e.step_counter)
    d_r, d_e = o_r.flat - start, o_e.flat - start
    diff = rel(d_r, d_e)
    print(f"replay vs eager: worst loss diff {worst:.2e}, update diff {diff:.3e} (bound {UPDATE_BOUND:.1e})")
    assert float(d_e.norm()) > 0 and diff <= UPDATE_BOUND, diff


@pytest.mark.parametrize("N", [1990, 390])                    # _fc1 on the tall kernels / on the one-launch kernels
def test_stale_rows_behind_the_bag_do_not_reach_any_product(N):
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    model = _model(5)
    st = RaggedTransMILStepper(model, None, B=1, backward=True)
    slot = st.slot([N])
    assert slot.cap > N
    _feed(slot, torch.randn((N, 768), generator=torch.Generator().manual_seed(N)).to(DEV), syn.make_labels(3, 1, 2).to(DEV))
    for _ in range(3):
        loss, _ = st.step(slot, [N])
    assert st.replays == 2
    want = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    loss0 = st.read_loss(loss)
    slot.x[N:] = float("nan")
    loss, _ = st.step(slot, [N])
    assert st.replays == 3
    loss1 = st.read_loss(loss)
    assert loss1 == loss1 and abs(loss1 - loss0) <= 1e-6 * abs(loss0)
    assert bool(torch.isfinite(slot.x).all())                  # the step's first launch cleared the tail
    for k, v in model.named_parameters():
        if k in want:
            assert bool(torch.isfinite(v.grad).all()), k
            assert rel(v.grad, want[k]) <= 1e-6, (k, rel(v.grad, want[k]))


def test_graph_count_and_cap():
    """max_graphs=1: the second side keeps running eagerly - and trains like the eager module does."""
    from mil_amd import ops, synthetic as syn
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    m_r, m_e = _model(8), _model(8)                            # eval mode: deterministic, gradients still flow
    o_r = FlatAdam([p for p in m_r.parameters()], lr=1e-4, counted=True)
    o_e = FlatAdam([p for p in m_e.parameters()], lr=1e-4, counted=True)
    start = o_r.flat.clone()
    st = RaggedTransMILStepper(m_r, o_r, B=1, max_graphs=1)
    bce = torch.nn.BCELoss()
    seq = [250, 250, 250, 390, 390, 390, 256]
    keys = set()
    for i, n in enumerate(seq):
        x = torch.randn((n, 768), generator=torch.Generator().manual_seed(300 + i)).to(DEV)
        y = syn.make_labels(30 + i, 1, 2).to(DEV)
        slot = st.slot([n])
        keys.add(slot.sides)
        _feed(slot, x, y)
        loss_r, _ = st.step(slot, [n])
        assert st.n_graphs <= len(keys)
        o_e.zero_grad()
        loss_e = bce(m_e([x], [n])[1], y)
        ops.backward(loss_e)
        o_e.step()
        assert abs(st.read_loss(loss_r) - float(loss_e.detach())) <= 1e-4 * abs(float(loss_e.detach())), (i, n)
    assert st.n_graphs == 1 and st.eager_steps == 1 + 3 and st.replays == 3
    # the same Adam on both sides, fed gradients that each meet the 2e-3 gradient bound: the updates agree within it
    assert rel(o_r.flat - start, o_e.flat - start) <= 2e-3
    assert list(st.graph_bytes) == [("transmil-sides", (16,), False, True)]


def test_a_bad_device_length_is_reported_when_the_loss_is_read():
    from mil_amd.transmil_step import RaggedTransMILStepper
    model = _model(5)
    st = RaggedTransMILStepper(model, None, B=1, backward=False)
    slot = st.slot([250])
    slot.x.normal_()
    slot.len_dev.fill_(300)                                    # outside (225, 256]: the feed and the host disagree
    loss, _ = st.step(slot, [250], on_device=True)
    with pytest.raises(RuntimeError, match="grid side"):
        st.read_loss(loss)


def _child(cmd, limit):
    return subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, cwd=REPO)


def test_train_ddp_with_the_transmil_graph_switch(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "train_ddp.py"), "--variant", "image_only", "--model_pathology", "TransMIL",
           "--transmil_graph", "1", "--synthetic", "[300, 768, 6]", "--ragged", "--batch_size", "1", "--n_epochs", "2",
           "--iter_per_epoch", "6", "--save_dir", str(tmp_path)]
    r = _child(cmd, 500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "cohort resident in HBM" in r.stdout
    assert "Epoch: [1]" in r.stdout and "Loss" in r.stdout and "nan" not in r.stdout.lower()
    ck = torch.load(tmp_path / "checkpoint_best.pth.tar", weights_only=True)
    assert any(k.endswith("layer1.attn.to_qkv.weight") for k in ck["state_dict"])
    assert ck["optimizer"]["step"] == 12
    # the host-fed fallback: lengths copied to the slot by the loop
    r = _child(cmd + ["--resident_cohort", "0", "--save_dir", str(tmp_path / "h")], 500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "cohort resident in HBM" not in r.stdout and "nan" not in r.stdout.lower()


def test_test_ddp_predictions_with_and_without_the_switch(tmp_path):
    train = [sys.executable, os.path.join(PKG, "train_ddp.py"), "--variant", "image_only", "--model_pathology", "TransMIL",
             "--synthetic", "[300, 768, 6]", "--ragged", "--batch_size", "1", "--n_epochs", "1", "--iter_per_epoch", "2",
             "--save_dir", str(tmp_path)]
    r = _child(train, 500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    code = ("import sys, json; sys.path.insert(0, '.'); import mil_amd; from mil_amd import test_ddp; "
            "from mil_amd.config import create_arg_parser; "
            "p, _ = test_ddp.test(create_arg_parser(sys.argv[1:])); print('PREDS ' + json.dumps(p))")
    argv = ["--variant", "image_only", "--model_pathology", "TransMIL", "--synthetic", "[300, 768, 12]", "--ragged",
            "--test_pth", str(tmp_path)]
    preds = []
    for extra in ([], ["--transmil_graph", "1"]):
        r = _child([sys.executable, "-c", code, *argv, *extra], 500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("PREDS ")][-1]
        preds.append(json.loads(line[6:]))
    assert len(preds[0]) == len(preds[1]) == 12
    for a, b in zip(*preds):
        assert abs(a - b) <= 1e-4 * max(abs(a), 1e-30), (a, b)


def test_build_model_with_the_switch_replays_the_eval_forward():
    """What test_ddp.py runs per sample - model([x]) in eval mode under no_grad - on the model build_model returns with the
    switch: replayed from the side's graph from the second visit on, equal to the plain forward within the 1e-4 bound."""
    from mil_amd import train_ddp
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768,
                              variant="image_only", transmil_graph=1)
    torch.manual_seed(3)
    model = train_ddp.build_model(args).to(DEV).eval()
    assert model.graph_eval
    with torch.no_grad():
        for i, n in enumerate([250, 240, 256, 390]):
            x = torch.randn((1, n, 768), generator=torch.Generator().manual_seed(40 + i)).to(DEV)
            h, prob = model([x])
            h, prob, z = h.clone(), prob.clone(), model.last_logits.clone()
            model.graph_eval = False
            h0, prob0 = model([x])
            model.graph_eval = True
            assert rel(h, h0) <= 1e-4 and rel(prob, prob0) <= 1e-4 and rel(z, model.last_logits) <= 1e-4, (i, n)
    st = model._eval_stepper
    assert st.replays == 2 and st.eager_steps == 2 and st.n_graphs == 1
    args.transmil_graph = 0
    assert not train_ddp.build_model(args).graph_eval
