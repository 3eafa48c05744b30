"""GPU: TransMIL (model/dim1/TransMIL.py, csrc/transmil.hip) against the float64 restatement of tests/transmil_ref.py -
each new kernel stage, the whole extractor in eval and train mode, ragged bags, the attention maps and the training entry."""
import os
import subprocess
import sys

import pytest
import torch

import transmil_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
DEV = torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _ops():
    from mil_amd import ops
    return ops


@pytest.mark.parametrize("case", [
    # (batch, M, N, K, A transposed, B transposed)
    (8, 256, 256, 256, False, False), (8, 300, 64, 7936, True, False), (3, 77, 130, 64, False, True), (8, 256, 64, 7936, False, False),
])
def test_bgemm_strides_and_split_k(case):
    ops = _ops()
    b, M, N, K, ta, tb = case
    g = torch.Generator().manual_seed(1)
    A = torch.randn((b, K, M) if ta else (b, M, K), generator=g, dtype=torch.float64)
    B = torch.randn((b, N, K) if tb else (b, K, N), generator=g, dtype=torch.float64)
    D = torch.randn((b, M, N), generator=g, dtype=torch.float64)
    Ad, Bd, Dd = A.float().to(DEV), B.float().to(DEV), D.float().to(DEV)
    sA = (M * K, 1, M) if ta else (M * K, K, 1)
    sB = (K * N, 1, K) if tb else (K * N, N, 1)
    C = torch.empty((b, M, N), device=DEV)
    ops.tm_bgemm(Ad, sA, Bd, sB, C, (M * N, N, 1), b, M, N, K, alpha=0.5)
    ref = 0.5 * (A.transpose(1, 2) if ta else A) @ (B.transpose(1, 2) if tb else B)
    assert rel(C, ref) < 1e-5
    # epilogue: alpha A B + beta D + diag I (no split with D)
    ops.tm_bgemm(Ad, sA, Bd, sB, C, (M * N, N, 1), b, M, N, K, alpha=-1.0, beta=-7.0, diag=15.0, D=Dd)
    ref2 = -2.0 * ref - 7.0 * D + 15.0 * torch.eye(M, N, dtype=torch.float64)
    assert rel(C, ref2) < 1e-5
    # accumulate (beta = 1: the split-K path where the shape asks for it)
    C2 = Dd.clone()
    ops.tm_bgemm(Ad, sA, Bd, sB, C2, (M * N, N, 1), b, M, N, K, beta=1.0)
    assert rel(C2, 2.0 * ref + D) < 1e-5


@pytest.mark.parametrize("n_pad", [256, 512, 7936])
def test_nystrom_core_fwd_bwd(n_pad):
    ops = _ops()
    g = torch.Generator().manual_seed(n_pad)
    pad = 37 if n_pad > 256 else 3
    qkv = torch.randn((n_pad, 1536), generator=g, dtype=torch.float64)
    qkv[:pad] = 0                                                     # front zero pad, as the layer feeds it
    w = (torch.rand((8, 1, 33, 1), generator=g, dtype=torch.float64) * 2 - 1) / 33 ** 0.5
    dO = torch.randn((n_pad, 512), generator=g, dtype=torch.float64)
    dO[:pad] = 0
    qr, wr = qkv.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out, _ = R.core(qr, wr)
    out.backward(dO)
    qd, wd = qkv.float().to(DEV).requires_grad_(True), w.float().to(DEV).requires_grad_(True)
    o, attn = ops.nystrom_core(qd, wd)
    assert attn is None
    o.backward(dO.float().to(DEV))
    assert rel(o, out) < 1e-4
    assert rel(qd.grad, qr.grad) < 2e-3                  # all rows: the pad rows' q / k / v gradients too
    assert rel(qd.grad[:pad], qr.grad[:pad]) < 2e-3
    assert rel(wd.grad, wr.grad) < 2e-3
    # the same per q / k / v block, pad rows and conv halo: one norm over dqkv is a statement about dv alone (|dv| is 12 x
    # |dq| at n_pad 512 and 1760 x at 7936)
    got = {"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad.reshape(R.H, R.CONV)}
    R.hold("core", f"n_pad {n_pad}", got, R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32), R.core_blocks(n_pad, pad))


@pytest.mark.parametrize("N", [7, 250, 1000])
def test_ppeg_and_gather_fwd_bwd(N):
    ops = _ops()
    from mil_amd import synthetic as syn
    geo = R.geometry(N)
    p = {k: v.double() for k, v in syn.transmil_params(5, 768).items() if k.startswith("pos_layer")}
    g = torch.Generator().manual_seed(N)
    x = torch.randn((geo["seq"], 512), generator=g, dtype=torch.float64)
    dy = torch.randn((geo["seq"], 512), generator=g, dtype=torch.float64)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    R.ppeg(xr, geo["s"], pr).backward(dy)
    pd = {k: v.float().to(DEV).requires_grad_(True) for k, v in p.items()}
    xd = x.float().to(DEV).requires_grad_(True)
    y = ops.tm_ppeg(xd, geo["s"], *[pd["pos_layer." + n] for n in ("proj.weight", "proj.bias", "proj1.weight", "proj1.bias",
                                                                   "proj2.weight", "proj2.bias")])
    y.backward(dy.float().to(DEV))
    assert rel(y, R.ppeg(x, geo["s"], p)) < 1e-5
    assert rel(xd.grad, xr.grad) < 1e-5
    for k in p:
        assert rel(pd[k].grad, pr[k].grad) < 1e-4, k
    # cls row, border ring of width 3 and interior of the grid each on their own
    blocks = {"y": R.ppeg_blocks(geo["s"]), "dx": R.ppeg_blocks(geo["s"])}
    R.hold("ppeg", f"N {N}", {"y": y.detach(), "dx": xd.grad}, R.ppeg_run(p, x, dy, geo["s"]),
           R.ppeg_run(p, x, dy, geo["s"], torch.float32), blocks)
    # sequence assembly: [cls | tokens | first add tokens again], the repeats' gradients add
    h = torch.randn((N, 512), generator=g)
    cls = torch.randn((1, 1, 512), generator=g)
    idx = [-2] + list(range(N)) + list(range(geo["add"]))
    hd, cd = h.to(DEV).requires_grad_(True), cls.to(DEV).requires_grad_(True)
    seq = ops.tm_row_gather(hd, cd, torch.tensor(idx, dtype=torch.int32, device=DEV))
    ref = torch.cat([cls.reshape(1, -1), h, h[:geo["add"]]], 0)
    assert torch.equal(seq.cpu(), ref)
    d = torch.randn(seq.shape, generator=g)
    seq.backward(d.to(DEV))
    dh = d[1:N + 1].clone()
    dh[:geo["add"]] += d[N + 1:]
    assert rel(hd.grad, dh) < 1e-6 and rel(cd.grad.reshape(-1), d[0]) < 1e-6


def _model(seed=11, L=768, C=2):
    from mil_amd.model.dim1 import TransMIL
    from mil_amd import synthetic as syn
    p = syn.transmil_params(seed, L, C)
    net = TransMIL(n_classes=C, L=L)
    net.load_state_dict(p)
    return net.to(DEV), {k: v.double() for k, v in p.items()}


def _check_bag(net, p, x, tol_h=1e-4, tol_g=2e-3, keeps=None):
    """fwd + bwd of one bag through the module against the restatement: h, x gradient, every parameter gradient."""
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
    worst = rel(xd.grad, xr.grad)
    for k, prm in net.named_parameters():
        if k.startswith("_fc2"):
            assert prm.grad is None
            continue
        assert rel(prm.grad, pr[k].grad) < tol_g, (k, rel(prm.grad, pr[k].grad))
        worst = max(worst, rel(prm.grad, pr[k].grad))
    print(f"restatement N={x.shape[0]}: h {rel(h[0], h_ref):.2e} worst grad {worst:.2e}")
    # to_qkv.weight.grad by its q, k and v row blocks (as one tensor it is the v block's), against what the float32
    # restatement loses on the CPU
    x32 = x.float().clone().requires_grad_(True)
    p32 = {k: v.float().clone().requires_grad_(True) for k, v in p.items()}
    h32, _ = R.transmil(x32, p32, None if keeps is None else [k.float() for k in keeps])
    (h32 * gw.float()).sum().backward()
    grads = dict(net.named_parameters())
    for layer in ("layer1", "layer2"):
        k = f"{layer}.attn.to_qkv.weight"
        R.hold("module", f"N {x.shape[0]} {k}", {"g": grads[k].grad}, {"g": pr[k].grad}, {"g": p32[k].grad}, {"g": R.wqkv_blocks()})


@pytest.mark.parametrize("N", [7, 250, 1000, 2000, 1, 2, 256, 257])      # 1: s = 1; 256: add = 0; 257: the largest add
def test_module_eval_against_restatement(N):
    net, p = _model()
    net.eval()
    x = torch.randn((N, 768), generator=torch.Generator().manual_seed(N))
    _check_bag(net, p, x)


def test_module_n15592_fwd_bwd():
    net, p = _model(seed=12)
    net.eval()
    x = torch.randn((15592, 768), generator=torch.Generator().manual_seed(7))
    _check_bag(net, p, x)


def test_head_logits_and_top1_through_aggregator():
    import argparse
    from mil_amd.model.utils_clip import get_model
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    torch.manual_seed(0)
    model = get_model(args).to(DEV).eval()
    lengths = [7, 250]
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(2))
    h, prob = model([x.to(DEV)], lengths)
    assert h.shape == (2, 512) and prob.shape == (2, 2)
    p = {k.replace("extractor_pathology.", ""): v.detach().double().cpu() for k, v in model.state_dict().items()}
    Wf, bf = p["fc.1.weight"], p["fc.1.bias"]
    off = 0
    for b, n in enumerate(lengths):
        hr, _ = R.transmil(x[off:off + n].double(), p)
        off += n
        z = hr @ Wf.t() + bf
        assert rel(model.last_logits[b], z) < 1e-4
        assert int(prob[b].argmax()) == int(z.argmax())


def test_ragged_batch_equals_bags_alone():
    net, _ = _model()
    net.eval()
    lengths = [7, 1000, 2000]
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(4)).to(DEV)
    xb = x.clone().requires_grad_(True)
    h, _ = net(xb, lengths)
    h.sum().backward()
    off = 0
    for b, n in enumerate(lengths):
        xa = x[off:off + n].clone().requires_grad_(True)
        ha, _ = net(xa, [n])
        ha.sum().backward()
        assert rel(h[b], ha[0]) < 1e-6
        assert rel(xb.grad[off:off + n], xa.grad) < 1e-5
        off += n


def test_train_mode_masks_and_gradients():
    net, p = _model(seed=13)
    net.train()
    net._drop_seed = 1234
    x = torch.randn((300, 768), generator=torch.Generator().manual_seed(5))
    h1, _ = net(x.to(DEV), [300])
    bits1 = [b.clone() for b in net.last_bits[0]]
    keep = torch.cat([R.unpack_bits(b.cpu(), 512).reshape(-1) for b in bits1])
    assert abs(float(keep.mean()) - 0.9) < 0.01
    h2, _ = net(x.to(DEV), [300])                          # the pass counter moved: fresh masks
    assert not torch.equal(net.last_bits[0][0], bits1[0])
    net2, _ = _model(seed=13)
    net2.train()
    net2._drop_seed = 1234
    h3, _ = net2(x.to(DEV), [300])                         # same seed, same counter: the same masks
    assert torch.equal(net2.last_bits[0][0], bits1[0]) and torch.equal(net2.last_bits[0][1], bits1[1])
    assert rel(h3, h1) < 1e-6                               # split-K products add atomically: equal up to order
    keeps = [R.unpack_bits(b.cpu(), 512) for b in bits1]
    net.force_bits = [tuple(bits1)]
    _check_bag(net, p, x, keeps=keeps)


def test_need_attn_maps():
    net, p = _model()
    net.eval()
    x = torch.randn((250, 768), generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        h, (a0, a1) = net(x.to(DEV), [250], need_attn=True)
    _, (r0, r1) = R.transmil(x.double(), p, return_attn=True)
    assert a0.shape == (1, 8, 512, 512)                  # N = 250: seq 257, n_pad 512
    assert rel(a0[0], r0) < 1e-4 and rel(a1[0], r1) < 1e-4


def test_train_ddp_transmil_runs(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "train_ddp.py"), "--variant", "image_only", "--model_pathology", "TransMIL",
           "--synthetic", "[300, 768, 6]", "--ragged", "--batch_size", "2", "--n_epochs", "1", "--iter_per_epoch", "3",
           "--save_dir", str(tmp_path)]
    r = subprocess.run(["timeout", "-k", "10", "500", *cmd], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch: [0]" in r.stdout and "Loss" in r.stdout and "nan" not in r.stdout.lower()
    ck = torch.load(tmp_path / "checkpoint_best.pth.tar", weights_only=True)
    assert any(k.endswith("layer1.attn.to_qkv.weight") for k in ck["state_dict"])
    bad = subprocess.run(["timeout", "-k", "10", "120", *cmd, "--fused_step"], capture_output=True, text=True)
    assert bad.returncode != 0 and "TransMIL runs on the autograd path only" in bad.stdout + bad.stderr


@pytest.mark.parametrize("tag", ["transmil_N7", "transmil_N250", "transmil_N1000", "transmil_N2000", "transmil_ragged"])
def test_module_eval_against_reference_goldens(tag, golden):
    """The image-only model (aggregator_clip + TransMIL, eval mode) against tests/golden/transmil_*.npz, which the
    reference's own TransMIL.py produced in float64 (tools/gen_golden_transmil.py)."""
    import argparse
    from mil_amd import synthetic as syn
    from mil_amd.model.utils_clip import get_model
    g = golden(tag)
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    model = get_model(args)
    sd = {"extractor_pathology." + k: v for k, v in syn.transmil_params(seed, 768, 2).items()}
    sd.update(syn.head_params(seed + 1, 512, 2))
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    x = torch.cat([torch.randn((n, 768), generator=torch.Generator().manual_seed(seed + 100 + i), dtype=torch.float64)
                   for i, n in enumerate(lengths)], 0).float().to(DEV).requires_grad_(True)
    y = syn.make_labels(seed + 7, len(lengths), 2).to(DEV)
    h, prob = model([x], lengths)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    err = {"h": rel(h, g["h"]), "logits": rel(model.last_logits, g["logits"]),
           "loss": abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))}
    assert err["h"] <= 1e-4 and err["logits"] <= 1e-4 and err["loss"] <= 1e-4, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    grads = {"g." + k: v.grad for k, v in model.named_parameters()}
    grads["dx"] = x.grad
    worst = 0.0
    for k, v in grads.items():
        if k.startswith("g.extractor_pathology._fc2"):
            assert v is None
            continue
        e = max(abs(float(v.norm()) - float(g[k + ".norm"])) / float(g[k + ".norm"]), rel(v.flatten()[::97], g[k + ".sample"]))
        assert e <= 2e-3, (k, e)
        worst = max(worst, e)
    print(f"golden {tag}: h {err['h']:.2e} logits {err['logits']:.2e} loss {err['loss']:.2e} worst grad {worst:.2e}")
