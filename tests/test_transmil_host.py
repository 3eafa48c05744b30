"""CPU: TransMIL geometry, the float64 restatement (tests/transmil_ref.py) against transformers' Nystromformer attention,
the folded PPEG and its weight-gradient split, and the image-only model built with --model_pathology TransMIL."""
import argparse
import json
import os

import pytest
import torch
import torch.nn.functional as F

import transmil_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("N,s,add,seq,n_pad", [
    (1, 1, 0, 2, 256), (2, 2, 2, 5, 256), (7, 3, 2, 10, 256), (250, 16, 6, 257, 512), (1000, 32, 24, 1025, 1280),
    (2000, 45, 25, 2026, 2048), (7600, 88, 144, 7745, 7936), (15592, 125, 33, 15626, 15872),
])
def test_geometry(N, s, add, seq, n_pad):
    from mil_amd.model.dim1.TransMIL import geometry
    g = geometry(N)
    assert (g["s"], g["add"], g["seq"], g["n_pad"]) == (s, add, seq, n_pad)
    assert g["l"] == n_pad // 256 and g["pad"] == n_pad - seq
    assert g == R.geometry(N)


def test_front_pad_never_zero():
    # s^2 + 1 is never a multiple of 4, so never of 256: the first landmark always averages at least one zero row
    from mil_amd.model.dim1.TransMIL import geometry
    assert min(geometry(N)["pad"] for N in range(1, 20001)) >= 1


@pytest.mark.parametrize("n", [257, 700])   # n_pad > 256: with n_pad == 256 transformers takes exact softmax attention
def test_restatement_matches_transformers_nystromformer(n):
    tr = pytest.importorskip("transformers")
    from transformers.models.nystromformer.modeling_nystromformer import NystromformerSelfAttention
    n_pad = 256 * -(-n // 256)
    cfg = tr.NystromformerConfig(hidden_size=512, num_attention_heads=8, num_landmarks=256, segment_means_seq_len=n_pad,
                                 conv_kernel_size=33, inv_coeff_init_option=False, attention_probs_dropout_prob=0.0)
    att = NystromformerSelfAttention(cfg).double().eval()
    g = torch.Generator().manual_seed(n)
    Wqkv = torch.randn((1536, 512), generator=g, dtype=torch.float64) / 512 ** 0.5
    Wconv = torch.randn((8, 1, 33, 1), generator=g, dtype=torch.float64) / 33 ** 0.5
    with torch.no_grad():
        att.query.weight.copy_(Wqkv[:512]); att.key.weight.copy_(Wqkv[512:1024]); att.value.weight.copy_(Wqkv[1024:])
        for lin in (att.query, att.key, att.value):
            lin.bias.zero_()
        att.conv.weight.copy_(Wconv)
    x = torch.randn((n, 512), generator=g, dtype=torch.float64)
    dO = torch.randn((n, 512), generator=g, dtype=torch.float64)

    xa = x.clone().requires_grad_(True)
    xp = F.pad(xa, (0, 0, n_pad - n, 0))
    out_t = att(xp.unsqueeze(0))[0][0][-n:]
    (out_t * dO).sum().backward()
    xb = x.clone().requires_grad_(True)
    Wq = Wqkv.clone().requires_grad_(True)
    Wc = Wconv.clone().requires_grad_(True)
    o, _ = R.core(F.pad(xb, (0, 0, n_pad - n, 0)) @ Wq.t(), Wc)
    (o[-n:] * dO).sum().backward()

    def r(a, b):
        return float((a - b).norm() / b.norm())
    assert r(o[-n:].detach(), out_t.detach()) < 1e-12
    assert r(xb.grad, xa.grad) < 1e-12
    dW = torch.cat([att.query.weight.grad, att.key.weight.grad, att.value.weight.grad])
    assert r(Wq.grad, dW) < 1e-12
    assert r(Wc.grad, att.conv.weight.grad) < 1e-12


def test_ppeg_folds_into_one_7x7_and_its_weight_gradient_splits():
    g = torch.Generator().manual_seed(0)
    C, s = 16, 9
    W = {k: torch.randn((C, 1, k, k), generator=g, dtype=torch.float64, requires_grad=True) for k in (7, 5, 3)}
    b = {k: torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True) for k in (7, 5, 3)}
    x = torch.randn((1, C, s, s), generator=g, dtype=torch.float64)
    dy = torch.randn((1, C, s, s), generator=g, dtype=torch.float64)
    y3 = x + sum(F.conv2d(x, W[k], b[k], padding=k // 2, groups=C) for k in (7, 5, 3))
    (y3 * dy).sum().backward()
    delta = torch.zeros((C, 1, 7, 7), dtype=torch.float64)
    delta[:, :, 3, 3] = 1
    Wf = (W[7] + F.pad(W[5], (1, 1, 1, 1)) + F.pad(W[3], (2, 2, 2, 2)) + delta).detach().requires_grad_(True)
    bf = (b[7] + b[5] + b[3]).detach().requires_grad_(True)
    y1 = F.conv2d(x, Wf, bf, padding=3, groups=C)
    (y1 * dy).sum().backward()
    assert torch.allclose(y1, y3, atol=1e-12, rtol=0)
    assert torch.allclose(W[7].grad, Wf.grad, atol=1e-12, rtol=0)
    assert torch.allclose(W[5].grad, Wf.grad[:, :, 1:6, 1:6], atol=1e-12, rtol=0)
    assert torch.allclose(W[3].grad, Wf.grad[:, :, 2:5, 2:5], atol=1e-12, rtol=0)
    for k in (7, 5, 3):
        assert torch.allclose(b[k].grad, bf.grad, atol=1e-12, rtol=0)


def _golden_keys():
    with open(os.path.join(GOLDEN, "transmil_state_dict_keys.json")) as f:
        return json.load(f)["keys"]


def test_image_only_model_builds_with_transmil_and_matches_the_reference_keys():
    from mil_amd.model.utils_clip import get_model
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768,
                              variant="image_only")
    model = get_model(args)
    keys = {k[len("extractor_pathology."):]: list(v.shape) for k, v in model.state_dict().items()
            if k.startswith("extractor_pathology.")}
    assert keys == _golden_keys()
    assert tuple(model.fc[1].weight.shape) == (2, 512)


def test_synthetic_params_cover_the_reference_keys():
    from mil_amd import synthetic as syn
    p = syn.transmil_params(1, 768)
    assert {k: list(v.shape) for k, v in p.items()} == _golden_keys()
    assert torch.equal(p["_fc1.0.weight"], syn.transmil_params(1, 768)["_fc1.0.weight"])


def test_fused_and_graph_paths_refuse_transmil_before_gpu_work(monkeypatch):
    from mil_amd import train_ddp
    monkeypatch.setattr(train_ddp, "env_world", lambda: (1, 0, 0))
    for extra in (dict(fused_step=True, hip_graph=0), dict(fused_step=False, hip_graph=1)):
        args = argparse.Namespace(variant="image_only", model_pathology="TransMIL", multiprocessing_distributed=False, **extra)
        with pytest.raises(ValueError, match="TransMIL runs on the autograd path only"):
            train_ddp.main_worker(0, 1, args)


GOLDEN_CASES = ["transmil_N7", "transmil_N250", "transmil_N1000", "transmil_N2000", "transmil_ragged"]


def golden_bags(seed, lengths, L=768, dtype=torch.float64):
    """The bags tools/gen_golden_transmil.py fed the reference (float64 draws; the GPU test casts them)."""
    return [torch.randn((n, L), generator=torch.Generator().manual_seed(seed + 100 + i), dtype=torch.float64).to(dtype)
            for i, n in enumerate(lengths)]


@pytest.mark.parametrize("tag", GOLDEN_CASES)
def test_restatement_reproduces_the_reference_goldens(tag):
    """tests/golden/transmil_*.npz come from the reference's own TransMIL.py (tools/gen_golden_transmil.py): the wrapper
    (square padding and repeats, cls position, PPEG, norm of the cls row) and every gradient of the restatement against it."""
    from conftest import load_golden
    from mil_amd import synthetic as syn
    g = load_golden(tag)
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    p = {k: v.double().requires_grad_(True) for k, v in syn.transmil_params(seed, 768, 2).items()}
    hp = {k: v.double().requires_grad_(True) for k, v in syn.head_params(seed + 1, 512, 2).items()}
    y = syn.make_labels(seed + 7, len(lengths), 2).double()
    assert torch.equal(y, g["labels"])
    bags = [b.requires_grad_(True) for b in golden_bags(seed, lengths)]
    h = torch.stack([R.transmil(b, p)[0] for b in bags])
    z = h @ hp["fc.1.weight"].t() + hp["fc.1.bias"]
    loss = torch.nn.BCELoss()(torch.sigmoid(z), y)
    loss.backward()

    def r(a, b):
        return float((a.detach() - b).norm() / b.norm().clamp_min(1e-300))
    assert r(h, g["h"]) <= 1e-10 and r(z, g["logits"]) <= 1e-10
    assert abs(float(loss) - float(g["loss"])) <= 1e-10 * abs(float(g["loss"]))
    grads = {"extractor_pathology." + k: v.grad for k, v in p.items()}
    grads.update({k: v.grad for k, v in hp.items()})
    grads["dx"] = torch.cat([b.grad for b in bags], 0)
    for k, v in grads.items():
        name = k if k == "dx" else "g." + k
        if k.startswith("extractor_pathology._fc2"):
            assert v is None and float(g[name + ".norm"]) == 0.0, k
            continue
        assert abs(float(v.norm()) - float(g[name + ".norm"])) <= 1e-10 * float(g[name + ".norm"]), k
        assert r(v.flatten()[::97], g[name + ".sample"]) <= 1e-10, k
