"""GPU: the fusion model with the TransMIL aggregator over the multi-modal bag (args.fusion_transmil; model/aggregator.py,
model/dim1/TransMIL.py: flat_segments, csrc/transmil.hip: k_tm_seq_index_segs) - the index kernel against its host mirror,
the aggregator stage alone against the float64 restatement (tests/transmil_ref.py), the whole module against the fixture the
reference's own TransMIL.py made (tools/gen_golden_fusion_transmil.py) and against float64 compositions of oracle pieces,
ragged batches, the pinned refusals, the state_dict keys, the cls-token attention over the bag and the training entry."""
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import transmil_ref as R
from conftest import GOLDEN, load_golden
from test_fusion_transmil_host import INDEX_CASES, bag_segments
from test_transmil_cls_attn_host import fold_cls_row

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
DEV = torch.device("cuda:0")
TOL_H, TOL_G = 1e-4, 2e-3                    # the module's own bars (tests/test_gpu_transmil.py)
STAGE_CASES = INDEX_CASES[:7]                # without the 40-bag one


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_args(**kw):
    a = dict(modality=["pathology"], model_pathology="ABMIL", model_CI="CLIP", aggregator="TransMIL", num_classes=2,
             learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18", fusion_transmil=1, clip_layers=1)
    a.update(kw)
    return SimpleNamespace(**a)


def get_model(args):
    from mil_amd.model.utils import get_model as gm
    return gm(args)


def zero_rule(name, got, ref_norm):
    """Gradients that are zero by construction cannot be held to a relative error: softmax over ONE key (P = 1: exactly
    zero, tests/test_gpu_aggregator.py) and a constant added to every key's score (k_proj.bias: rounding noise on both sides,
    conftest.check_grad).  True if `name` is such a tensor (and it has been checked)."""
    g = torch.zeros(1) if got is None else got.detach().cpu().float()
    if ref_norm == 0.0:
        assert float(g.abs().max()) <= 1e-10, name
        return True
    if name.endswith("k_proj.bias"):
        assert float(g.abs().max()) < 5e-5, name
        return True
    if ref_norm < 1e-7:
        assert float(g.abs().max()) < 1e-6, name
        return True
    return False


# --------------------------------------------------------------------------- 1. the index kernel
@pytest.mark.parametrize("desc", INDEX_CASES, ids=lambda d: f"{len(d)}x{d[0]}")
def test_index_kernel_equals_the_host_mirror(desc):
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import segment_table, seq_index_segments
    segs, rows = bag_segments(desc)
    table, total = segment_table(segs)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    idx = ops.tm_seq_index_segs(torch.tensor(table, dtype=torch.int32, device=DEV), total, rows, flag=flag)
    want = seq_index_segments(segs, x_rows=rows)
    assert idx.dtype == torch.int32 and idx.cpu().tolist() == want
    assert int(flag) == 0
    # a table whose side does not match the rows of its first bag: flagged, still equal to the mirror, nothing out of range
    sides = [r[0] for r in table]
    sides[0] += 1
    bad, total_bad = segment_table(segs, sides)
    buf = torch.full((total_bad + 7,), 12345, dtype=torch.int32, device=DEV)
    got = ops.tm_seq_index_segs(torch.tensor(bad, dtype=torch.int32, device=DEV), total_bad, rows, idx_out=buf, flag=flag)
    assert int(flag) == 1
    assert got.cpu().tolist() == seq_index_segments(segs, sides, x_rows=rows)
    assert int(got.max()) < rows and int(got.min()) >= -2 and bool((buf[total_bad:] == 12345).all())


# --------------------------------------------------------------------------- 2. the aggregator stage alone
def _stage_model(seed=17):
    from mil_amd import synthetic as syn
    from mil_amd.model.dim1 import TransMIL
    p = syn.transmil_params(seed, 512, 2)
    net = TransMIL(n_classes=2, L=512)
    net.load_state_dict(p)
    return net.to(DEV), {k: v.double() for k, v in p.items()}


def _check_stage(net, p, x0, segs, keeps=None):
    gw = torch.randn((len(segs), 512), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    xr = x0.double().clone().requires_grad_(True)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    hs = []
    for b, bag in enumerate(segs):
        xb = torch.cat([xr[f:f + n] for f, n in bag], 0)                 # the bag's rows in sequence order
        hs.append(R.transmil(xb, pr, None if keeps is None else keeps[b])[0])
    h_ref = torch.stack(hs)
    (h_ref * gw).sum().backward()
    net.zero_grad(set_to_none=True)
    xd = x0.to(DEV).requires_grad_(True)
    h, attn = net.flat_segments(xd, segs)
    assert attn == [None, None] and tuple(h.shape) == (len(segs), 512)
    (h * gw.float().to(DEV)).sum().backward()
    worst = {"h": rel(h, h_ref), "dx0": rel(xd.grad, xr.grad)}
    for k, prm in net.named_parameters():
        if k.startswith("_fc2"):
            assert prm.grad is None
            continue
        worst[k] = rel(prm.grad, pr[k].grad)
    print("STAGE |", segs, "| train" if keeps is not None else "| eval", "| h %.2e | dx0 %.2e | worst grad %.2e (%s)" % (
        worst["h"], worst["dx0"], *max(((v, k) for k, v in worst.items() if k != "h"))))
    assert worst["h"] <= TOL_H, worst["h"]
    bad = {k: v for k, v in worst.items() if k != "h" and not v <= TOL_G}
    assert not bad, bad


@pytest.mark.parametrize("desc", STAGE_CASES, ids=lambda d: f"{len(d)}x{d[0]}")
def test_aggregator_stage_against_restatement(desc):
    net, p = _stage_model()
    segs, rows = bag_segments(desc)
    x0 = torch.randn((rows, 512), generator=torch.Generator().manual_seed(rows))
    net.eval()
    _check_stage(net, p, x0, segs)
    # train mode: the module's own Philox keep bits of one pass, then the same bits forced and restated
    net.train()
    net._drop_seed = 4321
    net.flat_segments(x0.to(DEV), segs)
    bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    assert len(bits) == len(segs)
    net.force_bits = bits
    _check_stage(net, p, x0, segs, keeps=[[R.unpack_bits(b.cpu(), 512) for b in pair] for pair in bits])


# --------------------------------------------------------------------------- 3. the whole module, eval
def _fusion_params(seed, twoway, with_ct=False, **clip):
    """Live parameters of the branch + the TransMIL aggregator's; the ABMIL aggregator's keys of fused_params stay out."""
    from mil_amd import synthetic as syn
    p = {k: v for k, v in syn.fused_params(seed, twoway, with_ct=with_ct, **clip).items() if not k.startswith("aggregator.")}
    p.update(syn.transmil_params(seed, L=512, prefix="aggregator."))
    w, b = syn.linear_params(torch.Generator().manual_seed(seed + 40), 512, 512)
    p["fc_CI.0.weight"], p["fc_CI.0.bias"] = w, b
    return p


def _load(model, p):
    have = set(model.state_dict())
    absent = {k.split(".")[0] for k in p if k not in have}
    assert absent <= {"fc_pathology", "TwoWayTransformer_Pth"}, absent       # modules a ['CI'] model does not build
    model.load_state_dict({k: v for k, v in p.items() if k in have}, strict=False)
    return model.to(DEV).eval()


def test_module_eval_against_the_reference_made_fixture():
    """tests/golden/fusion_transmil_small.npz: fused_small_clip, B = 2, lengths [7, 250], P = 1, the aggregator stage by the
    reference's own TransMIL.py in float64."""
    from mil_amd import synthetic as syn
    g = load_golden("fusion_transmil_small")
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    clip = dict(clip_layers=2, clip_width=512, clip_vocab=49408)
    p = _fusion_params(seed, "TwoWayTransformer_Pth", **clip)
    model = _load(get_model(make_args(clip_heads=8, **clip)), p)
    B = len(lengths)
    x = syn.make_bags(seed + 3, B, max(lengths), 768).to(DEV).requires_grad_(True)
    ids = syn.make_token_ids(seed + 4, B, 1).to(DEV)
    y = syn.make_labels(seed + 5, B).to(DEV)
    prob, q = model([x], ids, lengths=lengths)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    err = {"h": rel(model.last_pooled, g["h"]), "logits": rel(model.last_logits, g["logits"]),
           "loss": abs(float(loss) - float(g["loss"])) / abs(float(g["loss"])), "x_Pth2CI": rel(q, g["x_Pth2CI"])}
    print("FIXTURE |", " | ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert max(err.values()) <= TOL_H, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    grads = {"g." + k: v.grad for k, v in model.named_parameters() if k in p and not k.startswith("clinic_extractor.")
             and k.split(".")[0] != "fc_CI"}
    grads["dx"] = torch.cat([x.grad[b, :n] for b, n in enumerate(lengths)], 0)
    assert float(x.grad[0, lengths[0]:].abs().max()) == 0.0                       # padding rows: dropped, no gradient
    assert {k for k in g if k.endswith(".norm")} == {k + ".norm" for k in grads}
    bad, worst = {}, 0.0
    for k, v in grads.items():
        if k.startswith("g.aggregator._fc2"):
            assert v is None
            continue
        gn = float(g[k + ".norm"])
        if zero_rule(k, v, gn):
            continue
        e = max(abs(float(v.norm()) - gn) / gn, rel(v.flatten()[::97], g[k + ".sample"]))
        worst = max(worst, e)
        if not e <= TOL_G:
            bad[k] = e
    print(f"FIXTURE | worst grad {worst:.2e}")
    assert not bad, bad
    assert all(v.grad is None for k, v in model.named_parameters() if k.startswith(("clinic_extractor.", "extractor_pathology.")))


COMPOSED = {"pathology": dict(modality=["pathology"], P=10, n=[27], twoway="TwoWayTransformer_Pth", seed=71),
            "CI": dict(modality=["CI"], P=10, n=None, twoway="TwoWayTransformer_Pth", seed=72),
            "CT-pathology": dict(modality=["CT", "pathology"], P=1, n=[1], D=2, twoway="TwoWayTransformer_Both", seed=73)}


def _composed_inputs(c):
    from mil_amd import synthetic as syn
    seed = c["seed"]
    out = dict(ids=syn.make_token_ids(seed + 4, 1, c["P"]), y=syn.make_labels(seed + 5, 1))
    if c["n"] is not None:
        out["x"] = syn.make_bags(seed + 3, 1, c["n"][0], 768)
    if "D" in c:
        out["ct"] = torch.randn((1, c["D"], 512), generator=torch.Generator().manual_seed(seed + 6))
    return out


def _compose(c, p, inp, dtype):
    """The module's dataflow for one bag from oracle.mil_oracle pieces and transmil_ref.transmil, everything in `dtype`
    (model/aggregator.py:173,192,195 - upstream's sequence order; element 0 of TransMIL's tuple into fc).
    -> dict(h, logits, prob, loss, attn, x0, grads) with grads over every live parameter and the inputs."""
    from oracle import mil_oracle as orc
    live = [k for k in p if not k.startswith("clinic_extractor.")]
    q = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
    q.update({k: q[k].clone().requires_grad_(True) for k in live})
    lin = lambda t_, name: orc.linear_tanh(t_, q[name + ".0.weight"], q[name + ".0.bias"])      # noqa: E731
    with torch.no_grad():
        t = orc.clip_encode_text(inp["ids"][0], q, 8)
    leaves = {}
    if c["modality"] == ["CI"]:
        x0 = lin(t, "fc_CI")                                                                   # :195
    else:
        x = leaves["dx"] = inp["x"][0].to(dtype).clone().requires_grad_(True)
        xi = lin(x, "fc_pathology")
        e, f = orc.twoway_transformer(xi, orc.sinusoidal_pe(xi.shape[0], 512), lin(t, "fc_CI2Pth"), q, c["twoway"])
        if "D" in c:
            ct = leaves["dct"] = inp["ct"][0].to(dtype).clone().requires_grad_(True)
            a, c_ = orc.twoway_transformer(ct, orc.sinusoidal_pe(ct.shape[0], 512), lin(t, "fc_CI2CT"), q, c["twoway"])
            x0 = torch.cat([a, c_, e, f], 0)                                                   # :173
        else:
            x0 = torch.cat([e, f], 0)                                                          # :192
    tm = {k[len("aggregator."):]: v for k, v in q.items() if k.startswith("aggregator.")}
    h, attn = R.transmil(x0, tm, return_attn=True)
    z, prob = orc.head_forward(h.unsqueeze(0), q)
    loss = orc.bce_loss(prob, inp["y"].to(dtype))
    loss.backward()
    grads = {"g." + k: q[k].grad for k in live}
    grads.update({k: v.grad for k, v in leaves.items()})
    return dict(h=h.detach(), logits=z.detach(), prob=prob.detach(), loss=loss.detach(), attn=[a.detach() for a in attn],
                x0=x0.detach(), grads=grads)


@functools.lru_cache(maxsize=None)
def _composed(name):
    """(parameters, inputs, float64 composition, float32 composition) of one COMPOSED case; made once, never changed."""
    c = COMPOSED[name]
    p = _fusion_params(c["seed"], c["twoway"], with_ct="D" in c, clip_layers=1)
    inp = _composed_inputs(c)
    return p, inp, _compose(c, p, inp, torch.float64), _compose(c, p, inp, torch.float32)


def _run_module(name, **kw):
    c = COMPOSED[name]
    p, inp, _, _ = _composed(name)
    model = _load(get_model(make_args(modality=c["modality"], **kw)), p)
    xs, leaves = [], {}
    if "D" in c:
        leaves["dct"] = inp["ct"].to(DEV).requires_grad_(True)
        xs.append(leaves["dct"])
    if c["n"] is not None:
        leaves["dx"] = inp["x"].to(DEV).requires_grad_(True)
        xs.append(leaves["dx"])
    return model, xs, leaves, inp["ids"].to(DEV), inp["y"].to(DEV)


@pytest.mark.parametrize("name", list(COMPOSED))
def test_module_eval_against_float64_composition(name):
    """A tensor passes within the module's bar (1e-4 outputs, 2e-3 gradients) or within bound(e32, K_STAGE["module"]), e32 the
    error of the same composition in float32 on the CPU; every ratio is printed (docs/lab_notes.md keeps the table)."""
    p, _, r64, r32 = _composed(name)
    model, xs, leaves, ids, y = _run_module(name)
    out = model(xs, ids)
    prob = out[0] if isinstance(out, tuple) else out
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    k_mod = R.K_STAGE["module"]
    bad = []

    def hold(tag, got, ref, ref32, bar):
        e, e32 = rel(got, ref), rel(ref32, ref)
        print(f"RATIO | fusion_transmil | {name} | {tag} | gpu {e:.2e} | e32 {e32:.2e} | {e / max(e32, R.FLOOR):.2f}")
        if not (e <= bar or e <= R.bound(e32, k_mod)):
            bad.append((tag, e, e32))

    hold("h", model.last_pooled[0], r64["h"], r32["h"], TOL_H)
    hold("logits", model.last_logits, r64["logits"], r32["logits"], TOL_H)
    hold("loss", loss, r64["loss"], r32["loss"], TOL_H)
    assert torch.equal(prob.detach().cpu().argmax(-1), r64["prob"].argmax(-1))
    params = dict(model.named_parameters())
    for k, ref in r64["grads"].items():
        got = leaves[k].grad[0] if k in leaves else getattr(params.get(k[2:]), "grad", None)
        if k.startswith("g.aggregator._fc2") or ref is None:
            assert got is None and ref is None, k
            continue
        if zero_rule(k, got, float(ref.norm())):
            continue
        assert got is not None, k
        hold(k, got, ref, r32["grads"][k], TOL_G)
    assert not bad, bad


# --------------------------------------------------------------------------- 4. ragged batch = bags alone
def test_ragged_batch_equals_bags_alone():
    from mil_amd import synthetic as syn
    torch.manual_seed(3)
    model = get_model(make_args()).to(DEV).eval()
    lengths = [7, 250]
    x = syn.make_bags(31, 2, 250, 768).to(DEV)
    ids = syn.make_token_ids(32, 2, 1).to(DEV)
    xb = x.clone().requires_grad_(True)
    prob, _ = model([xb], ids, lengths=lengths)
    prob.sum().backward()
    for b, n in enumerate(lengths):
        xa = x[b:b + 1, :n].clone().requires_grad_(True)
        pa, _ = model([xa], ids[b:b + 1])
        pa.sum().backward()
        e_p, e_dx = rel(prob[b], pa[0]), rel(xb.grad[b, :n], xa.grad[0])
        print(f"RAGGED | bag {b} n {n} | prob {e_p:.2e} | dx {e_dx:.2e}")
        assert e_p <= 1e-6 and e_dx <= 1e-5, (b, e_p, e_dx)


# --------------------------------------------------------------------------- 5. the pin still holds
def test_without_the_flag_both_still_raise_and_bucket_is_refused():
    for kw in (dict(aggregator="TransMIL"), dict(aggregator="ABMIL", model_pathology="TransMIL")):
        args = make_args(**kw)
        del args.fusion_transmil
        with pytest.raises(NotImplementedError, match="fusion_transmil"):
            get_model(args)
        args.fusion_transmil = 0
        with pytest.raises(NotImplementedError, match="fusion_transmil"):
            get_model(args)
    model = get_model(make_args()).to(DEV).eval()
    with pytest.raises(NotImplementedError, match="bucket"):
        model([torch.zeros((64, 768), device=DEV)], None, text_features=torch.zeros((1, 1, 512), device=DEV), bucket=object())


# --------------------------------------------------------------------------- 6. state_dict keys
def test_state_dict_keys_under_both_prefixes():
    with open(os.path.join(GOLDEN, "transmil_state_dict_keys.json")) as f:
        keys = json.load(f)["keys"]
    sd = get_model(make_args(model_pathology="TransMIL", modality=["CT", "pathology"])).state_dict()
    for pre in ("aggregator.", "extractor_pathology."):
        assert [k[len(pre):] for k in sd if k.startswith(pre)] == list(keys), pre
        for k, shape in keys.items():
            want = [512, 512] if k == "_fc1.0.weight" else shape             # the fixture's extractor reads 768-wide patches
            assert list(sd[pre + k].shape) == want, (pre, k)


# --------------------------------------------------------------------------- 7. the cls token's attention over the bag
def test_last_bag_attn_is_the_folded_cls_row_patches_first():
    name = "pathology"
    c = COMPOSED[name]
    n, P = c["n"][0], c["P"]
    _, _, r64, _ = _composed(name)
    model, xs, _, ids, _ = _run_module(name)
    model.note_attn = True
    with torch.no_grad():
        prob, _ = model([xs[0].detach()], ids)
    assert len(model.last_bag_attn) == 1 and len(model.last_note_attn) == 3
    a = model.last_bag_attn[0]
    assert tuple(a.shape) == (2, 8, n + P) and a.dtype == torch.float32
    g = R.geometry(n + P)
    for layer in range(2):
        full = r64["attn"][layer]                                            # [8, n_pad, n_pad]
        seq = fold_cls_row(full, g["pad"], n + P, g["s"])                    # sequence order: the note's tokens first
        ref = torch.cat([seq[:, P:], seq[:, :P]], -1)
        e = rel(a[layer], ref)
        print(f"BAGATTN | layer {layer} | rel {e:.2e}")
        assert e <= TOL_H, (layer, e)
        # every key of the row but the cls token itself and the zero rows in front is a row of the bag
        rest = full[:, g["pad"]].sum(-1) - full[:, g["pad"], g["pad"]] - full[:, g["pad"], :g["pad"]].sum(-1)
        assert float((a[layer].double().cpu().sum(-1) - rest).abs().max()) <= TOL_H
    # off again: nothing kept, the same answer
    model.note_attn = False
    with torch.no_grad():
        prob2, _ = model([xs[0].detach()], ids)
    assert float((prob - prob2).abs().max()) <= 1e-6


# --------------------------------------------------------------------------- 8. the authors' flags
def test_train_ddp_runs_the_authors_flags(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, "train_ddp.py"), "--variant", "fusion", "--modality", "['CT','pathology']",
           "--model_pathology", "TransMIL", "--aggregator", "TransMIL", "--fusion_transmil", "1", "--loss_point", "CT-Pth-Last",
           "--train_contract", "1", "--synthetic", "[300, 768, 6]", "--ragged", "--batch_size", "1", "--n_epochs", "1",
           "--iter_per_epoch", "3", "--clip_layers", "1", "--save_dir", str(tmp_path)]
    r = subprocess.run(["timeout", "-k", "10", "500", *cmd], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch: [0]" in r.stdout and "Loss" in r.stdout and "nan" not in r.stdout.lower()
    ck = torch.load(tmp_path / "checkpoint_best.pth.tar", weights_only=True)
    assert "aggregator.layer1.attn.to_qkv.weight" in ck["state_dict"] and "extractor_pathology.cls_token" in ck["state_dict"]
