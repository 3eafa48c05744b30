"""GPU: `aggregator.note_attn` on the fusion module - last_note_attn against a float64 restatement of
model/sam/transformer.py's token->image attention at its three sites (tests/note_attn_ref.py), last_bag_attn against the softmax
of the aggregator's scores, the switch changing nothing else, and test_ddp.py --save_note_attn.

Bound on the weights (all <= 1): 1e-5 absolute, i.e. the fusion module's asserted logit bar (2e-5, test_gpu_aggregator.py) not
tightened beyond what a 2-block chain in float32 supports; the measured maximum is printed and recorded in docs/lab_notes.md."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import note_attn_ref as R
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
NS = [70, 130]
TOL = 1e-5
TW = "TwoWayTransformer_Pth"


def _args(**kw):
    a = dict(modality=["pathology"], model_pathology="ABMIL", model_CI="CLIP", aggregator="ABMIL", num_classes=2,
             learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18", clip_layers=1)
    a.update(kw)
    return SimpleNamespace(**a)


_CACHE = {}


def _setup(P):
    """(model, x [sum N, 768] padded batch inputs, text features, float64 weights [bag][site]): built once per P."""
    if P in _CACHE:
        return _CACHE[P]
    from mil_amd.model.utils import get_model
    torch.manual_seed(20 + P)
    model = get_model(_args()).to(DEV).eval()
    gen = torch.Generator().manual_seed(30 + P)
    x = torch.zeros((len(NS), max(NS), 768))
    for b, n in enumerate(NS):
        x[b, :n] = torch.randn((n, 768), generator=gen)
    t = torch.randn((len(NS), P, 512), generator=gen)
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items() if not k.startswith("clinic_extractor.")}
    ref = []
    for b, n in enumerate(NS):
        xi = orc.linear_tanh(x[b, :n].double(), p["fc_pathology.0.weight"], p["fc_pathology.0.bias"])
        point = orc.linear_tanh(t[b].double(), p["fc_CI2Pth.0.weight"], p["fc_CI2Pth.0.bias"])
        sites, _, _ = R.twoway_note_attention(xi, orc.sinusoidal_pe(n, 512).double(), point, p, TW)
        ref.append(sites)                                            # [bag][site] -> [H, P, n]
    _CACHE[P] = (model, x.to(DEV), t.to(DEV), ref)
    return _CACHE[P]


def _forward(model, x, t, on):
    model.note_attn = on
    with torch.no_grad():
        prob, q = model([x], None, lengths=NS, text_features=t)
    return prob.clone(), q.clone(), model.last_logits.clone()


@pytest.mark.parametrize("P", [1, 2])
def test_note_attention_equals_the_restatement(P):
    model, x, t, ref = _setup(P)
    _forward(model, x, t, True)
    assert len(model.last_note_attn) == 3 and all(len(site) == len(NS) for site in model.last_note_attn)
    top = 0.0
    for s in range(3):
        for b, n in enumerate(NS):
            got = model.last_note_attn[s][b]
            want = ref[b][s][:, 0, :] if P == 1 else ref[b][s].permute(1, 0, 2)
            assert tuple(got.shape) == ((8, n) if P == 1 else (P, 8, n))
            err = float((got.double().cpu() - want).abs().max())
            print(f"NOTE | P {P} | site {s} | bag {b} | max|got - ref64| {err:.2e} | largest weight {float(want.max()):.2e}")
            top = max(top, err)
            sums = got.double().sum(-1).cpu()
            assert float((sums - want.sum(-1)).abs().max()) <= 8 * TOL           # every head sums to (about) 1 over the patches
    print(f"NOTE | P {P} | measured maximum {top:.2e} | bound {TOL:.0e}")
    assert top <= TOL


@pytest.mark.parametrize("P", [1, 2])
def test_bag_attention_is_the_softmax_of_the_aggregators_scores(P):
    model, x, t, _ = _setup(P)
    _forward(model, x, t, True)
    scores = model.aggregator.last_scores.double().cpu()
    off, Tk = R.offsets(NS), sum(NS)
    assert len(model.last_bag_attn) == len(NS)
    for b, n in enumerate(NS):
        s = torch.cat([scores[off[b]:off[b + 1]], scores[Tk + b * P:Tk + (b + 1) * P]])      # patches first, then the tokens
        got = model.last_bag_attn[b]
        assert tuple(got.shape) == (n + P,)
        R.hold("bag_attn", f"P {P} bag {b}", got, s.softmax(0), s.float().softmax(0), R.softmax_blocks([0, n + P]))


def test_the_switch_changes_nothing_else():
    model, x, t, _ = _setup(1)
    model.last_note_attn = model.last_bag_attn = None
    off = _forward(model, x, t, False)
    assert model.last_note_attn is None and model.last_bag_attn is None
    on = _forward(model, x, t, True)
    assert model.last_note_attn is not None
    again = _forward(model, x, t, False)
    for a, b, c in zip(off, on, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    model.note_attn = True                                    # not under no_grad: nothing is kept
    model.last_note_attn = model.last_bag_attn = None
    model([x], None, lengths=NS, text_features=t)
    assert model.last_note_attn is None and model.last_bag_attn is None


def test_ct_modality_raises():
    from mil_amd.model.utils import get_model
    model = get_model(_args(modality=["CT"])).to(DEV).eval()
    model.note_attn = True
    with torch.no_grad(), pytest.raises(NotImplementedError, match="note_attn"):
        model([torch.zeros((1, 4, 512), device=DEV)], None, text_features=torch.zeros((1, 1, 512), device=DEV))


def test_image_only_abmil_leaves_the_bag_weights():
    from mil_amd.model.utils_clip import get_model
    torch.manual_seed(3)
    model = get_model(SimpleNamespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768,
                                      variant="image_only")).to(DEV).eval()
    x = torch.randn((200, 768), generator=torch.Generator().manual_seed(4)).to(DEV)      # two bags, flat rows
    with torch.no_grad():
        out0 = model([x], [70, 130])
        assert model.last_bag_attn is None
        model.note_attn = True
        out1 = model([x], [70, 130])
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])
    scores = model.extractor_pathology.last_scores.double().cpu()
    for b, (r0, n) in enumerate(((0, 70), (70, 130))):
        s = scores[r0:r0 + n]
        R.hold("bag_attn", f"image-only bag {b}", model.last_bag_attn[b], s.softmax(0), s.float().softmax(0), R.softmax_blocks([0, n]))


# --------------------------------------------------------------------------- the entry point
def test_test_ddp_saves_the_note_attention(tmp_path):
    """test_ddp.py --save_note_attn in a child process, plain and with --hip_graph 1 (which then runs the eager forward too), on
    a checkpoint of known weights: one <index>.npz per bag, note [3, 1, 8, N] and bag [N + 1], float32, equal to what the same
    model leaves in this process."""
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    from mil_amd.dataset import collate_bags, load_cohort
    argv = ["--variant", "fusion", "--modality", "['pathology']", "--clip_layers", "1", "--synthetic", "[130, 768, 2]",
            "--test_pth", str(tmp_path)]
    args = create_arg_parser(argv)
    data, args.patch_dim = load_cohort(args, "test", 1)
    torch.manual_seed(77)
    model = train_ddp.build_model(args)
    torch.save({"state_dict": model.state_dict()}, tmp_path / "checkpoint_best.pth.tar")
    model = model.to(DEV).eval()
    model.note_attn = True
    here = []
    with torch.no_grad():
        for i in range(len(data)):
            b = collate_bags([data[i]])
            model([b["pathology"].to(DEV)], b["CI"].to(DEV))
            here.append((torch.stack([s[0] for s in model.last_note_attn]).cpu().numpy(), model.last_bag_attn[0].cpu().numpy()))
    for tag, extra in (("plain", []), ("graph", ["--hip_graph", "1"])):
        out = tmp_path / tag
        cmd = [sys.executable, os.path.join(PKG, "test_ddp.py"), *argv, "--save_note_attn", str(out), *extra]
        r = subprocess.run(["timeout", "-k", "10", "300", *cmd], capture_output=True, text=True, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "ACC@" in r.stdout
        assert sorted(os.listdir(out)) == [f"{i}.npz" for i in range(len(data))]
        for i in range(len(data)):
            z = np.load(out / f"{i}.npz")
            n = int(data[i]["length"])
            note, bag = z["note"], z["bag"]
            assert note.shape == (3, 1, 8, n) and bag.shape == (n + 1,) and note.dtype == bag.dtype == np.float32
            assert np.isfinite(note).all() and np.isfinite(bag).all()
            assert float(np.abs(note[:, 0] - here[i][0]).max()) <= 1e-6, tag
            assert float(np.abs(bag - here[i][1]).max()) <= 1e-6, tag
