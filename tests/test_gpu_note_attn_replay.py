"""GPU: `aggregator.note_attn = "all"` on the replayed evaluation - fusion_step.RaggedFusionInference (ABMIL aggregator, one
graph per capacity) and RaggedFusionTransMILStepper(backward=False) (TransMIL aggregator, one graph per capacity and grid side)
run the export's launches inside their captured body, return its capacity-shaped tensors as static outputs and slice them by
each call's host lengths after the replay.  A key is revisited with other lengths: every exported tensor equals, bit for bit,
what the same object gives without graphs on the same bag.  With the scope off keys and counts are what they were.  And the
entry point: test_ddp.py --save_note_attn DIR --note_attn_scope all with --hip_graph 1 and with --fusion_transmil_graph 1."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
CT_MAP = (512, 4, 2, 2)
D = 4


def _model(agg, modality, seed=5):
    from mil_amd.model.utils import get_model
    a = dict(modality=list(modality), model_pathology="ABMIL", model_CI="CLIP", aggregator=agg, num_classes=2, learnablePrompt=0,
             alignment_base="CI", model_CT="resnetMC3_18", clip_layers=1, fusion_transmil=int(agg == "TransMIL"))
    torch.manual_seed(seed)
    return get_model(SimpleNamespace(**a)).to(DEV).eval()


def _bag(n, seed, with_ct):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 768), generator=g).to(DEV)
    ct = torch.randn((1,) + CT_MAP, generator=g).to(DEV) if with_ct else None
    return x, ct, torch.randn((1, 1, 512), generator=g).to(DEV)


def _feed(slot, x, ct, t):
    slot.x[:x.shape[0]].copy_(x)
    if ct is not None:
        slot.ct.copy_(ct)
    slot.text.copy_(t)


def _export(m, n, with_ct, bag_shape):
    """Clones of everything the export left for the one bag of this step, shapes checked."""
    out = []
    for site in m.last_note_attn:
        assert len(site) == 1 and tuple(site[0].shape) == (8, n)
        out.append(site[0].clone())
    if with_ct:
        for site in m.last_note_attn_ct:
            assert len(site) == 1 and tuple(site[0].shape) == (8, D)
            out.append(site[0].clone())
    else:
        assert m.last_note_attn_ct is None
    assert len(m.last_bag_attn) == 1 and tuple(m.last_bag_attn[0].shape) == bag_shape
    out.append(m.last_bag_attn[0].clone())
    assert all(bool(torch.isfinite(a).all()) for a in out)
    return out


# --------------------------------------------------------------------------- 5. replay
@pytest.mark.parametrize("modality", [("pathology",), ("CT", "pathology")])
def test_inference_replay_exports_what_the_eager_bucket_forward_exports(modality):
    from mil_amd.fusion_step import RaggedFusionInference
    with_ct = "CT" in modality
    m = _model("ABMIL", modality)
    kw = dict(B=1, P=1, ct_shape=CT_MAP if with_ct else None, tower_in_graph=False)
    graphed, plain = RaggedFusionInference(m, use_graph=True, **kw), RaggedFusionInference(m, use_graph=False, **kw)
    lengths = [130, 200, 130, 190]                          # one capacity, 256 rows
    T = 2 + D if with_ct else 1
    m.note_attn = "all"
    seen = []
    for i, n in enumerate(lengths):
        bag = _bag(n, 60 + i, with_ct)
        got = []
        for inf in (graphed, plain):
            slot = inf.slot(n)
            assert slot.cap == 256
            _feed(slot, *bag)
            prob = inf.forward(slot, [n]).clone()
            got.append([prob] + _export(m, n, with_ct, (n + T,)))
        assert len(got[0]) == len(got[1]) and all(torch.equal(a, b) for a, b in zip(*got)), (i, n)
        assert abs(float(got[0][-1].sum()) - 1) < 1e-4
        seen.append(got[0])
    assert graphed.replays == 3 and graphed.eager == 1 and plain.replays == 0 and plain.eager == 4
    assert list(graphed._graphs) == [(256, "note_attn", "all")]
    # the lengths are read on the device: the replays' bags are not the captured bag
    assert not torch.equal(seen[1][1][:, :130], seen[2][1]) and not torch.equal(seen[0][1], seen[2][1])
    # scope off: the key is the capacity and the counts are what they were, beside the exporting graph
    m.note_attn = False
    m.last_note_attn = m.last_bag_attn = None
    for i, n in enumerate(lengths):
        slot = graphed.slot(n)
        _feed(slot, *_bag(n, 60 + i, with_ct))
        prob = graphed.forward(slot, [n])
        assert torch.equal(prob, seen[i][0]) and m.last_bag_attn is None and m.last_note_attn is None
    assert list(graphed._graphs) == [(256, "note_attn", "all"), 256] and graphed.replays == 6 and graphed.eager == 2


@pytest.mark.parametrize("modality", [("pathology",), ("CT", "pathology")])
def test_transmil_stepper_replay_exports_what_it_exports_without_graphs(modality):
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    with_ct = "CT" in modality
    m = _model("TransMIL", modality)
    kw = dict(B=1, backward=False, ct_shape=CT_MAP if with_ct else None)
    graphed = RaggedFusionTransMILStepper(m, None, use_graph=True, **kw)
    plain = RaggedFusionTransMILStepper(m, None, use_graph=False, **kw)
    T = 2 + D if with_ct else 1
    lengths = [n - T + 1 for n in (200, 224, 200, 196)]     # multi-modal bags of 197 .. 225 rows: one capacity, side 15
    assert len({graphed.sides([n]) for n in lengths}) == 1 and graphed.sides([lengths[0]]) == (15,)
    m.note_attn = "all"
    seen = []
    for i, n in enumerate(lengths):
        bag = _bag(n, 80 + i, with_ct)
        got = []
        for st in (graphed, plain):
            slot = st.slot(n)
            assert slot.cap == 256
            _feed(slot, *bag)
            loss, prob = st.step(slot, [n])
            st.read_loss(loss)
            got.append([prob.clone(), st.last["h"].clone()] + _export(m, n, with_ct, (2, 8, n + T)))
        assert len(got[0]) == len(got[1]) and all(torch.equal(a, b) for a, b in zip(*got)), (i, n)
        seen.append(got[0])
    assert graphed.n_graphs == 1 and graphed.eager_steps == 1 and graphed.replays == 3 and plain.replays == 0
    key_on = graphed.key(256, [lengths[0]])
    assert key_on[-2:] == ("note_attn", "all")
    assert not torch.equal(seen[0][2], seen[2][2])          # same length, another bag
    m.note_attn = False                                     # scope off: today's key, today's counts
    key_off = graphed.key(256, [lengths[0]])
    assert key_off == key_on[:-2] and "note_attn" not in key_off and "cls" not in key_off
    off = RaggedFusionTransMILStepper(m, None, use_graph=True, **kw)
    m.last_note_attn = m.last_bag_attn = None
    for i, n in enumerate(lengths):
        slot = off.slot(n)
        _feed(slot, *_bag(n, 80 + i, with_ct))
        loss, prob = off.step(slot, [n])
        assert torch.equal(prob, seen[i][0]) and m.last_bag_attn is None and m.last_note_attn is None
    assert off.n_graphs == 1 and off.eager_steps == 1 and off.replays == 3
    assert [k[0] for k in off.gs._graphs] == [key_off]


# --------------------------------------------------------------------------- 6. the entry point
TM = ["--aggregator", "TransMIL", "--fusion_transmil", "1", "--fusion_transmil_graph", "1", "--flat_adam", "1"]


@pytest.mark.parametrize("tag,extra", [("hip_graph", ["--hip_graph", "1"]), ("fusion_transmil_graph", TM)])
def test_test_ddp_saves_the_note_attention_from_the_replayed_forward(tag, extra, tmp_path):
    """test_ddp.py --save_note_attn DIR --note_attn_scope all in a child process on a checkpoint of known weights, CT + pathology:
    one <index>.npz per bag - note [3, 1, 8, N], note_ct [3, 1, 8, 160], bag [N + 162] ([2, 8, N + 162] with TransMIL), float32,
    finite - equal to what the same checkpoint leaves in this process through the eager forward."""
    from mil_amd import synthetic as syn, train_ddp
    from mil_amd.config import create_arg_parser
    from mil_amd.dataset import collate_bags, load_cohort
    tm = tag == "fusion_transmil_graph"
    argv = ["--variant", "fusion", "--modality", "['CT', 'pathology']", "--clip_layers", "1", "--synthetic", "[130, 768, 2]",
            "--test_pth", str(tmp_path), *(TM if tm else [])]
    args = create_arg_parser(argv)
    data, args.patch_dim = load_cohort(args, "test", 1)
    torch.manual_seed(78)
    model = train_ddp.build_model(args)
    torch.save({"state_dict": model.state_dict()}, tmp_path / "checkpoint_best.pth.tar")
    model = model.to(DEV).eval()
    model.graph_eval = False                                  # here: the eager forward
    model.note_attn = "all"
    here = []
    with torch.no_grad():
        for i in range(len(data)):
            b = collate_bags([data[i]])
            ct = syn.make_ct_map(args.seed + 104729 + i, 1, 160, 2).to(DEV)          # test_ddp.py's stand-in for the CT map
            model([ct, b["pathology"].to(DEV)], b["CI"].to(DEV))
            here.append((torch.stack([s[0] for s in model.last_note_attn]).cpu().numpy(),
                         torch.stack([s[0] for s in model.last_note_attn_ct]).cpu().numpy(),
                         model.last_bag_attn[0].cpu().numpy()))
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(PKG, "test_ddp.py"), *argv, "--save_note_attn", str(out), "--note_attn_scope", "all",
           *([] if tm else extra)]
    r = subprocess.run(["timeout", "-k", "10", "300", *cmd], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ACC@" in r.stdout
    assert sorted(os.listdir(out)) == [f"{i}.npz" for i in range(len(data))]
    for i in range(len(data)):
        z = np.load(out / f"{i}.npz")
        n = int(data[i]["length"])
        assert sorted(z.files) == ["bag", "note", "note_ct"]
        note, note_ct, bag = z["note"], z["note_ct"], z["bag"]
        assert note.shape == (3, 1, 8, n) and note_ct.shape == (3, 1, 8, 160)
        assert bag.shape == ((2, 8, n + 162) if tm else (n + 162,))
        assert note.dtype == note_ct.dtype == bag.dtype == np.float32
        assert np.isfinite(note).all() and np.isfinite(note_ct).all() and np.isfinite(bag).all()
        for name, got, want in (("note", note[:, 0], here[i][0]), ("note_ct", note_ct[:, 0], here[i][1]), ("bag", bag, here[i][2])):
            err = float(np.abs(got - want).max())
            print(f"ENTRY | {tag} | bag {i} | {name} | max|child - here| {err:.2e}")
            assert err <= 1e-6, (tag, i, name, err)
