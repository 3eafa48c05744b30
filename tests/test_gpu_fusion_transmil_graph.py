"""GPU: the fusion model's TransMIL-aggregator step replayed from hipGraphs (fusion_step.RaggedFusionTransMILStepper,
model/dim1/TransMIL.py: BucketGeometry / flat_bucket, csrc/transmil.hip: k_tm_seq_index_bucket) - the index kernel against its
host mirror, a graph replayed on the other lengths of its key against the eager host-lengths module, the replayed training run
against the same stepper without graphs and against the eager `fusion_transmil` path, stale rows behind a bag, bit-equal
repeats under `deterministic`, the flag raised for a bad length on the device, and both entry points.

Shapes: clip_layers = 1, one text token per bag, 256-row buckets, multi-modal bags of side 15 / 16 (n_pad 256 / 512); the CT
side is given as 6 tokens per bag, so the tail behind the patches is [1] or [1, 6, 1]."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from test_fusion_transmil_graph_host import BUCKET_CASES

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
DEV = torch.device("cuda:0")
TOL_H, TOL_G = 1e-4, 2e-3                    # the module's own bars (tests/test_gpu_fusion_transmil.py): the ceilings here

# The training step of this stepper runs on TransMIL's fixed-order sums (the stepper sets `aggregator.deterministic`): replay
# against the same stepper with use_graph=False then measures 0 in every case below - loss, masks and the update after 8 steps
# bit-equal, 14 pairs of 14 on the MI355X - and 4 x 0 is 0, so the assertion is equality.  (On the atomic sums the pathology
# branch parted by up to 8.3e-3 in the update, two runs WITHOUT graphs as well; docs/lab_notes.md, "fusion TransMIL graphs".
# That path is not offered by the stepper.)
TRAIN_SEED = 11

BRANCH = {"pathology": dict(modality=["pathology"], tail=[1], ct=None,
                            key_a=[200, 224, 196], key_b=[225, 240, 255]),
          "CT-pathology": dict(modality=["CT", "pathology"], tail=[1, 6, 1], ct=(6, 512),
                               key_a=[214, 189, 217], key_b=[218, 230, 247])}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_model(branch, seed=3, **kw):
    from mil_amd.model.utils import get_model
    a = dict(modality=BRANCH[branch]["modality"], model_pathology="ABMIL", model_CI="CLIP", aggregator="TransMIL", num_classes=2,
             learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18", fusion_transmil=1, clip_layers=1)
    a.update(kw)
    torch.manual_seed(seed)
    return get_model(SimpleNamespace(**a)).to(DEV)


def inputs(branch, lengths, seed):
    """(patch rows per bag, CT tokens [B, 6, 512] or None, text features [B, 1, 512], labels [B, 2])"""
    from mil_amd import synthetic as syn
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    xs = [torch.randn((n, 768), generator=g).to(DEV) for n in lengths]
    ct = torch.randn((B, 6, 512), generator=g).to(DEV) if BRANCH[branch]["ct"] else None
    t = torch.randn((B, 1, 512), generator=g).to(DEV)
    return xs, ct, t, syn.make_labels(seed + 1, B).to(DEV)


def feed(slot, xs, ct, t, y):
    r = 0
    for x in xs:
        slot.x[r:r + x.shape[0]].copy_(x)
        r += x.shape[0]
    if ct is not None:
        slot.ct.copy_(ct)
    slot.text.copy_(t)
    slot.y.copy_(y)


def eager_forward(model, xs, ct, t, labels=None):
    """The existing host-lengths module on the same rows."""
    lengths = [x.shape[0] for x in xs]
    pad = torch.zeros((len(xs), max(lengths), 768), device=DEV)
    for b, x in enumerate(xs):
        pad[b, :x.shape[0]] = x
    xl = [pad] if ct is None else [ct, pad]
    out = model(xl, None, lengths=lengths, text_features=t, labels=labels)
    return out[0]


def make_stepper(model, branch, opt=None, **kw):
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    return RaggedFusionTransMILStepper(model, opt, ct_shape=BRANCH[branch]["ct"], **kw)


# --------------------------------------------------------------------------- 1. the index kernel
@pytest.mark.parametrize("tail,cap,lengths", BUCKET_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_index_kernel_equals_the_host_mirror(tail, cap, lengths):
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import bucket_side, seq_index_bucket
    sides = [bucket_side(n + sum(tail)) for n in lengths]
    want = seq_index_bucket(lengths, cap, tail)
    buf = torch.full((len(want) + 9,), 12345, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = torch.zeros(len(lengths), dtype=torch.int32, device=DEV)
    got = ops.tm_seq_index_bucket(torch.tensor(lengths, dtype=torch.int32, device=DEV), cap, tail, sides, buf, L, flag)
    assert got.dtype == torch.int32 and got.cpu().tolist() == want
    assert L.cpu().tolist() == [n + sum(tail) for n in lengths] and int(flag) == 0
    assert bool((buf[len(want):] == 12345).all())


@pytest.mark.parametrize("tail,cap,sides_of,dev_lengths", [
    ([1], 256, [200], [240]),                 # above its side's bucket: 241 > 225
    ([1], 256, [225], [150]),                 # below it: 151 <= 225
    ([1, 6, 1], 256, [214], [300]),           # beyond the capacity
    ([1], 512, [200, 224], [400, 224]),       # together beyond the capacity, bag 1 behind rows that do not exist
    ([1, 6, 1], 256, [214], [-3]),
    ([1], 256, [200], [2 ** 31 - 1]),
])
def test_index_kernel_clamps_and_flags_a_bad_length(tail, cap, sides_of, dev_lengths):
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import bucket_side, seq_index_bucket
    sides = [bucket_side(n + sum(tail)) for n in sides_of]
    rows = cap + len(sides) * sum(tail)
    want = seq_index_bucket(dev_lengths, cap, tail, sides)
    buf = torch.full((len(want) + 9,), 12345, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.tm_seq_index_bucket(torch.tensor(dev_lengths, dtype=torch.int32, device=DEV), cap, tail, sides, buf, None, flag)
    assert got.cpu().tolist() == want
    assert int(got.max()) < rows and int(got.min()) >= -2 and bool((buf[len(want):] == 12345).all())
    assert int(flag) == 1


def test_a_bad_device_length_is_reported_when_the_loss_is_read():
    model = make_model("pathology").eval()
    st = make_stepper(model, "pathology", backward=False)
    xs, ct, t, y = inputs("pathology", [200], 5)
    slot = st.slot(200)
    feed(slot, xs, ct, t, y)
    slot.bucket.len_dev.fill_(240)                             # the feed and the host disagree: 241 rows on a 15 x 15 grid
    loss, _ = st.step(slot, [200], on_device=True)
    with pytest.raises(RuntimeError, match="grid side"):
        st.read_loss(loss)
    slot.bucket.len_dev.fill_(200)
    loss, _ = st.step(slot, [200], on_device=True)
    assert st.read_loss(loss) == st.read_loss(loss)            # the flag was cleared; a good step reads


# --------------------------------------------------------------------------- 2. eval: replay on the other lengths of a key
@pytest.mark.parametrize("branch", list(BRANCH))
def test_eval_replay_on_other_lengths_of_the_key_equals_the_eager_module(branch):
    c = BRANCH[branch]
    model = make_model(branch).eval()
    st = make_stepper(model, branch, backward=False)
    a, b = c["key_a"], c["key_b"]
    seq = [a[0], a[0], a[1], a[2], b[0], b[0], b[1], b[2]]
    for i, n in enumerate(seq):
        xs, ct, t, y = inputs(branch, [n], 100 + i)
        slot = st.slot(n)
        assert slot.cap == 256
        feed(slot, xs, ct, t, y)
        loss, prob = st.step(slot, [n])
        st.read_loss(loss)
        prob, h = prob.clone(), st.last["h"].clone()
        with torch.no_grad():
            p0 = eager_forward(model, xs, ct, t)
        e_p, e_h = rel(prob, p0), rel(h, model.last_pooled)
        print(f"EVAL | {branch} | n {n} | prob {e_p:.2e} | h {e_h:.2e}")
        assert e_p <= TOL_H and e_h <= TOL_H, (i, n, e_p, e_h)
    assert st.n_graphs == 2 and st.eager_steps == 2 and st.replays == 6
    assert len(st.slots) == 1 and len(st.geoms) == 2


@pytest.mark.parametrize("branch", list(BRANCH))
def test_eval_two_bags_in_a_512_row_bucket(branch):
    c = BRANCH[branch]
    model = make_model(branch).eval()
    st = make_stepper(model, branch, B=2, backward=False)
    for i, lengths in enumerate([[c["key_a"][0], c["key_b"][0]]] * 2 + [[c["key_a"][1], c["key_b"][2]]]):
        xs, ct, t, y = inputs(branch, lengths, 200 + i)
        slot = st.slot(sum(lengths))
        assert slot.cap == 512 and slot.bucket.fits(lengths)
        feed(slot, xs, ct, t, y)
        loss, prob = st.step(slot, lengths)
        st.read_loss(loss)
        assert int(slot.bucket.k_off[1]) == lengths[0] != 0
        prob, h = prob.clone(), st.last["h"].clone()
        with torch.no_grad():
            p0 = eager_forward(model, xs, ct, t)
        e_p, e_h = rel(prob, p0), rel(h, model.last_pooled)
        print(f"EVAL B=2 | {branch} | {lengths} | prob {e_p:.2e} | h {e_h:.2e}")
        assert e_p <= TOL_H and e_h <= TOL_H, (lengths, e_p, e_h)
    assert st.n_graphs == 1 and st.replays == 2


# --------------------------------------------------------------------------- 3. train: replay against the same stepper, eager
def _train_pair(branch, seq, graph_b, deterministic=None, seed=11, lr=1e-4, graph_a=True):
    """Two identical models with a counted FlatAdam each: stepper A replays, stepper B is `graph_b`.  -> per-step losses and
    bits of both, the two parameter updates."""
    from mil_amd.optim import FlatAdam
    runs = []
    for use_graph in (graph_a, graph_b):
        model = make_model(branch, seed=seed).train()
        model.aggregator.deterministic = deterministic
        opt = FlatAdam(list(model.parameters()), lr=lr, counted=True)
        start = opt.flat.clone()
        st = make_stepper(model, branch, opt, use_graph=use_graph, drop_seed=4321)
        losses, bits = [], []
        for i, n in enumerate(seq):
            xs, ct, t, y = inputs(branch, [n], 300 + i)
            slot = st.slot(n)
            feed(slot, xs, ct, t, y)
            loss, _ = st.step(slot, [n])
            losses.append(st.read_loss(loss))
            bits.append([b.clone() for b in st.last["bits"]])
        runs.append(dict(st=st, opt=opt, losses=losses, bits=bits, update=opt.flat - start))
    return runs


@pytest.mark.parametrize("branch", list(BRANCH))
def test_replayed_training_equals_the_stepper_without_graphs(branch):
    """8 steps on two keys, the length moving inside each: losses, masks and the parameter update of the replayed run against
    the same stepper with use_graph=False - bit-equal (measured difference 0; the step runs on the fixed-order sums)."""
    c = BRANCH[branch]
    a, b = c["key_a"], c["key_b"]
    seq = [a[0], b[0], a[1], b[1], a[2], b[2], a[0], b[0]]                # two keys, four visits each, the length moving
    r, e = _train_pair(branch, seq, False, seed=TRAIN_SEED)
    assert r["st"].model.aggregator.deterministic is True and e["st"].model.aggregator.deterministic is True
    assert all("deterministic" in sig[0] for sig in r["st"].gs._graphs)
    assert r["st"].n_graphs == 2 and r["st"].eager_steps == 2 and r["st"].replays == len(seq) - 2
    assert e["st"].n_graphs == 0 and e["st"].replays == 0
    assert int(r["opt"].step_counter) == len(seq) == int(e["opt"].step_counter)
    worst = 0.0
    for i, n in enumerate(seq):
        d = abs(r["losses"][i] - e["losses"][i]) / abs(e["losses"][i])
        worst = max(worst, d)
        assert len(r["bits"][i]) == 3                                     # TransMIL's two layers of the one bag, the head
        for x, y in zip(r["bits"][i], e["bits"][i]):
            assert torch.equal(x, y), (i, n)
    # the masks move from pass to pass (the device pass counter advances inside the replay)
    assert not torch.equal(r["bits"][2][2], r["bits"][6][2])
    diff = rel(r["update"], e["update"])
    print(f"TRAIN | {branch} | worst loss diff {worst:.3e} | update diff {diff:.3e}")
    assert r["losses"] == e["losses"], worst
    assert torch.equal(r["opt"].flat, e["opt"].flat) and float(e["update"].norm()) > 0, diff
    # parameters that never receive a gradient stay where they started, in both runs (Adam skips them, weight decay included)
    for run in (r, e):
        opt = run["opt"]
        names = {id(p): k for k, p in run["st"].model.named_parameters()}
        for p, off in zip(opt.params, opt.offsets):
            k = names[id(p)]
            if k.startswith(("extractor_pathology.", "aggregator._fc2.", "prompt_embedding")):
                assert float(run["update"][off:off + p.numel()].abs().max()) == 0.0, k


@pytest.mark.parametrize("branch", list(BRANCH))
def test_first_step_equals_the_eager_fusion_transmil_path(branch):
    """TransMIL's masks forced on both sides, the head in eval mode (its Dropout draws from another generator on the eager
    path): loss and every gradient of the stepper's first step against the pinned eager module."""
    from mil_amd import ops
    n = BRANCH[branch]["key_a"][0]
    xs, ct, t, y = inputs(branch, [n], 77)
    seq_rows = 1 + 15 * 15
    bits = [tuple(ops.dropout_keep_bits(seq_rows, 512, 0.1, 99, j, DEV) for j in range(2))]
    grads, losses = [], []
    for new in (True, False):
        model = make_model(branch, seed=13).eval()
        model.aggregator.train()
        model.aggregator.force_bits = bits
        if new:
            st = make_stepper(model, branch, None, backward=True, drop_seed=1)
            slot = st.slot(n)
            feed(slot, xs, ct, t, y)
            loss, _ = st.step(slot, [n])
            losses.append(st.read_loss(loss))
            assert st.eager_steps == 1 and len(st.last["bits"]) == 2          # no head bits: the head is in eval mode
        else:
            eager_forward(model, xs, ct, t, labels=y)
            ops.backward(model.last_loss)
            losses.append(float(model.last_loss.detach()))
        grads.append({k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()})
    d = abs(losses[0] - losses[1]) / abs(losses[1])
    worst, bad = 0.0, {}
    for k, ge in grads[1].items():
        gr = grads[0][k]
        if ge is None or gr is None:
            # left out of the graph on one path only: then the other side's gradient is the dense zero it stands for
            other = gr if ge is None else ge
            assert other is None or float(other.abs().max()) <= 1e-6, k
            continue
        gn = float(ge.norm())
        if gn < 1e-7 or k.endswith("k_proj.bias"):                            # zero by construction: rounding noise on both sides
            assert float(gr.abs().max()) < 5e-5, k
            continue
        e = rel(gr, ge)
        worst = max(worst, e)
        if not e <= TOL_G:
            bad[k] = e
    print(f"FIRST STEP | {branch} | loss diff {d:.2e} | worst grad {worst:.2e}")
    assert d <= TOL_H, d
    assert not bad, bad
    assert all(grads[0][k] is None for k in grads[0] if k.startswith(("extractor_pathology.", "aggregator._fc2.")))


# --------------------------------------------------------------------------- 4. stale rows, determinism
@pytest.mark.parametrize("branch", list(BRANCH))
def test_stale_rows_of_a_longer_bag_do_not_reach_the_shorter_one(branch):
    """One slot, one key: a longer bag, then a shorter one whose rows [n_short, n_long) still hold the longer bag.  The
    replayed step on the shorter bag against a fresh stepper that only ever saw it: bit-equal (fixed-order sums)."""
    c = BRANCH[branch]
    n_long, n_short = max(c["key_a"]), min(c["key_a"])                      # one key: 224 / 196, 217 / 189
    xl, ctl, tl, yl = inputs(branch, [n_long], 41)
    xs, ct, t, y = inputs(branch, [n_short], 42)
    res = []
    for stale in (True, False):
        model = make_model(branch, seed=17).eval()                            # eval mode: no masks, gradients still flow
        st = make_stepper(model, branch, None, backward=True)
        slot = st.slot(n_short)
        for k in range(3):
            if stale and k < 2:
                feed(slot, xl, ctl, tl, yl)
                st.step(slot, [n_long])
            else:
                feed(slot, xs, ct, t, y)
                loss, prob = st.step(slot, [n_short])
        assert st.replays == 2 and st.n_graphs == 1
        if stale:
            assert float(slot.x[n_short:n_long].abs().max()) > 0
        res.append(dict(loss=st.read_loss(loss), prob=prob.clone(), h=st.last["h"].clone(),
                        grads={k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    a, b = res
    assert a["grads"].keys() == b["grads"].keys()
    assert a["loss"] == b["loss"] and torch.equal(a["prob"], b["prob"]) and torch.equal(a["h"], b["h"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("deterministic", [True, False], ids=["fixed-order", "atomic"])
@pytest.mark.parametrize("tail,cap,lengths", [([1], 256, [196]), ([1, 6, 1], 256, [189]), ([1], 512, [200, 224])],
                         ids=["pathology", "CT-pathology", "two-bags"])
def test_flat_bucket_never_reads_a_row_no_bag_names(tail, cap, lengths, deterministic):
    """The trap of the padding rows, at the stage that has it: x0's rows [sum len, cap) hold NaN.  Were `_fc1` run over all of
    x0, its weight gradient would multiply those rows by their zero gradient rows, 0 x NaN; gathered first, no product reads
    them.  h and every gradient are finite and equal (bit-equal on the fixed-order sums) to those of the same x0 with zeros
    there, and the gradient rows of x0 that no bag names are exactly zero."""
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.model.dim1.TransMIL import BucketGeometry, bucket_side
    torch.manual_seed(5)
    net = TransMIL(n_classes=2, L=512).to(DEV).eval()
    net.deterministic = deterministic
    B, R = len(lengths), sum(lengths)
    geom = BucketGeometry(cap, tail, [bucket_side(n + sum(tail)) for n in lengths], DEV)
    len_dev = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    base = torch.randn((geom.x_rows, 512), generator=torch.Generator().manual_seed(9)).to(DEV)
    gw = torch.randn((B, 512), generator=torch.Generator().manual_seed(10)).to(DEV)
    out = []
    for fill in (0.0, float("nan")):
        x0 = base.clone()
        x0[R:cap] = fill
        x0.requires_grad_(True)
        net.zero_grad(set_to_none=True)
        h, _ = net.flat_bucket(x0, geom, len_dev)
        (h * gw).sum().backward()
        assert int(geom.flag) == 0
        out.append(dict(h=h.detach().clone(), dx=x0.grad.clone(),
                        grads={k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    z, n = out
    assert bool(torch.isfinite(n["h"]).all()) and bool(torch.isfinite(n["dx"]).all())
    assert float(n["dx"][R:cap].abs().max()) == 0.0 and float(z["dx"][R:cap].abs().max()) == 0.0
    assert float(n["dx"][:R].abs().max()) > 0 and float(n["dx"][cap:].abs().max()) > 0
    assert torch.equal(n["h"], z["h"]) and "_fc1.0.weight" in n["grads"]
    for k, g in n["grads"].items():
        assert bool(torch.isfinite(g).all()), k
        if deterministic:
            assert torch.equal(g, z["grads"][k]), k
        else:
            assert rel(g, z["grads"][k]) <= 1e-5, (k, rel(g, z["grads"][k]))     # the same sums, atomics in another order


def test_two_replayed_runs_from_one_seed_give_the_same_bits():
    branch = "CT-pathology"
    c = BRANCH[branch]
    seq = [c["key_a"][0], c["key_a"][1], c["key_b"][0], c["key_a"][2], c["key_b"][1], c["key_a"][0]]
    r1, r2 = _train_pair(branch, seq, True)
    assert r1["st"].replays == r2["st"].replays == 4 and r1["st"].n_graphs == 2
    assert r1["losses"] == r2["losses"]
    assert torch.equal(r1["opt"].flat, r2["opt"].flat) and float(r1["update"].norm()) > 0


# --------------------------------------------------------------------------- 5. the entry points
def _child(cmd, limit):
    return subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, cwd=REPO)


FLAGS = ["--variant", "fusion", "--modality", "['CT','pathology']", "--model_pathology", "TransMIL", "--aggregator", "TransMIL",
         "--fusion_transmil", "1", "--loss_point", "CT-Pth-Last", "--train_contract", "1", "--synthetic", "[300, 768, 6]",
         "--ragged", "--batch_size", "1", "--clip_layers", "1"]


def test_entry_points_with_the_switch(tmp_path):
    train = [sys.executable, os.path.join(PKG, "train_ddp.py"), *FLAGS, "--fusion_transmil_graph", "1", "--n_epochs", "2",
             "--iter_per_epoch", "6", "--patch_keep", "1.0", "--augmentation", "0", "--save_dir", str(tmp_path)]
    r = _child(train, 500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Epoch: [1]" in r.stdout and "Loss" in r.stdout and "nan" not in r.stdout.lower()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("fusion TransMIL graphs")][-1]
    assert int(line.split("replays")[1].split()[0]) > 0, line
    ck = torch.load(tmp_path / "checkpoint_best.pth.tar", weights_only=True)
    assert "aggregator.layer1.attn.to_qkv.weight" in ck["state_dict"] and ck["optimizer"]["step"] == 12
    # test_ddp.py: the replayed per-bag forward against its eager output, from that checkpoint
    code = ("import sys, json; sys.path.insert(0, '.'); import mil_amd; from mil_amd import test_ddp; "
            "from mil_amd.config import create_arg_parser; "
            "p, _ = test_ddp.test(create_arg_parser(sys.argv[1:])); print('PREDS ' + json.dumps(p))")
    # twelve bags of ONE length: every bag after the first visits the same key, so the forward is replayed
    argv = [a for a in FLAGS if a != "--ragged"] + ["--synthetic", "[300, 768, 12]", "--test_pth", str(tmp_path)]
    preds = []
    for extra in ([], ["--fusion_transmil_graph", "1"]):
        r = _child([sys.executable, "-c", code, *argv, *extra], 500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        preds.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("PREDS ")][-1][6:]))
    assert len(preds[0]) == len(preds[1]) == 12
    for a, b in zip(*preds):
        assert abs(a - b) <= TOL_H * max(abs(a), 1e-30), (a, b)


@pytest.mark.parametrize("branch", list(BRANCH))
def test_build_model_with_the_switch_replays_the_eval_forward(branch):
    """What test_ddp.py runs per bag - model([ct,] x, ids) in eval mode under no_grad - on the model build_model returns with
    the switch: replayed from the key's graph from the second visit on, the module's own tuple, equal to the plain forward
    within the module's bar."""
    from mil_amd import synthetic as syn, train_ddp
    from mil_amd.config import create_arg_parser
    argv = ["--variant", "fusion", "--aggregator", "TransMIL", "--fusion_transmil", "1", "--clip_layers", "1",
            "--modality", str(BRANCH[branch]["modality"])]
    args = create_arg_parser(argv + ["--fusion_transmil_graph", "1"])
    torch.manual_seed(3)
    model = train_ddp.build_model(args).to(DEV).eval()
    assert model.graph_eval
    c = BRANCH[branch]
    with torch.no_grad():
        for i, n in enumerate([c["key_a"][0], c["key_a"][1], c["key_a"][2], c["key_b"][0]]):
            xs, ct, _, _ = inputs(branch, [n], 400 + i)
            ids = syn.make_token_ids(500 + i, 1, 1).to(DEV)
            xl = [xs[0][None]] if ct is None else [ct, xs[0][None]]
            out = [o.clone() for o in model(xl, ids)]
            h, z = model.last_pooled.clone(), model.last_logits.clone()
            model.graph_eval = False
            ref = model(xl, ids)
            model.graph_eval = True
            assert len(out) == len(ref) == (3 if ct is not None else 2)
            for a, b in zip(out, ref):
                assert a.shape == b.shape and rel(a, b) <= TOL_H, (i, n, rel(a, b))
            assert rel(h, model.last_pooled) <= TOL_H and rel(z, model.last_logits) <= TOL_H, (i, n)
    st = model._eval_stepper
    assert st.replays == 2 and st.eager_steps == 2 and st.n_graphs == 1
    assert not train_ddp.build_model(create_arg_parser(argv)).graph_eval
