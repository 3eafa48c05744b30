"""GPU: `aggregator.note_attn = "all"` on the fusion module - the note's weights over the CT tokens (last_note_attn_ct) and over
the patches (last_note_attn) against the float64 restatement of model/sam/transformer.py's token->image attention at its three
sites (tests/note_attn_ref.py: twoway_note_attention on the float64 state dict and the float64 tanh(fc_*) inputs), last_bag_attn
against the float64 softmax of the aggregator's scores in the documented row order (ABMIL) or against TransMIL.flat_segments'
own cls attention after the documented reorder, the switch changing nothing else, and the capacity-bucket forwards - device part
inside the forward, note_attn_finish(lengths) afterwards - held to the same float64 references.

Bound: tests/note_attn_ref.hold, K_NOTE = 16 x max(e32, 1e-7) per block - attn_blocks (bag, 64-key tile, head) for the site
weights, softmax_blocks for the pool weights -, e32 being what the same float32 code loses on the CPU.  Measured ratios:
docs/lab_notes.md."""
from types import SimpleNamespace

import pytest
import torch

import note_attn_ref as R
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS = [70, 130]
B = len(NS)
CT_MAP = (512, 4, 2, 2)                     # D = 4 tokens by the resnetMC3_18 rule, 16 by medicalNet's
CAP = 256


def _args(**kw):
    a = dict(modality=["CT", "pathology"], model_pathology="ABMIL", model_CI="CLIP", aggregator="ABMIL", num_classes=2,
             learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18", clip_layers=1)
    a.update(kw)
    return SimpleNamespace(**a)


_CACHE = {}


def _twoway(modality):
    return "TwoWayTransformer_CT" if list(modality) == ["CT"] else ("TwoWayTransformer_Both" if "CT" in modality
                                                                    else "TwoWayTransformer_Pth")


def _sites(image, point, p, name, dt):
    """(float64 reference [site] -> [H, T, N], the same in float32 held in float64)."""
    q = {k: v.to(dt) for k, v in p.items()}
    s, _, _ = R.twoway_note_attention(image.to(dt), orc.sinusoidal_pe(image.shape[0], 512).to(dt), point.to(dt), q, name)
    return [w.double() for w in s]


def _setup(modality=("CT", "pathology"), model_CT="resnetMC3_18", P=1, agg="ABMIL"):
    """(model, inputs, float64 / float32 site weights per branch): built once per configuration, never changed."""
    key = (tuple(modality), model_CT, P, agg)
    if key in _CACHE:
        return _CACHE[key]
    from mil_amd.model.utils import get_model
    torch.manual_seed(40 + P)
    extra = dict(aggregator="TransMIL", fusion_transmil=1) if agg == "TransMIL" else {}
    model = get_model(_args(modality=list(modality), model_CT=model_CT, **extra)).to(DEV).eval()
    gen = torch.Generator().manual_seed(50 + P)
    ct = torch.randn((B,) + CT_MAP, generator=gen)
    x = torch.zeros((B, max(NS), 768))
    for b, n in enumerate(NS):
        x[b, :n] = torch.randn((n, 768), generator=gen)
    t = torch.randn((B, P, 512), generator=gen)
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items() if not k.startswith("clinic_extractor.")}
    tw = _twoway(modality)
    ref = {"ct": [], "pth": []}
    tok = orc.ct_map_tokens(ct.double(), model_CT)                                 # [B, D, 512]
    for b, n in enumerate(NS):
        if "CT" in modality:
            point = orc.linear_tanh(t[b].double(), p["fc_CI2CT.0.weight"], p["fc_CI2CT.0.bias"])
            ref["ct"].append((_sites(tok[b], point, p, tw, torch.float64), _sites(tok[b], point, p, tw, torch.float32)))
        if "pathology" in modality:
            xi = orc.linear_tanh(x[b, :n].double(), p["fc_pathology.0.weight"], p["fc_pathology.0.bias"])
            point = orc.linear_tanh(t[b].double(), p["fc_CI2Pth.0.weight"], p["fc_CI2Pth.0.bias"])
            ref["pth"].append((_sites(xi, point, p, tw, torch.float64), _sites(xi, point, p, tw, torch.float32)))
    D = tok.shape[1]
    _CACHE[key] = SimpleNamespace(model=model, ct=ct.to(DEV), x=x.to(DEV), t=t.to(DEV), ref=ref, D=D, P=P, modality=list(modality))
    return _CACHE[key]


def _xs(c):
    return [c.ct, c.x] if "pathology" in c.modality else [c.ct]


def _forward(c, on):
    c.model.note_attn = on
    with torch.no_grad():
        out = c.model(_xs(c), None, lengths=NS if "pathology" in c.modality else None, text_features=c.t)
    return [o.clone() for o in out] + [c.model.last_logits.clone(), c.model.last_pooled.clone()]


def _hold_sites(tag, got_sites, refs, lens, P):
    """got_sites[site][bag] [8, n] ([P, 8, n]) against refs[bag] = (ref64, ref32), each [site] -> [H, T, n]."""
    assert len(got_sites) == 3 and all(len(site) == B for site in got_sites)
    top = 0.0
    for s in range(3):
        for b, n in enumerate(lens):
            got = got_sites[s][b]
            assert tuple(got.shape) == ((8, n) if P == 1 else (P, 8, n)), (tag, s, b, tuple(got.shape))
            got = got.reshape(P, 8, n)
            blocks = R.attn_blocks([0, n])
            for tk in range(P):
                ref, r32 = (w[s][:, tk, :].t() for w in refs[b])
                top = max(top, R.hold(f"{tag}.site{s}", f"bag {b} token {tk}", got[tk].t(), ref, r32, blocks))
                sums = got[tk].double().sum(-1).cpu()[None]              # every head sums to 1, within the same bound
                R.hold(f"{tag}.site{s}.sums", f"bag {b} token {tk}", sums, torch.ones_like(sums), r32.sum(0)[None], R.sum_blocks(1))
    print(f"TOP | {tag} | all sites | {top:.2f}")


def _bag_scores(c, scores):
    """The aggregator's scores of every bag in the documented row order, from the buffer's rows (host lengths)."""
    D, P = c.D, c.P
    out = []
    if "pathology" not in c.modality:                       # [B D CT tokens | B P text tokens]
        for b in range(B):
            out.append(torch.cat([scores[b * D:(b + 1) * D], scores[B * D + b * P:B * D + (b + 1) * P]]))
        return out
    off, Rp = R.offsets(NS), sum(NS)                        # [patches | B P CT-side text | B D CT tokens | B P pathology-side text]
    for b in range(B):
        out.append(torch.cat([scores[off[b]:off[b + 1]], scores[Rp + b * P:Rp + (b + 1) * P],
                              scores[Rp + B * P + b * D:Rp + B * P + (b + 1) * D],
                              scores[Rp + B * (P + D) + b * P:Rp + B * (P + D) + (b + 1) * P]]))
    return out


def _hold_bag(tag, got, per_bag_scores):
    assert len(got) == len(per_bag_scores)
    for b, s in enumerate(per_bag_scores):
        assert tuple(got[b].shape) == (s.numel(),), (tag, b, tuple(got[b].shape))
        R.hold("bag_attn", f"{tag} bag {b}", got[b], s.softmax(0), s.float().softmax(0), R.softmax_blocks([0, s.numel()]))


# --------------------------------------------------------------------------- 2. eager, ABMIL aggregator
@pytest.mark.parametrize("modality,model_CT,P", [(("CT", "pathology"), "resnetMC3_18", 1), (("CT", "pathology"), "medicalNet", 1),
                                                 (("CT",), "resnetMC3_18", 1), (("CT",), "medicalNet", 1),
                                                 (("CT", "pathology"), "resnetMC3_18", 10)])
def test_eager_ct_weights_against_float64(modality, model_CT, P):
    c = _setup(modality, model_CT, P)
    assert c.D == (16 if model_CT == "medicalNet" else 4)
    _forward(c, "all")
    m = c.model
    tag = f"{'+'.join(modality)} {model_CT} P {P}"
    _hold_sites(f"note_ct {tag}", m.last_note_attn_ct, c.ref["ct"], [c.D] * B, P)
    if "pathology" in modality:
        _hold_sites(f"note {tag}", m.last_note_attn, c.ref["pth"], NS, P)
    else:
        assert m.last_note_attn is None
    lens = [(n if "pathology" in modality else 0) + c.D + P * (2 if "pathology" in modality else 1) for n in NS]
    assert [a.numel() for a in m.last_bag_attn] == lens
    _hold_bag(tag, m.last_bag_attn, _bag_scores(c, m.aggregator.last_scores.double().cpu()))


@pytest.mark.parametrize("modality", [("CT", "pathology"), ("CT",)])
def test_the_scope_changes_nothing_else(modality):
    c = _setup(modality)
    m = c.model
    m.last_note_attn = m.last_note_attn_ct = m.last_bag_attn = None
    off = _forward(c, False)
    assert m.last_note_attn is None and m.last_note_attn_ct is None and m.last_bag_attn is None
    on = _forward(c, "all")
    assert m.last_note_attn_ct is not None and m.last_bag_attn is not None
    again = _forward(c, False)
    for a, b_, c_ in zip(off, on, again):
        assert torch.equal(a, b_) and torch.equal(a, c_)
    m.note_attn = True                                      # today's scope: CT stays refused, exactly as before
    with torch.no_grad(), pytest.raises(NotImplementedError, match="note_attn is built for modality"):
        m(_xs(c), None, lengths=NS if "pathology" in modality else None, text_features=c.t)
    m.note_attn = "all"                                     # not under no_grad: nothing is kept
    m.last_note_attn = m.last_note_attn_ct = m.last_bag_attn = None
    m(_xs(c), None, lengths=NS if "pathology" in modality else None, text_features=c.t)
    assert m.last_note_attn is None and m.last_note_attn_ct is None and m.last_bag_attn is None
    m.note_attn = "CT"
    with torch.no_grad(), pytest.raises(ValueError, match="note_attn must be"):
        m(_xs(c), None, lengths=NS if "pathology" in modality else None, text_features=c.t)
    m.note_attn = False


def test_true_and_all_agree_on_the_pathology_model():
    """The pathology model: "all" leaves what True leaves, bit for bit, and the forward's results do not move."""
    c = _setup(("pathology",))
    outs = {}
    for on in (False, True, "all"):
        c.model.note_attn = on
        with torch.no_grad():
            out = c.model([c.x], None, lengths=NS, text_features=c.t)
        outs[on] = [o.clone() for o in out] + [c.model.last_logits.clone(), c.model.last_pooled.clone()]
        if on:
            outs[on] += [a for site in c.model.last_note_attn for a in site] + list(c.model.last_bag_attn)
            assert c.model.last_note_attn_ct is None
    assert all(torch.equal(a, b_) for a, b_ in zip(outs[False], outs[True]))
    assert len(outs[True]) == len(outs["all"]) and all(torch.equal(a, b_) for a, b_ in zip(outs[True], outs["all"]))


def test_alignment_base_ct_stays_refused():
    from mil_amd.model.utils import get_model
    model = get_model(_args(modality=["CT"], alignment_base="CT")).to(DEV).eval()
    model.note_attn = "all"
    with torch.no_grad(), pytest.raises(NotImplementedError, match="note_attn"):
        model([torch.zeros((1, 4, 512), device=DEV)], None, text_features=torch.zeros((1, 1, 512), device=DEV))


# --------------------------------------------------------------------------- 3. eager, TransMIL aggregator
@pytest.mark.parametrize("modality", [("CT", "pathology"), ("CT",)])
def test_eager_transmil_bag_weights_are_flat_segments_own(modality):
    """last_bag_attn[b] [2, 8, rows of the bag] = what flat_segments(.., need_attn="cls") returned for that bag, its columns
    moved from sequence order (text tokens first, patches last) to the rows' order in memory."""
    c = _setup(modality, agg="TransMIL")
    m, D, P = c.model, c.D, c.P
    seen = {}
    inner = m.aggregator.flat_segments

    def spy(x0, segs, need_attn=False):
        out = inner(x0, segs, need_attn=need_attn)
        seen.update(segs=segs, need_attn=need_attn, attn=out[1])
        return out
    m.aggregator.flat_segments = spy
    try:
        _forward(c, "all")
    finally:
        del m.aggregator.flat_segments
    assert seen["need_attn"] == "cls" and len(m.last_bag_attn) == B
    for b, n in enumerate(NS):
        a = torch.stack([seen["attn"][0][b], seen["attn"][1][b]])
        if "pathology" in modality:                         # sequence: [P | D | P | patches] -> patches, P, D, P
            T = 2 * P + D
            want = torch.cat([a[..., T:], a[..., :T]], -1)
            assert tuple(want.shape) == (2, 8, n + T)
        else:                                               # sequence: [P | D] -> D, P
            want = torch.cat([a[..., P:], a[..., :P]], -1)
            assert tuple(want.shape) == (2, 8, D + P)
        got = m.last_bag_attn[b]
        assert got.shape == want.shape and torch.equal(got, want)
        assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0
    _hold_sites(f"note_ct transmil {'+'.join(modality)}", m.last_note_attn_ct, c.ref["ct"], [D] * B, P)


# --------------------------------------------------------------------------- 4. the capacity-bucket forwards
def _packed(c):
    x = torch.zeros((CAP, 768), device=DEV)
    r = 0
    for b, n in enumerate(NS):
        x[r:r + n] = c.x[b, :n]
        r += n
    return x


def _site_rows_behind_the_bags_are_zero(m):
    meta, ts = m._note_meta, m._note_tensors
    for i, br in enumerate(meta["branches"]):
        for X in ts[3 * i:3 * i + 3]:
            rows = sum(NS) if br == "pth" else B * meta["D"]
            assert X.shape[0] == (CAP if br == "pth" else rows)
            assert bool((X[rows:] == 0).all()), f"{br}: rows behind the bags must read exactly 0"


@pytest.mark.parametrize("modality", [("pathology",), ("CT", "pathology")])
def test_bucket_forward_abmil_against_float64(modality):
    from mil_amd.segments import FusionBucket
    c = _setup(modality)
    m, D = c.model, c.D
    with_ct = "CT" in modality
    bucket = FusionBucket(CAP, B, DEV, 1, tail=[1, D, 1] if with_ct else None).set_lengths(NS)
    xs = [c.ct, _packed(c)] if with_ct else [_packed(c)]
    m.note_attn = False
    with torch.no_grad():
        off = [o.clone() for o in m(xs, None, text_features=c.t, bucket=bucket)] + [m.last_logits.clone()]
    m.note_attn = "all"
    with torch.no_grad():
        on = [o.clone() for o in m(xs, None, text_features=c.t, bucket=bucket)] + [m.last_logits.clone()]
    assert all(torch.equal(a, b_) for a, b_ in zip(off, on))
    assert m.last_bag_attn is None and m.last_note_attn is None        # the slicing by host lengths is the caller's
    _site_rows_behind_the_bags_are_zero(m)
    w = m._note_tensors[-1]
    assert w.shape == (CAP + B * sum(bucket.tail),) and bool((w[sum(NS):CAP] == 0).all())
    m.note_attn_finish(NS)
    tag = f"bucket abmil {'+'.join(modality)}"
    _hold_sites(f"note {tag}", m.last_note_attn, c.ref["pth"], NS, 1)
    if with_ct:
        _hold_sites(f"note_ct {tag}", m.last_note_attn_ct, c.ref["ct"], [D] * B, 1)
    else:
        assert m.last_note_attn_ct is None
    # the aggregator's scores lie in the bucket's rows: [cap patch rows | segment 0 of every bag | ..]
    s, off_, per = m.aggregator.last_scores.double().cpu(), R.offsets(NS), []
    for b in range(B):
        pieces, base = [s[off_[b]:off_[b + 1]]], CAP
        for rows in bucket.tail:
            pieces.append(s[base + b * rows:base + (b + 1) * rows])
            base += B * rows
        per.append(torch.cat(pieces))
    _hold_bag(tag, m.last_bag_attn, per)
    m.note_attn = True                                      # today's scope: the bucket forward stays refused
    with torch.no_grad(), pytest.raises(NotImplementedError, match="note_attn is built for modality"):
        m(xs, None, text_features=c.t, bucket=bucket)
    m.note_attn = False


@pytest.mark.parametrize("modality", [("pathology",), ("CT", "pathology")])
def test_bucket_forward_transmil_against_float64(modality):
    """The stepper's geometry without graphs: sites against float64; the cls attention of the bucket form against the eager
    form's at the module's own bar for that pair (tests/test_gpu_fusion_transmil_graph.py: TOL_H)."""
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from test_gpu_fusion_transmil_graph import TOL_H, rel
    c = _setup(modality, agg="TransMIL")
    m, D = c.model, c.D
    with_ct = "CT" in modality
    m.note_attn = "all"
    with torch.no_grad():
        m([c.ct, c.x] if with_ct else [c.x], None, lengths=NS, text_features=c.t)
    eager_bag = [a.clone() for a in m.last_bag_attn]
    st = RaggedFusionTransMILStepper(m, None, B=B, use_graph=False, backward=False, ct_shape=CT_MAP if with_ct else None)
    slot = st.slot(sum(NS))
    assert slot.cap == CAP
    slot.x.copy_(_packed(c))
    slot.text.copy_(c.t)
    if with_ct:
        slot.ct.copy_(c.ct)
    st.step(slot, NS)
    _site_rows_behind_the_bags_are_zero(m)
    tag = f"bucket transmil {'+'.join(modality)}"
    _hold_sites(f"note {tag}", m.last_note_attn, c.ref["pth"], NS, 1)
    if with_ct:
        _hold_sites(f"note_ct {tag}", m.last_note_attn_ct, c.ref["ct"], [D] * B, 1)
    T = 2 + D if with_ct else 1
    for b, n in enumerate(NS):
        got = m.last_bag_attn[b]
        assert tuple(got.shape) == (2, 8, n + T) == tuple(eager_bag[b].shape)
        e = rel(got, eager_bag[b])
        print(f"BAG | {tag} | bag {b} | rel to the eager form {e:.2e}")
        assert e <= TOL_H
    m.note_attn = False
