"""GPU: every gate-forward and weight-gradient route of the fp32 one-call step (mil_image_only_step_run) against a float64
restatement of the step, element by element.  Each case names the kernels it is meant to reach; tests/step_ref.py mirrors
the host rules that choose them and the library states the plan its launches execute (mil_gate_step_route): both must
give the named route, so a shape cannot drift to another kernel unnoticed.

Bounds: scores, gates and logits max|got - ref| <= 1e-5 max|ref|; every gradient <= 1e-4 max|ref|; loss within 1e-5
relative; top-1 equal.  On the split-bf16 (PW) cases the forward's error is also at most 1.5x that of the fp32-MFMA K loop
on the same input (floor 1e-7)."""
import pytest
import torch

from mil_amd import ops, synthetic as syn
from mil_amd.bags import BagLayout, bucket_rows
from mil_amd.trainer import PARAM_ORDER, ImageOnlyTrainer, RaggedImageOnlyStepper
from step_ref import (BU, BV, GF_TM, WB, WU, WV, WW, dw_split, gates_ref, keep_from_bits, lib_route, max_err, num_cu, split_kg,
                      step_ref, step_route)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL_FWD, TOL_GRAD, TOL_LOSS = 1e-5, 1e-4, 1e-5
GRAD_NAMES = ("dWv", "dbv", "dWu", "dbu", "dw", "db", "dWf", "dbf")       # PARAM_ORDER


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.empty_cache()


def _randn(R, L, seed):
    return torch.randn((R, L), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _run(p, x, lay, y, train, pieces=True, backward=True):
    tr = ImageOnlyTrainer(p, DEV, train_mode=train, seed=11)
    tr.gate_pieces = pieces
    tr.forward(x, lay, y)
    if backward:
        tr.backward()
    torch.cuda.synchronize()
    return tr


def _outputs(tr, n):
    """What the step computed for its first n rows (bucketed batches: the true rows)."""
    last = tr.last
    return dict(scores=last["scores"][:n].clone(), gates=last["gates"][:n].clone(), logits=last["logits"].clone(),
                prob=last["prob"].clone(), loss=tr.loss_sum.clone(), grad=tr.fp.grad.clone())


def _ref_of(tr, x, lengths, p, y, n=None):
    """float64 step on the keep bits this trainer's pass drew (train mode)."""
    L = x.shape[1]
    kx = keep_from_bits(tr.last["xbits"][:n], L) if tr.train_mode else None
    km = keep_from_bits(tr.last["mbits"], L) if tr.train_mode else None
    return step_ref(x, lengths, p, y, tr.loss, kx, km)


def _check(tag, tr, got, ref):
    e = {k: max_err(got[k], ref[k]) for k in ("scores", "gates", "logits")}
    e["loss"] = abs(float(got["loss"]) - ref["loss"]) / abs(ref["loss"])
    ge = {}
    for k in PARAM_ORDER:
        g = tr.fp.view(got["grad"], k)
        if k == WB:
            # d loss / d b is zero (a shift of every score leaves the softmax as it is): rounding noise on both sides,
            # held against the scale of the score weights' gradient
            ge[k] = float(g.abs().max()) / float(ref["grads"][WW].abs().max())
        else:
            ge[k] = max_err(g, ref["grads"][k])
    print(f"{tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + " | " +
          " ".join(f"{n} {ge[k]:.1e}" for n, k in zip(GRAD_NAMES, PARAM_ORDER)))
    for k in ("scores", "gates", "logits"):
        assert e[k] <= TOL_FWD, (tag, k, e[k])
    assert e["loss"] <= TOL_LOSS, (tag, e["loss"])
    for n, k in zip(GRAD_NAMES, PARAM_ORDER):
        assert ge[k] <= TOL_GRAD, (tag, n, ge[k])
    assert torch.equal(got["prob"].argmax(1).cpu(), ref["prob"].argmax(1).cpu()), tag
    return e


def _pw_within_fp32_loop(tag, e, p, x, lay, y, train):
    """The same input through the fp32-MFMA K loop (no weight pieces): the split-bf16 forward's error stays within 1.5x of
    that loop's (floor 1e-7), the rule of test_gpu_gate_pieces.py."""
    tr = _run(p, x, lay, y, train, pieces=False, backward=False)
    assert step_route(x.shape[0], x.shape[1], y.shape[1], train, aligned32=lay.aligned32, pieces=False)["main"] == "fwd2"
    keep = keep_from_bits(tr.last["xbits"], x.shape[1]) if train else None
    rs, rg = gates_ref(x, p, keep)
    f32 = dict(scores=max_err(tr.last["scores"], rs), gates=max_err(tr.last["gates"], rg))
    print(f"{tag}: fp32-MFMA loop scores {f32['scores']:.1e} gates {f32['gates']:.1e}")
    for k in f32:
        assert e[k] <= 1.5 * max(f32[k], 1e-7), (tag, k, e[k], f32[k])


def _route_case(tag, lengths, L, C, want, train):
    R = sum(lengths)
    lay = BagLayout.make(lengths, DEV)
    have = step_route(R, L, C, train, aligned32=lay.aligned32)
    assert {k: have[k] for k in want} == want, (tag, have)
    planned = lib_route(R, L, C, train, aligned32=lay.aligned32)
    print(f"{tag}: library route {planned}")
    assert {k: planned[k] for k in want} == want, (tag, planned)
    p = syn.image_only_params(300 + L + C, L=L, C=C)
    x = _randn(R, L, R + L)
    y = syn.make_labels(R, len(lengths), C).to(DEV)
    tr = _run(p, x, lay, y, train)
    e = _check(tag, tr, _outputs(tr, R), _ref_of(tr, x, lengths, p, y))
    del tr
    if have["main"] == "fwd2_pw":
        _pw_within_fp32_loop(tag, e, p, x, lay, y, train)


PW = dict(main="fwd2_pw", tail=None, pool="alone", dw="dw2")
PW_FUSED = dict(PW, pool="fused")
GEN = dict(bits="in_kernel")
DRAWN = dict(bits="generator")
# id, bag lengths, L, C, the route in both modes, in train mode only, in eval mode only
CASES = [
    ("r32_rt1", [1000] * 8, 512, 2, dict(main="r32", rt=1, tail=None, pool="alone", dw="dw<1>"), DRAWN, {}),
    ("r32_rt2", [1000] * 16, 512, 2, dict(main="r32", rt=2, tail=None, pool="alone", dw="dw2"), DRAWN, {}),
    ("r32_rt3", [1000] * 24, 512, 2, dict(main="r32", rt=3, tail=None, pool="alone", dw="dw2"), DRAWN, {}),
    # the bench headline: 32 x 1024 x 512, pool pass in the forward's epilogue
    ("pw_fused_pool", [1024] * 32, 512, 2, PW_FUSED, GEN, {}),
    # 234.5 row tiles: the last workgroup holds 64 rows = two whole 32-row pool tiles
    ("pw_fused_pool_partial_tile", [1024] * 29 + [320], 512, 2, PW_FUSED, GEN, {}),
    # ragged bags (1 and 33 rows among them): stand-alone pool, the last workgroup holds 48 rows
    ("pw_partial_tile", [1] + [1024] * 14 + [33] + [1024] * 14 + [1294], 512, 2, PW, GEN, {}),
    # other widths without the fused pool; 31 000 rows (not ~33 000: the rows beyond 32 768 would go to the big tail)
    *[(f"pw_L{L}_C{C}", [1000] * 31, L, C, PW, GEN, {}) for L in (256, 768, 1024) for C in (2, 3)],
    # 391 row tiles: two rounds of the grid, 80 rows in the last workgroup
    ("pw_two_rounds_partial_tile", [1000] * 50, 768, 2, PW, GEN, {}),
    # one whole round + 40 rows: eval mil_linear_small_fwd + k_gate_tail_scores; train: generator launch, PW with the
    # given bits, r32 for the 40 rows
    ("pw_small_tail", [1024] * 32 + [40], 512, 2, dict(main="fwd2_pw", tail="small", pool="alone", dw="dw2"),
     dict(bits="generator", tail_kernel="r32", tail_rt=1), dict(tail_kernel="linear_small")),
    ("pw_big_tail", [1024] * 32 + [1000], 1024, 2,
     dict(main="fwd2_pw", tail="big", tail_kernel="r32", tail_rt=1, pool="alone", dw="dw2"), DRAWN, {}),
    # the authors' regime: one bag of a few thousand patches
    ("r32_one_bag_dw_kg1", [7600], 512, 2, dict(main="r32", rt=1, tail=None, pool="alone", dw="dw<1>"), DRAWN, {}),
]


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name,lengths,L,C,route,route_train,route_eval", CASES, ids=[c[0] for c in CASES])
def test_route_against_float64(name, lengths, L, C, route, route_train, route_eval, train):
    want = dict(route, **(route_train if train else dict(route_eval, bits=None)))
    _route_case(f"{name} {'train' if train else 'eval'}", lengths, L, C, want, train)


def test_dw_kg2_route_against_float64():
    """k_gate_bwd_dw<.., KG = 2>: R * L >= 2^29, where k_gate_bwd_dw2 (32-bit offsets) hands over.  512 bags x 1024 rows
    x 1024 columns, 2 GiB of x, eval mode."""
    _route_case("dw_kg2 eval", [1024] * 512, 1024, 2, dict(PW, dw="dw<2>", bits=None), False)


# ------------------------------------------------------------------------------------------ k_gate_bwd_dw<true, KG> (bf16 x)
def _x16_dw_shape(kg):
    """KG = 2: L = 1024 and 29 rows more than the smallest row count that plans two K groups (5 149 rows on 256 CUs: ten
    chunks of 544, the last of 253 rows).  KG = 1: 100 x 128, four chunks of one 32-row slice each, the last of 4 rows."""
    if kg == 1:
        return 100, 128
    L = 1024
    rmin = 512 * (num_cu() // (3 * (L // 128)))
    assert split_kg(rmin - 1, L, num_cu()) == 1 and split_kg(rmin, L, num_cu()) == 2, rmin
    return rmin + 29, L


@pytest.mark.parametrize("keep", [False, True], ids=["eval", "keep_bits"])
@pytest.mark.parametrize("kg", [2, 1], ids=["kg2", "kg1"])
def test_x16_weight_gradient_against_float64(kg, keep):
    """k_gate_bwd_dw<true, KG, *> through ops.gate_bwd_params_x16 (the x16 shapes of test_gpu_bf16.py all plan KG = 1; bf16 x
    has no dw2 kernel, so where fp32 x would take it the plan's two K groups run here).  dWv, dbv, dWu, dbu, dw, db against
    float64 on the bf16-rounded x, max|got - ref| <= 1e-4 max|ref| (TOL_GRAD).  Measured (docs/lab_notes.md; the same bits
    on the build before the kernels were rebuilt from parts): at most 3.5e-7 (kg2) and 1.8e-7 (kg1) over the six outputs."""
    R, L = _x16_dw_shape(kg)
    S, kc = dw_split(R, L, num_cu())
    assert split_kg(R, L, num_cu()) == kg and lib_route(R, L, 2, False)["dw"] == ("dw2" if kg == 2 else "dw<1>"), (R, L)
    assert R % 32 != 0 and R % kc != 0 and S > 1, (R, kc, S)
    g = torch.Generator(device=DEV).manual_seed(500 + R + L)
    x16 = torch.randn((R, L), device=DEV, generator=g).to(torch.bfloat16)
    pre = torch.randn((R, 384), device=DEV, generator=g)
    gates = torch.cat([torch.tanh(pre[:, :192]), torch.sigmoid(pre[:, 192:])], 1).contiguous()
    ds = torch.randn(R, device=DEV, generator=g) * 1e-3
    w = torch.randn(192, device=DEV, generator=g) * 0.1
    bits = torch.randint(-2 ** 31, 2 ** 31, (R, L // 32), device=DEV, generator=g).to(torch.int32) if keep else None
    xscale = 2.0 if keep else 1.0
    got = dict(dWv=torch.empty((192, L), device=DEV), dbv=torch.empty(192, device=DEV), dWu=torch.empty((192, L), device=DEV),
               dbu=torch.empty(192, device=DEV), dw=torch.empty(192, device=DEV), db=torch.empty(1, device=DEV))
    ops.gate_bwd_params_x16(x16, gates, ds, w, *got.values(), xbits=bits, xscale=xscale)
    torch.cuda.synchronize()
    # float64: dPreV = ds w U (1 - V^2), dPreU = ds w V U (1 - U); dW = dPre^T (x keep) xscale
    xd = x16.double() * (keep_from_bits(bits, L) if keep else 1.0)
    V, U = gates[:, :192].double(), gates[:, 192:].double()
    d, wd = ds.double().unsqueeze(1), w.double().unsqueeze(0)
    pv, pu = d * wd * U * (1 - V * V), d * wd * V * U * (1 - U)
    ref = dict(dWv=pv.t() @ xd * xscale, dbv=pv.sum(0), dWu=pu.t() @ xd * xscale, dbu=pu.sum(0), dw=(d * V * U).sum(0),
               db=d.sum().view(1))
    err = {k: max_err(got[k], ref[k]) for k in got}
    print(f"x16 dw kg{kg} {R} x {L} {'keep bits' if keep else 'eval'}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v <= TOL_GRAD, (kg, keep, k, v)


# ------------------------------------------------------------------------------------------ k_gate_fwd (L > 4096)
@pytest.mark.parametrize("keep", [False, True], ids=["eval", "keep_bits"])
def test_legacy_gate_forward_against_float64(keep):
    """k_gate_fwd, the 128-row kernel with 64-bit source pointers that takes over beyond L = 4096 (ops.gate_scores_fwd with
    saved gates), at L = 4128: 48 rows more than the smallest row count that leaves the 32-row kernel, so 191 full tiles
    and one of 49 rows.  Once without keep bits, once with bits from ops.dropout_keep_bits and xscale = 2.  Scores and
    gates against float64, max|got - ref| <= 1e-5 max|ref| (TOL_FWD) - measured before the kernel's epilogue became the
    shared gate_fwd_scores_epilogue: scores 1.03e-6, gates 4.67e-6 without keep bits; 5.6e-7, 4.23e-6 with them."""
    L = 4128
    rmin = ((3 * num_cu()) // 4 - 1) * GF_TM + 1          # gate_route_plan: fewer 128-row tiles than 3/4 of the CUs go to r32
    R = rmin + 48
    for route in (step_route, lib_route):
        assert route(rmin - 1, L, 2, False, given_bits=keep)["main"] == "r32"
        assert route(rmin, L, 2, False, given_bits=keep)["main"] == "legacy"
        have = route(R, L, 2, False, given_bits=keep)
        assert have["main"] == "legacy" and have["tail"] is None, have
    p = syn.image_only_params(300 + L, L=L)
    x = _randn(R, L, R + L)
    bits = ops.dropout_keep_bits(R, L, 0.5, 29, 0, DEV) if keep else None
    gp = [p[k].to(DEV) for k in (WV, BV, WU, BU)] + [p[WW].reshape(-1).to(DEV), p[WB].to(DEV)]
    scores, gates = ops.gate_scores_fwd(x, *gp, save_gates=True, xbits=bits, xscale=2.0 if keep else 1.0)
    torch.cuda.synchronize()
    rs, rg = gates_ref(x, p, keep_from_bits(bits, L) if keep else None)
    es, eg = max_err(scores, rs), max_err(gates, rg)
    print(f"legacy {R} x {L} {'keep bits' if keep else 'eval'}: scores {es:.2e} gates {eg:.2e}")
    assert es <= TOL_FWD and eg <= TOL_FWD, (es, eg)


# ------------------------------------------------------------------------------------------ bucketed (device lengths)
BUCKETS = {24576: [11800, 11000], 32768: [15000, 15904]}


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("cap", sorted(BUCKETS))
def test_bucketed_pw_step_ignores_the_rows_beyond_the_batch(cap, train):
    """A bucketed step (DeviceBagLayout: lengths and tile map on the device) at a capacity that runs the split-bf16
    forward: once with the rows beyond the true count zeroed, once holding large finite garbage.  The true rows' results
    and every gradient are bit-identical between the two, and both match float64."""
    L, C = 512, 2
    lengths = BUCKETS[cap]
    n = sum(lengths)
    assert bucket_rows(n) == cap
    want = dict(PW, bits="in_kernel" if train else None)
    have = step_route(cap, L, C, train, bucketed=True)
    assert {k: have[k] for k in want} == want, have
    planned = lib_route(cap, L, C, train, bucketed=True)
    print(f"bucket {cap} {'train' if train else 'eval'}: library route {planned}")
    assert {k: planned[k] for k in want} == want, planned
    p = syn.image_only_params(71, L=L)
    x = _randn(n, L, 72)
    y = syn.make_labels(73, len(lengths)).to(DEV)
    runs = []
    for garbage in (False, True):
        tr = ImageOnlyTrainer(p, DEV, train_mode=train, seed=13)
        slot = RaggedImageOnlyStepper(tr, B=len(lengths), use_graph=False).slot(n)
        assert slot.cap == cap
        slot.x[:n].copy_(x)
        if garbage:
            slot.x[n:].copy_(_randn(cap - n, L, 74) * 1e3)
        else:
            slot.x[n:].zero_()
        slot.y.copy_(y)
        slot.layout.set_lengths(lengths)
        tr.forward(slot.x, slot.layout, slot.y)
        tr.backward()
        torch.cuda.synchronize()
        runs.append((tr, _outputs(tr, n)))
    (tr, a), (_, b) = runs
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} depends on the rows beyond the batch"
    _check(f"bucket {cap} {'train' if train else 'eval'}", tr, a, _ref_of(tr, x, lengths, p, y, n))


@pytest.mark.parametrize("adam", ["in_fold", "stage"])
def test_weight_pieces_follow_every_update_across_buckets(adam):
    """Steps alternating between the 24 576- and 32 768-row buckets.  in_fold: RaggedImageOnlyStepper with graphs - each
    bucket's step is captured on its second visit and replayed, Adam in the fold launch rewrites the planes; stage:
    eager forward / backward and MIL_STAGE_ADAM on its own.  After every update the next forward's gates and scores equal
    float64 from the CURRENT masters: a plane left one Adam step (~1e-3) behind misses the bound by orders of magnitude."""
    L = 512
    fold = adam == "in_fold"
    tr = ImageOnlyTrainer(syn.image_only_params(75, L=L), DEV, lr=1e-3, train_mode=True, seed=17, counted=fold)
    st = RaggedImageOnlyStepper(tr, B=2, use_graph=fold)
    seq = [[11800, 11000], [15000, 15904], [12000, 11900], [15500, 16000], [11000, 12500], [16100, 15200]]
    for i, lengths in enumerate(seq):
        n = sum(lengths)
        slot = st.slot(n)
        slot.x[:n].copy_(_randn(n, L, 80 + i))
        slot.y.copy_(syn.make_labels(90 + i, len(lengths)).to(DEV))
        before = tr.fp.flat.clone()
        if fold:
            st.step(slot, lengths)
        else:
            slot.layout.set_lengths(lengths)
            tr.forward(slot.x, slot.layout, slot.y)
            tr.backward()
            tr.reduce_and_step()
        tr.forward(slot.x, slot.layout, slot.y)
        torch.cuda.synchronize()
        moved = float((tr.fp.flat - before).abs().max())
        assert moved > 1e-4, (i, moved)
        keep = keep_from_bits(tr.last["xbits"][:n], L)
        rs, rg = gates_ref(slot.x[:n], tr.fp.state_dict(), keep)
        es, eg = max_err(tr.last["scores"][:n], rs), max_err(tr.last["gates"][:n], rg)
        print(f"adam {adam}, step {i} (bucket {slot.cap}): scores {es:.1e} gates {eg:.1e}, largest update {moved:.1e}")
        assert es <= TOL_FWD and eg <= TOL_FWD, (i, es, eg)
    if fold:
        assert st.replays >= 4 and len(st.slots) == 2
