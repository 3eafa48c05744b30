"""GPU: the per-patch cls attention on the packed route (csrc/cls_attn_fused.hip: mil_tm_cls_attn_packed; ops.tm_cls_attention_packed,
nystrom_core_packed(need_attn="cls"); TransMIL.packed_cls / MIL_TM_PACKED_CLS) - the kernel alone on bags of 250, 7, 1500 and 256
patches, the core, the module in eval and train mode and the replayed slot of two bags.

The kernel is held to BIT-equality with the single-bag entry mil_tm_cls_attn_fused on every bag's rows and slices, and through it
to float64: every block of cls_blocks within R.bound(e32, K_FUSED), K_FUSED as tests/test_gpu_cls_attn_fused.py has it for that
entry - bit equality with a kernel already held to that bound means no new constant is measured.  Each comparison with float64
prints its `RATIO |` lines first."""
import pytest
import torch

import tm_cls_packed_ref as Q
import tm_fixed_ref as F
import tm_packed_ref as P
import transmil_ref as R
from fused_attn_common import DEV, _bits, rel
from test_gpu_cls_attn_fused import K_FUSED
from test_gpu_transmil_cls_attn import _agg, _bag, _model

pytestmark = pytest.mark.gpu

PACKED_FWD = tuple(n for n in P.STATUS if "bwd" not in n)                 # what a packed forward launches, once per layer
CLS_ENTRIES = ("mil_tm_cls_attn", "mil_tm_cls_attn_fused")                # the single-bag cls entries


def hold(tag, got, ref, r32, N, s):
    """Every block of got [8, N] within bound(e32, K_FUSED) of ref; the ratios are printed first."""
    blocks = Q.cls_blocks(N, s)
    e32, eg = R.block_err(r32, ref, blocks), R.block_err(got, ref, blocks)
    assert set(eg) == set(e32) and len(eg) >= R.H + 2
    bad = []
    for b, e in eg.items():
        print(f"RATIO | cls_attn_packed | {tag} | {b} | gpu {e:.2e} | e32 {e32[b]:.2e} | {e / max(e32[b], R.FLOOR):.2f}")
        if not e <= R.bound(e32[b], K_FUSED):
            bad.append((b, e, e32[b]))
    assert not bad, (tag, bad)


# --------------------------------------------------------------------------- the kernel alone
def _dev_case(peak):
    """The packed case on the device in float32 - what the kernel is given -, its block table, and the float64 / float32
    restatements per bag."""
    from mil_amd import ops
    c = Q.packed_case(peak)
    dev = [c[k].float().to(DEV) for k in ("qkv", "qL", "kL", "Z", "lse3")]
    return c, dev, ops.tm_packed_table(Q.BLOCKS, DEV)


def _single(c, dev, b, n):
    """mil_tm_cls_attn_fused on bag b's rows and slices, host length n."""
    from mil_amd import ops
    qkv, qL, kL, Z, lse3 = dev
    g = c["geo"][b]
    row = 256 * Q.offsets(Q.BLOCKS)[b]
    return ops.tm_cls_attention_fused(qkv[row:row + g["n_pad"]], qL[b], kL[b], Z[b], lse3[b], g["pad"], g["s"], n=n)


@pytest.mark.parametrize("peak", Q.PEAKS)
def test_kernel_alone(peak):
    from mil_amd import ops
    c, dev, tab = _dev_case(peak)
    qkv, qL, kL, Z, lse3 = dev
    assert qkv.shape == (2816, 1536) and tab.blocks == (2, 1, 6, 2)
    with F.recorded() as log:
        outs = ops.tm_cls_attention_packed(qkv, tab, qL, kL, Z, lse3, Q.SIDES, n=list(Q.LENGTHS))
    assert [n for n, _ in log] == ["mil_tm_cls_attn_packed"]
    again = ops.tm_cls_attention_packed(qkv, tab, qL, kL, Z, lse3, ops.tm_cls_table(Q.SIDES, DEV), n=list(Q.LENGTHS))
    ref, r32 = Q.per_bag_ref(c), Q.per_bag_ref(c, torch.float32)
    assert len(outs) == 4 and outs[0].untyped_storage().data_ptr() == outs[3].untyped_storage().data_ptr()      # views of one buffer
    for b, (N, s) in enumerate(zip(Q.LENGTHS, Q.SIDES)):
        a = outs[b]
        assert a.shape == (R.H, s * s) and a.dtype == torch.float32 and a.is_contiguous()
        assert torch.equal(_bits(a), _bits(_single(c, dev, b, N))), b      # the single-bag entry's bits
        assert torch.equal(_bits(a), _bits(again[b])), b                   # no atomics, every sum in a fixed order
        assert bool((a[:, N:] == 0).all())
        hold(f"kernel peak {peak} bag {b} N {N}", a[:, :N], ref[b][:, :N], r32[b][:, :N].double(), N, s)


@pytest.mark.parametrize("peak", Q.PEAKS)
def test_kernel_alone_with_the_lengths_on_the_device(peak):
    """One length above its bucket (300 in side 16 -> 256), one below (3 in side 39 -> 1445), two inside: the host call at the
    clamped values, bit for bit; and a host length outside its bucket is refused."""
    from mil_amd import _lib, ops
    c, dev, tab = _dev_case(peak)
    given, clamped = [300, 7, 3, 256], [256, 7, 1445, 256]
    assert [Q.clamp(n, s) for n, s in zip(given, Q.SIDES)] == clamped
    len_dev = torch.tensor(given, dtype=torch.int32, device=DEV)
    outs = ops.tm_cls_attention_packed(*dev[:1], tab, *dev[1:], Q.SIDES, len_dev=len_dev)
    want = ops.tm_cls_attention_packed(*dev[:1], tab, *dev[1:], Q.SIDES, n=clamped)
    ref, r32 = Q.per_bag_ref(c, lengths=clamped), Q.per_bag_ref(c, torch.float32, lengths=clamped)
    for b, (N, s) in enumerate(zip(clamped, Q.SIDES)):
        assert torch.equal(_bits(outs[b]), _bits(want[b])), b
        assert torch.equal(_bits(outs[b]), _bits(_single(c, dev, b, N))), b
        assert bool((outs[b][:, N:] == 0).all())
        hold(f"kernel dev peak {peak} bag {b} N {N}", outs[b][:, :N], ref[b][:, :N], r32[b][:, :N].double(), N, s)
    for bad in ([300, 7, 1500, 256], [250, 7, 3, 256], [250, 4, 1500, 256], [250, 7, 1500]):
        with pytest.raises(_lib.MilHipError):
            ops.tm_cls_attention_packed(*dev[:1], tab, *dev[1:], Q.SIDES, n=bad)
    with pytest.raises(_lib.MilHipError):                                  # sides that do not go with the table's blocks
        ops.tm_cls_attention_packed(*dev[:1], tab, *dev[1:], (16, 3, 39, 15), n=[250, 7, 1500, 200])
    with pytest.raises(ValueError):
        ops.tm_cls_attention_packed(*dev[:1], tab, *dev[1:], Q.SIDES)


# --------------------------------------------------------------------------- the core
def _core_packed(qkv, w, dO, **kw):
    from mil_amd import ops
    qd = qkv.clone().requires_grad_(True)
    wd = w.clone().requires_grad_(True)
    with F.recorded() as log:
        out = ops.nystrom_core_packed(qd, Q.BLOCKS, wd, deterministic=True, **kw)
        o, attn = out if isinstance(out, tuple) else (out, None)
        o.backward(dO)
    torch.cuda.synchronize()
    return {"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad}, attn, [n for n, _ in log]


def test_core_forms_the_attention_and_leaves_out_and_the_backward_alone():
    from mil_amd import ops
    c = Q.packed_case(1.0)
    qkv = c["qkv"].float().to(DEV)
    gen = torch.Generator().manual_seed(5)
    w = ((torch.rand((R.H, 1, R.CONV, 1), generator=gen) * 2 - 1) / R.CONV ** 0.5).to(DEV)
    dO = torch.randn((Q.ROWS, 512), generator=gen).to(DEV)
    plain, none, _ = _core_packed(qkv, w, dO)
    on, attn, names = _core_packed(qkv, w, dO, need_attn="cls", cls=dict(sides=Q.SIDES, n=list(Q.LENGTHS)))
    assert none is None and len(attn) == 4
    for k in ("out", "dqkv", "dw"):
        assert F.bits_equal(on[k], plain[k]), k
    assert names.count("mil_tm_cls_attn_packed") == 1 and not set(names) & set(CLS_ENTRIES) and not set(names) & set(P.SINGLE)
    row = 0
    for b, g in enumerate(c["geo"]):
        a = attn[b]
        assert a.shape == (R.H, g["s"] ** 2) and not a.requires_grad and bool((a[:, g["N"]:] == 0).all())
        _, single = ops.nystrom_core(qkv[row:row + g["n_pad"]], w, "cls", pad=g["pad"], s=g["s"], n=g["N"], fused_cls=True,
                                     deterministic=True)
        assert torch.equal(_bits(a), _bits(single)), b
        row += g["n_pad"]
    len_dev = torch.tensor(Q.LENGTHS, dtype=torch.int32, device=DEV)
    dev, attn_dev, _ = _core_packed(qkv, w, dO, need_attn="cls", cls=dict(sides=ops.tm_cls_table(Q.SIDES, DEV), len_dev=len_dev))
    assert F.bits_equal(dev["out"], plain["out"]) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(attn_dev, attn))
    with pytest.raises(ValueError):
        ops.nystrom_core_packed(qkv, Q.BLOCKS, w, need_attn=True)


# --------------------------------------------------------------------------- the module
def test_module_eval_against_restatement(monkeypatch):
    """Lengths [7, 250, 300] with packed = packed_cls = True: both layers' attention against the float64 restatement at the bound
    of test_gpu_cls_attn_fused.test_module_eval_against_restatement, h against the same launches without the attention (its bar
    there) and against float64 (1e-4, the golden test's bar on h); the packed entries ran once per layer and no single-bag one."""
    for name in ("MIL_TM_PACKED", "MIL_TM_PACKED_CLS", "MIL_TM_FUSED_CLS"):
        monkeypatch.delenv(name, raising=False)
    lengths = [7, 250, 300]
    net, p = _model()
    net.eval()
    net.packed = net.packed_cls = True
    bags = [_bag(n) for n in lengths]
    x = torch.cat([b[0] for b in bags], 0).float().to(DEV)
    with torch.no_grad():
        with F.recorded() as log:
            h, (a0, a1) = net(x, lengths, need_attn="cls")
        names = [n for n, _ in log]
        h0, none = net(x, lengths)
        assert all(names.count(n) == 2 for n in PACKED_FWD + ("mil_tm_cls_attn_packed",)), names
        assert not set(names) & set(P.SINGLE) and not set(names) & set(CLS_ENTRIES)
        net.packed_cls = None                                             # the default: the bag-by-bag launches
        with F.recorded() as log:
            hd, (d0, d1) = net(x, lengths, need_attn="cls")
        names = [n for n, _ in log]
    assert none == [None, None] and rel(h, h0) < 1e-6
    assert not set(names) & set(P.NAMES) and "mil_tm_cls_attn_packed" not in names
    assert names.count("mil_tm_cls_attn") == 2 * len(lengths) and names.count("mil_tm_landmarks") == 2 * len(lengths)
    assert len(a0) == len(a1) == len(d0) == len(lengths) and rel(h, hd) < 1e-4
    for b, (n, (x64, p64, ref, r32)) in enumerate(zip(lengths, bags)):
        s = R.geometry(n)["s"]
        with torch.no_grad():
            h64, _ = R.transmil(x64, p64)
        e = rel(h[b], h64)
        print(f"RATIO | cls_attn_packed | module N {n} of {lengths} | h | rel {e:.2e} | bound 1e-04")
        assert e <= 1e-4, (b, e)
        for layer, a in enumerate((a0[b], a1[b])):
            assert a.shape == (R.H, n) and not a.requires_grad
            hold(f"module N {n} of {lengths} layer {layer}", a, ref[layer], r32[layer], n, s)


def test_train_mode_gradients_are_those_without_the_attention():
    """Lengths [250, 7], train mode, deterministic, the keep bits forced: with need_attn="cls" on the packed route every
    parameter gradient, dx and h have the bits of the packed route with need_attn=False - the attention is no part of the
    graph -, and the attention is bit-reproducible."""
    lengths = [250, 7]
    net, _ = _model()
    net.train()
    net._drop_seed = 77
    net.deterministic = True
    net.packed = net.packed_cls = True
    x = torch.randn((sum(lengths), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        net(x, lengths)
    net.force_bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    gw = torch.randn((2, 512), generator=torch.Generator().manual_seed(3)).to(DEV)
    runs = []
    for want in ("cls", False, "cls"):
        net.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        with F.recorded() as log:
            h, attn = net(xd, lengths, need_attn=want)
            (h * gw).sum().backward()
        torch.cuda.synchronize()
        names = [n for n, _ in log]
        assert names.count("mil_tm_cls_attn_packed") == (2 if want else 0) and not set(names) & set(P.SINGLE + CLS_ENTRIES)
        g = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
        g["dx"], g["h"] = xd.grad.clone(), h.detach().clone()
        runs.append((g, attn))
    (on, attn), (off, none), (again, attn2) = runs
    assert none == [None, None] and on.keys() == off.keys() and len(on) > 20
    for k in on:
        assert F.bits_equal(on[k], off[k]) and F.bits_equal(on[k], again[k]), k
    for layer in range(2):
        for b, n in enumerate(lengths):
            a = attn[layer][b]
            assert a.shape == (R.H, n) and not a.requires_grad and bool(torch.isfinite(a).all())
            assert torch.equal(_bits(a), _bits(attn2[layer][b])), (layer, b)


# --------------------------------------------------------------------------- the replayed slot
def test_replayed_slot_of_two_bags_carries_the_attention(monkeypatch):
    """RaggedTransMILStepper, B = 2, eval forward with patch_attn on a model with packed = packed_cls = True: the key ends
    ("packed", "cls"); the eager visit and the capture's replay give the same bits; a second replay with other lengths of the
    same sides gives THAT step's attention (held to float64, zeros from the new lengths on); a model with the switch off gets
    another key."""
    from mil_amd.transmil_step import RaggedTransMILStepper
    for name in ("MIL_TM_PACKED", "MIL_TM_PACKED_CLS", "MIL_TM_FUSED_CLS"):
        monkeypatch.delenv(name, raising=False)
    model = _agg()
    model.patch_attn = True
    ex = model.extractor_pathology
    ex.packed = ex.packed_cls = True
    st = RaggedTransMILStepper(model, None, B=2, backward=False)
    seen = []
    for i, lengths in enumerate([[40, 250], [40, 250], [45, 240]]):        # eager visit, capture with its first replay, replay
        bags = [_bag(n) for n in lengths]
        slot = st.slot(lengths)
        assert slot.sides == (7, 16) and st.key(slot.sides)[-2:] == ("packed", "cls") and "patch_attn" in st.key(slot.sides)
        slot.x[:sum(lengths)].copy_(torch.cat([b[0] for b in bags], 0).float())
        with F.recorded() as log:
            st.step(slot, lengths)
        torch.cuda.synchronize()
        if i == 0:
            names = [n for n, _ in log]
            assert names.count("mil_tm_cls_attn_packed") == 2 and not set(names) & set(P.SINGLE + CLS_ENTRIES)
        got = [[a.clone() for a in layer] for layer in slot.last["patch_attn"]]
        seen.append(got)
        for layer in range(2):
            for b, (n, s) in enumerate(zip(lengths, slot.sides)):
                a = got[layer][b]
                assert a.shape == (R.H, s * s) and bool((a[:, n:] == 0).all())
                hold(f"replay step {i} N {n} layer {layer}", a[:, :n], bags[b][2][layer], bags[b][3][layer], n, s)
    assert st.n_graphs == 1 and st.eager_steps == 1 and st.replays == 2
    for layer in range(2):
        for b in range(2):
            assert torch.equal(_bits(seen[0][layer][b]), _bits(seen[1][layer][b])), (layer, b)
            assert not torch.equal(_bits(seen[1][layer][b]), _bits(seen[2][layer][b])), (layer, b)
    on = st.key((7, 16))
    ex.packed_cls = False
    off = st.key((7, 16))
    assert off != on and "packed" not in off and "cls" not in off and "patch_attn" in off
