"""CPU: the host side of the per-patch cls attention on the packed route (mil_tm_cls_attn_packed, ops.tm_cls_attention_packed,
nystrom_core_packed(need_attn="cls"), TransMIL.packed_cls / MIL_TM_PACKED_CLS / --tm_packed_cls) on the built library, no GPU - the
two entries are declared, exported and bound alike at ABI 22; the size entry returns the documented counts; the status entry
refuses a null pointer, a bad bag or block count, a patch count outside [nb, 256 total_blocks) and a misaligned operand before any
launch; the geometry table equals a hand-written one; the switch resolves keyword, then environment, and reaches config.py,
build_model and both steppers' keys; and, in float64, the GPU kernel case (tests/test_gpu_tm_cls_packed.py) is not blind to the
four mistakes a packed cls kernel can make silently."""
import argparse
import ctypes
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

import tm_cls_packed_ref as Q
import transmil_ref as R
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

EINVAL = -22
MARGIN = 10.0
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in Q.NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    ptr, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["mil_tm_cls_attn_packed"][1][-4:] == [ptr, i, i, ptr]         # .., blk_off, nb, total_blocks, stream
    assert "mil_tm_cls_attn_packed_ws_floats" in _lib.VALUE_RETURNING and "mil_tm_cls_attn_packed" not in _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 22 and lib.mil_abi_version() == _lib.ABI_VERSION


def test_size_entry_returns_the_documented_counts(lib):
    assert lib.mil_tm_cls_attn_packed_ws_floats(11, 4) == 4 * 8 * 256 + 8 * 256 * 11 == Q.ws_floats(11, 4) == 30720
    assert lib.mil_tm_cls_attn_packed_ws_floats(1, 1) == 8 * 256 + 8 * 256 == Q.ws_floats(1, 1)
    for tb, nb in ((1, 1), (2, 1), (1024, 1024), (4000, 7)):
        assert lib.mil_tm_cls_attn_packed_ws_floats(tb, nb) == Q.ws_floats(tb, nb), (tb, nb)
        assert lib.mil_tm_cls_attn_packed_ws_floats(tb, 1) == lib.mil_tm_cls_attn_fused_ws_floats(256 * tb)     # one bag: its twin's
    for tb, nb in ((0, 0), (3, 4), (4, 0), (4, -1), (2000, 1025), (INT_MAX // 256 + 1, 1)):
        assert lib.mil_tm_cls_attn_packed_ws_floats(tb, nb) == 0, (tb, nb)


def _call(lib, ptrs, patches, nb, tb, qkv=None):
    """ptrs: qkv, qL, kL, Z, lse3, cls_tab, len_dev, ws, out, blk_off."""
    q, qL, kL, Z, lse3, ctab, ln, ws, out, tab = ptrs
    return lib.mil_tm_cls_attn_packed(q if qkv is None else qkv, qL, kL, Z, lse3, ctab, patches, ln, ws, out, tab, nb, tb, None)


def test_status_entry_refuses_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                      # never read: the entry returns first
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = [p] * 10
    for nb, tb in ((0, 4), (-1, 4), (1025, 4000), (4, 3), (1, 0), (1, INT_MAX // 256 + 1)):      # bad nb, total_blocks < nb, too many rows
        assert _call(lib, good, max(nb, 1), nb, tb) == EINVAL, (nb, tb)
    for patches in (0, 3, -5, 256 * 11, 256 * 11 + 7, INT_MAX):        # nb = 4 bags of at least one patch, fewer than the rows
        assert _call(lib, good, patches, 4, 11) == EINVAL, patches
    for hole in range(10):
        a = list(good)
        a[hole] = None
        assert _call(lib, a, sum(s * s for s in Q.SIDES), 4, 11) == EINVAL, hole
    for k in range(3):                                                 # qkv, qL, kL are read as float4
        a = list(good)
        a[k] = ctypes.c_void_p(p.value + 4)
        assert _call(lib, a, sum(s * s for s in Q.SIDES), 4, 11) == EINVAL, k
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_cls_attn_packed(*[p] * 5, p, 10, p, p, p, p, 0, 4, None)


def test_the_geometry_table_is_the_hand_written_one():
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import PackedGeometry
    want = [16, 3, 39, 16, 0, 256, 265, 1786, 2042]
    assert Q.cls_table(Q.SIDES) == want and ops.tm_cls_table_host(Q.SIDES) == want
    assert ops.tm_cls_table_host([1]) == [1, 0, 1] and ops.tm_cls_table_host((125, 2)) == [125, 2, 0, 15625, 15629]
    for sides in ((1,), (1, 1), (125,), (16, 16, 16, 16), (44, 39, 32, 23) * 2):
        assert ops.tm_cls_table_host(sides) == Q.cls_table(sides), sides
    for bad in ([], [0, 1], [3, -2], [1] * 1025, [46341]):
        with pytest.raises(ValueError):
            ops.tm_cls_table(bad, torch.device("cpu"))
    t = ops.tm_cls_table(Q.SIDES, torch.device("cpu"))
    assert (t.nb, t.patches, t.sides, t.off) == (4, 2042, Q.SIDES, want[4:]) and t.dev.dtype == torch.int32 and t.dev.tolist() == want
    pk = PackedGeometry(Q.SIDES, torch.device("cpu"))                # the geometry of both steppers builds it from the sides
    assert pk.cls_table.dev.tolist() == want and pk.table.blocks == Q.BLOCKS and pk.table.rows == Q.ROWS == 2816
    # the blocks of the table are those of the sides, as ops.tm_cls_attention_packed checks them
    assert [-(-(s * s + 1) // 256) for s in Q.SIDES] == list(Q.BLOCKS) and [R.geometry(n)["s"] for n in Q.LENGTHS] == list(Q.SIDES)
    assert [R.geometry(n)["pad"] for n in Q.LENGTHS] == [255, 246, 14, 255] and R.geometry(256)["add"] == 0


def test_the_switch_keyword_then_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    for kw, env in itertools.product((None, False, True), (None, "", "0", "1")):
        if env is None:
            monkeypatch.delenv("MIL_TM_PACKED_CLS", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_PACKED_CLS", env)
        assert ops.tm_packed_cls(kw) is bool(kw if kw is not None else env == "1"), (kw, env)
    assert TransMIL(2).packed_cls is None


def test_the_ops_take_their_arguments():
    from mil_amd import ops
    qkv, w = torch.zeros((Q.ROWS, 1536)), torch.zeros((8, 1, 33, 1))
    with pytest.raises(ValueError, match="no packed form"):
        ops.nystrom_core_packed(qkv, Q.BLOCKS, w, need_attn=True)
    with pytest.raises(ValueError, match="need_attn"):
        ops.nystrom_core_packed(qkv, Q.BLOCKS, w, need_attn="all")
    for cls in (None, dict(sides=Q.SIDES), dict(n=list(Q.LENGTHS)), dict(sides=Q.SIDES, n=list(Q.LENGTHS), len_dev=torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="cls=dict"):
            ops.nystrom_core_packed(qkv, Q.BLOCKS, w, need_attn="cls", cls=cls)
    tab = ops.tm_packed_table(Q.BLOCKS, torch.device("cpu"))
    small = [torch.zeros((4, 8, 256, 64))] * 2 + [torch.zeros((4, 8, 256, 256)), torch.zeros((4, 8, 256))]
    with pytest.raises(ValueError, match="either"):
        ops.tm_cls_attention_packed(qkv, tab, *small, Q.SIDES)
    with pytest.raises(ValueError, match="either"):
        ops.tm_cls_attention_packed(qkv, tab, *small, Q.SIDES, n=list(Q.LENGTHS), len_dev=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.MilHipError, match="no CPU path"):        # accepted: it gets as far as the device check
        ops.tm_cls_attention_packed(qkv, tab, *small, Q.SIDES, n=list(Q.LENGTHS))


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--tm_packed_cls", "1"]).tm_packed_cls == 1
    assert create_arg_parser([]).tm_packed_cls == 0
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed=1, tm_packed_cls=1)
    ex = build_model(args).extractor_pathology
    assert ex.packed is True and ex.packed_cls is True and ex.packed_ppeg is None
    args.tm_packed_cls = 0
    ex = build_model(args).extractor_pathology
    assert ex.packed is True and ex.packed_cls is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", tm_packed=1, tm_packed_cls=1))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.packed is True and m.packed_cls is True for m in mods)
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed_cls=1)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set


def test_both_steppers_key_the_packed_cls(monkeypatch):
    """The image-only stepper: with patch_attn set, `packed and packed_cls` keeps the packed route and the key ends ("packed",
    "cls") or ("packed", "ppeg", "cls"), patch_attn staying in it; with packed_cls off such a slot has no packed marker, as
    before; without patch_attn the switch changes nothing.  The fusion stepper carries the marker wherever it carries `packed`."""
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.transmil_step import RaggedTransMILStepper
    monkeypatch.delenv("MIL_TM_PACKED_CLS", raising=False)
    ex = TransMIL(2)
    model = SimpleNamespace(extractor_pathology=ex, aggregator=ex, training=False, patch_attn=True)
    image = lambda sides: RaggedTransMILStepper.key(SimpleNamespace(model=model, backward=False), sides)        # noqa: E731
    plain, plain_one = image((7, 16)), image((7,))
    assert "patch_attn" in plain and "packed" not in plain
    ex.packed = True
    assert image((7, 16)) == plain                               # the switch unset: the attention keeps the bag-by-bag route
    ex.packed_cls = True
    assert image((7, 16)) == plain + ("packed", "cls") and image((7,)) == plain_one
    ex.packed_ppeg = True
    assert image((7, 16)) == plain + ("packed", "ppeg", "cls")
    ex.packed_ppeg, ex.packed_cls = None, False
    assert image((7, 16)) == plain
    monkeypatch.setenv("MIL_TM_PACKED_CLS", "1")                 # the attribute wins over the environment ...
    assert image((7, 16)) == plain
    ex.packed_cls = None                                         # ... which decides when it is None
    assert image((7, 16)) == plain + ("packed", "cls")
    monkeypatch.delenv("MIL_TM_PACKED_CLS")
    ex.packed, ex.packed_cls = False, True
    assert image((7, 16)) == plain                               # without the packed route it changes nothing
    ex.packed, model.patch_attn = True, False
    assert image((7, 16))[-1:] == ("packed",) and "cls" not in image((7, 16))          # no attention asked: no marker
    fus_self = SimpleNamespace(model=model, backward=True, sides=lambda lengths: tuple(lengths))
    fusion = lambda lengths: RaggedFusionTransMILStepper.key(fus_self, 1024, lengths)                           # noqa: E731
    assert fusion((49, 256))[-2:] == ("packed", "cls") and "packed" not in fusion((49,))
    ex.packed_ppeg = True
    assert fusion((49, 256))[-3:] == ("packed", "ppeg", "cls")
    ex.packed_cls = None
    assert fusion((49, 256))[-2:] == ("packed", "ppeg")
    ex.packed = False
    assert "packed" not in fusion((49, 256)) and "cls" not in fusion((49, 256))


# ---- float64: the GPU kernel case sees the four mistakes.  The GPU test holds every bag to BIT-equality with the single-bag entry
# and, per block of cls_blocks, to bound(e32, K_FUSED) of float64; here each mistake has to leave that bound by 10 x on some block.
def test_the_restatement_is_the_per_bag_reference():
    for peak in Q.PEAKS:
        c = Q.packed_case(peak)
        assert c["qkv"].shape == (Q.ROWS, 1536) and [g["l"] for g in c["geo"]] == list(Q.BLOCKS)
        ref = Q.per_bag_ref(c)
        got = Q.bag_views(Q.packed_out(c))
        for b, (N, s) in enumerate(zip(Q.LENGTHS, Q.SIDES)):
            assert ref[b].shape == got[b].shape == (R.H, s * s) and bool((ref[b][:, N:] == 0).all()) and bool((got[b][:, N:] == 0).all())
            e = R.block_err(got[b][:, :N], ref[b][:, :N], Q.cls_blocks(N, s))
            assert max(e.values()) <= 1e-12, (peak, b, e)
        assert torch.equal(Q.packed_flat(ref), torch.cat([a.reshape(-1) for a in ref]))
        # other lengths of the same sides, as a device length gives them: the clamp is the bucket's
        assert [Q.clamp(n, s) for n, s in zip((300, 7, 3, 256), Q.SIDES)] == [256, 7, 1445, 256]


@pytest.mark.parametrize("plant", Q.MUTATIONS)
def test_a_planted_mistake_leaves_the_gpu_bound(plant):
    from test_gpu_cls_attn_fused import K_FUSED
    for peak in Q.PEAKS:
        c = Q.packed_case(peak)
        ref, r32 = Q.per_bag_ref(c), Q.per_bag_ref(c, torch.float32)
        wrong = Q.bag_views(Q.packed_out(c, mutate=plant))
        best = (0.0, None)
        for b, (N, s) in enumerate(zip(Q.LENGTHS, Q.SIDES)):
            blocks = Q.cls_blocks(N, s)
            e32 = R.block_err(r32[b][:, :N].double(), ref[b][:, :N], blocks)
            em = R.block_err(wrong[b][:, :N], ref[b][:, :N], blocks)
            blk = max(em, key=lambda k: em[k] / R.bound(e32[k], K_FUSED))
            margin = em[blk] / R.bound(e32[blk], K_FUSED)
            print(f"planted {plant:<8} peak {peak} bag {b} (N {N}) margin {margin:9.1f}x on {blk}")
            if margin > best[0]:
                best = (margin, b)
        assert best[0] >= MARGIN, (plant, peak, best)
