"""CPU: the host side of the packed sequence (mil_tm_*_packed, ops.nystrom_core_packed, TransMIL.packed) on the built library, no
GPU - the twelve entries are declared, exported and bound alike; the status entries refuse a null pointer, a bag count outside
[1, 1024], fewer blocks than bags and more rows than an int holds, before any launch; the size entries return the documented
counts; the switch resolves keyword, then environment; config.py parses --tm_packed and build_model sets it; both steppers' keys
carry ("packed",); the combined indices and the block table are the per-bag ones shifted; and, in float64, the GPU stage
cases (tests/test_gpu_tm_packed_stages.py) are not blind to the three mistakes a packed kernel can make silently."""
import argparse
import ctypes
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

import tm_packed_ref as P
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
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name in P.NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    ptr, i = ctypes.c_void_p, ctypes.c_int
    for name in P.STATUS:                                   # .., blk_off, nb, total_blocks, stream
        assert _lib.SIGNATURES[name][1][-4:] == [ptr, i, i, ptr], name
        twin = name.replace("_packed", "")                  # the twin's arguments without n_pad, plus the three
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[twin][1]) + 2, name
    for name in P.SIZES:                                    # total_blocks, nb, backward
        assert _lib.SIGNATURES[name] == (ctypes.c_size_t, [i, i, i]) and name in _lib.VALUE_RETURNING
    assert not set(P.STATUS) & _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 20 and lib.mil_abi_version() == _lib.ABI_VERSION


def _call(lib, name, ptrs, tab, nb, tb):
    """The status entry with `ptrs` for its pointers (in order), the scale where it has one, the table arguments, a null stream."""
    args, it = [], iter(ptrs)
    for t in _lib.SIGNATURES[name][1][:-4]:
        args.append(next(it) if t is ctypes.c_void_p else 0.125)
    return getattr(lib, name)(*args, tab, nb, tb, None)


def test_status_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                      # never read: the entries return first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in P.STATUS:
        npt = sum(t is ctypes.c_void_p for t in _lib.SIGNATURES[name][1][:-4])
        optional = {5} if name == "mil_tm_tok_attn_fwd_packed" else set()       # its ws: the forward has no workspace
        for nb, tb in ((0, 4), (-1, 4), (1025, 2000), (3, 2), (1, 0), (2, INT_MAX // 256 + 1), (1, INT_MAX)):
            assert _call(lib, name, [p] * npt, p, nb, tb) == EINVAL, (name, nb, tb)
        assert _call(lib, name, [p] * npt, None, 2, 4) == EINVAL, name         # the table
        for hole in set(range(npt)) - optional:
            a = [p] * npt
            a[hole] = None
            assert _call(lib, name, a, p, 2, 4) == EINVAL, (name, hole)
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_resconv_packed(p, p, p, p, 0, 4, None)


def test_size_entries_return_the_documented_counts(lib):
    for tb, nb in ((7, 4), (2, 1), (1, 1), (1024, 1024), (4000, 3)):
        assert lib.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 0) == tb * 8 * 256 * 66
        assert lib.mil_tm_lmk_attn_packed_ws_floats(tb, nb, 1) == nb * 2048 + 2 * tb * 8 * 16384
        assert lib.mil_tm_tok_attn_packed_ws_floats(tb, nb, 0) == 0
        assert lib.mil_tm_tok_attn_packed_ws_floats(tb, nb, 1) == 2 * tb * 8 * 16384
        assert lib.mil_tm_resconv_packed_ws_floats(tb, nb, 0) == 0
        assert lib.mil_tm_resconv_packed_ws_floats(tb, nb, 1) == tb * 264
    # one bag: the single-bag entries' sizes
    for tb in (1, 3):
        for bw in (0, 1):
            assert lib.mil_tm_lmk_attn_packed_ws_floats(tb, 1, bw) == lib.mil_tm_lmk_attn_ws_floats(256 * tb, bw)
            assert lib.mil_tm_tok_attn_packed_ws_floats(tb, 1, bw) == lib.mil_tm_tok_attn_ws_floats(256 * tb, bw)
        assert lib.mil_tm_resconv_packed_ws_floats(tb, 1, 1) == lib.mil_tm_resconv_ws_floats(256 * tb)
    for name in P.SIZES:
        for tb, nb in ((4, 0), (4, 1025), (2, 3), (0, 1), (-1, 1), (INT_MAX // 256 + 1, 1)):
            assert getattr(lib, name)(tb, nb, 1) == 0, (name, tb, nb)


def test_the_switch_keyword_then_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    for kw, env in itertools.product((None, False, True), (None, "", "0", "1")):
        if env is None:
            monkeypatch.delenv("MIL_TM_PACKED", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_PACKED", env)
        assert ops.tm_packed(kw) is bool(kw if kw is not None else env == "1"), (kw, env)
    assert TransMIL(2).packed is None


def test_nystrom_core_packed_takes_its_arguments():
    from mil_amd import ops
    qkv, w = torch.zeros((768, 1536)), torch.zeros((8, 1, 33, 1))
    with pytest.raises(_lib.MilHipError, match="no CPU path"):         # accepted: it gets as far as the device check
        ops.nystrom_core_packed(qkv, [1, 2], w, deterministic=True, pieces=3)
    with pytest.raises(_lib.MilHipError, match="outside the built shape"):
        ops.nystrom_core_packed(qkv, [1, 1], w)
    with pytest.raises(ValueError):
        ops.nystrom_core_packed(qkv, [1, 2], w, pieces=2)
    for bad in ([], [0, 1], [1] * 1025):
        with pytest.raises(ValueError):
            ops.tm_packed_table(bad, torch.device("cpu"))
    t = ops.tm_packed_table([1, 2, 1, 3], torch.device("cpu"))
    assert (t.nb, t.total_blocks, t.rows) == (4, 7, 1792) and t.dev.dtype == torch.int32
    assert t.dev.tolist() == P.table((1, 2, 1, 3)) == [0, 1, 3, 4, 7, 0, 1, 1, 2, 3, 3, 3]


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--tm_packed", "1"]).tm_packed == 1
    assert create_arg_parser([]).tm_packed == 0
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed=1)
    assert build_model(args).extractor_pathology.packed is True
    args.tm_packed = 0
    assert build_model(args).extractor_pathology.packed is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", tm_packed=1))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.packed is True for m in mods)
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed=1)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set


def test_both_steppers_key_the_packed_route():
    """("packed",) ends the key when the slot holds more than one bag and the switch is on - in the place of ("batch_bags",)
    when both are on -, never with one bag, and (the image-only stepper) never with the attention outputs."""
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.transmil_step import RaggedTransMILStepper
    ex = TransMIL(2)
    model = SimpleNamespace(extractor_pathology=ex, aggregator=ex, training=True, patch_attn=False)
    image = lambda sides: RaggedTransMILStepper.key(SimpleNamespace(model=model, backward=True), sides)        # noqa: E731
    fus_self = SimpleNamespace(model=model, backward=True, sides=lambda lengths: tuple(lengths))
    fusion = lambda lengths: RaggedFusionTransMILStepper.key(fus_self, 1024, lengths)                                   # noqa: E731
    for key, one, two in ((image, (7,), (7, 16)), (fusion, (49,), (49, 256))):
        ex.packed, ex.batch_bags = None, None
        plain = key(two)
        assert "packed" not in plain and "batch_bags" not in plain
        ex.packed = True
        assert key(two) == plain + ("packed",) and "packed" not in key(one)
        ex.batch_bags = True
        assert key(two) == plain + ("packed",)                  # it takes the place of ("batch_bags",)
        ex.packed = False
        assert key(two) == plain + ("batch_bags",)
    ex.packed, ex.batch_bags, model.patch_attn = True, None, True
    assert "packed" not in image((7, 16))


def test_combined_indices_are_the_per_bag_ones_shifted():
    from mil_amd.model.dim1.TransMIL import PackedGeometry, pad_index, packed_index, side_geometry
    sides = (3, 16, 39)
    geo = [side_geometry(s) for s in sides]
    assert [g["n_pad"] for g in geo] == [256, 512, 1536] and [g["pad"] for g in geo] == [246, 255, 14]
    pad, unpad, blocks = packed_index(sides)
    assert blocks == [1, 2, 6]
    row = prow = 0
    for g in geo:
        own = pad_index(g)
        assert pad[prow:prow + g["n_pad"]] == [i if i < 0 else i + row for i in own]
        assert unpad[row:row + g["seq"]] == [prow + g["pad"] + j for j in range(g["seq"])]
        # the round trip: sequence row j comes back from where the pad index put it
        assert [pad[u] for u in unpad[row:row + g["seq"]]] == list(range(row, row + g["seq"]))
        row, prow = row + g["seq"], prow + g["n_pad"]
    assert len(pad) == prow == 2304 and len(unpad) == row
    pk = PackedGeometry(sides, torch.device("cpu"))
    assert pk.pad_idx.tolist() == pad and pk.unpad_idx.tolist() == unpad and pk.table.dev.tolist() == P.table((1, 2, 6))
    assert pk.table.dev.tolist()[:4] == [0, 1, 3, 9]


# ---- float64: the GPU stage cases see the three mistakes.  The GPU tests hold every per-bag output to BIT-equality with the
# single-bag entry, a bound of zero, so any move at all would show; here each mistake is held to more: it has to move the
# output by 10 x the float64 bound the single-bag entries themselves are held to (tests/test_gpu_transmil_stages.py:
# bound(e32, K_STAGE[stage]) per block), so it cannot hide in rounding either.
def _margin(wrong, ref, r32, k):
    blocks = {"all": (Ellipsis,)}
    e32 = R.block_err(r32, ref, blocks)["all"]
    return R.block_err(wrong, ref, blocks)["all"] / R.bound(e32, k)


@pytest.mark.parametrize("blocks", [P.BLOCKS[0]])
def test_a_conv_window_that_crosses_a_bag_boundary_shows(blocks):
    c = P.stage_case(blocks)
    ref, r32, wrong = P.conv_ref(c, blocks), P.conv_ref(c, blocks, torch.float32), P.conv_ref(c, blocks, leak=True)
    for b in range(len(blocks)):
        rows = P.bag_rows(blocks, b)
        m = _margin(wrong[rows], ref[rows], r32[rows], R.K_STAGE["resconv"])
        print(f"planted conv leak: bag {b} margin {m:.3g}x")
        assert m >= MARGIN, (b, m)
    inner = slice(256 + 16, 768 - 16)                          # away from the boundaries nothing moves
    assert torch.equal(wrong[inner], ref[inner])


@pytest.mark.parametrize("blocks", [P.BLOCKS[0]])
def test_a_landmark_mean_with_a_neighbours_group_shows(blocks):
    c = P.stage_case(blocks)
    ref, r32 = P.landmarks_ref(c, blocks), P.landmarks_ref(c, blocks, torch.float32)
    wrong = P.landmarks_ref(c, blocks, neighbour=True)
    for b in range(len(blocks)):
        for which, name in enumerate(("qL", "kL")):
            m = _margin(wrong[which][b], ref[which][b], r32[which][b], R.K_STAGE["landmarks"])
            print(f"planted neighbour l: bag {b} {name} margin {m:.3g}x")
            assert m >= MARGIN, (b, name, m)


@pytest.mark.parametrize("blocks", [P.BLOCKS[0]])
def test_a_merge_over_all_chunks_shows(blocks):
    c = P.stage_case(blocks)
    ref, r32, wrong = P.lmk_w_ref(c, blocks), P.lmk_w_ref(c, blocks, torch.float32), P.lmk_w_ref(c, blocks, all_chunks=True)
    for b in range(len(blocks)):
        m = _margin(wrong[b], ref[b], r32[b], R.K_STAGE["core"])
        print(f"planted merge over all chunks: bag {b} margin {m:.3g}x")
        assert m >= MARGIN, (b, m)
