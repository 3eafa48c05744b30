"""CPU: the host side of the packed PPEG (mil_tm_ppeg_*_packed, ops.tm_ppeg_packed, TransMIL.packed_ppeg) on the built library, no
GPU - the four entries are declared, exported and bound alike; the status entries refuse a null pointer, a bag count outside
[1, 1024], fewer than two rows per bag and more rows than a 512-wide int index holds, before any launch; the size entry returns the
documented counts; the switch resolves keyword, then environment; config.py parses --tm_packed_ppeg and build_model sets it; both
steppers' keys end ("packed", "ppeg") only with both switches on and more than one bag; the host table equals its restatement;
and, in float64, the GPU stage case (tests/test_gpu_tm_ppeg_packed_stages.py) is not blind to the three mistakes a packed PPEG
kernel can make silently."""
import argparse
import ctypes
import itertools
import os
from types import SimpleNamespace

import pytest
import torch

import tm_ppeg_packed_ref as Q
import transmil_ref as R
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

EINVAL = -22
FACTOR = 100.0
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name in Q.NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    ptr, i = ctypes.c_void_p, ctypes.c_int
    for name in Q.STATUS:                                   # .., tab, nb, total_rows, stream
        assert _lib.SIGNATURES[name][1][-4:] == [ptr, i, i, ptr], name
        twin = name.replace("_packed", "")                  # the twin's arguments without s, plus the three
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[twin][1]) + 2, name
        assert all(t is ptr for t in _lib.SIGNATURES[name][1][:-4]), name
    assert _lib.SIGNATURES["mil_tm_ppeg_packed_ws_floats"] == (ctypes.c_size_t, [i])
    assert "mil_tm_ppeg_packed_ws_floats" in _lib.VALUE_RETURNING and not set(Q.STATUS) & _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 21 and lib.mil_abi_version() == _lib.ABI_VERSION


def _call(lib, name, ptrs, tab, nb, rows):
    return getattr(lib, name)(*ptrs, tab, nb, rows, None)


def test_status_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                      # never read: the entries return first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in Q.STATUS:
        npt = len(_lib.SIGNATURES[name][1]) - 4                         # every pointer in front of the table: ws included
        for nb, rows in ((0, 10), (-1, 10), (1025, 4000), (3, 5), (1, 1), (1, 0), (1, -4), (2, INT_MAX // 512 + 1), (1, INT_MAX)):
            assert _call(lib, name, [p] * npt, p, nb, rows) == EINVAL, (name, nb, rows)
        assert _call(lib, name, [p] * npt, None, 2, 12) == EINVAL, name          # the table
        for hole in range(npt):
            a = [p] * npt
            a[hole] = None
            assert _call(lib, name, a, p, 2, 12) == EINVAL, (name, hole)
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_ppeg_fwd_packed(p, p, p, p, p, p, p, p, p, 0, 10, None)


def test_size_entry_returns_the_documented_counts(lib):
    for c in (1, 2, 8, 1000, INT_MAX // 25600):
        assert lib.mil_tm_ppeg_packed_ws_floats(c) == c * 50 * 512
    for c in (0, -1, INT_MAX // 25600 + 1, INT_MAX):
        assert lib.mil_tm_ppeg_packed_ws_floats(c) == 0, c
    for s in (1, 3, 8, 9, 16, 17, 125):                               # one bag: the single-bag entry's size
        assert lib.mil_tm_ppeg_packed_ws_floats(Q.chunks((s,))) == lib.mil_tm_ppeg_ws_floats(s), s
    assert Q.chunks(Q.SIDES[0]) == 8 and lib.mil_tm_ppeg_packed_ws_floats(8) == 204800


def test_the_switch_keyword_then_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    for kw, env in itertools.product((None, False, True), (None, "", "0", "1")):
        if env is None:
            monkeypatch.delenv("MIL_TM_PACKED_PPEG", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_PACKED_PPEG", env)
        assert ops.tm_packed_ppeg(kw) is bool(kw if kw is not None else env == "1"), (kw, env)
    assert TransMIL(2).packed_ppeg is None


def test_tm_ppeg_packed_takes_its_arguments():
    from mil_amd import ops
    sides = Q.SIDES[0]
    W = [torch.zeros(s) for s in ((512, 1, 7, 7), (512,), (512, 1, 5, 5), (512,), (512, 1, 3, 3), (512,))]
    with pytest.raises(_lib.MilHipError, match="no CPU path"):         # accepted: it gets as far as the device check
        ops.tm_ppeg_packed(torch.zeros((449, 512)), sides, *W, deterministic=True)
    with pytest.raises(_lib.MilHipError, match="outside the built shape"):
        ops.tm_ppeg_packed(torch.zeros((448, 512)), sides, *W)
    for bad in ([], [0, 1], [3, -2], [1] * 1025, [2048, 100]):
        with pytest.raises(ValueError):
            ops.tm_ppeg_table(bad, torch.device("cpu"))
    t = ops.tm_ppeg_table(sides, torch.device("cpu"))
    assert (t.nb, t.rows, t.chunks, t.sides) == (5, 449, 8, sides) and t.dev.dtype == torch.int32


def test_the_host_table_is_its_restatement():
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import PackedGeometry
    for sides in Q.SIDES + ((1,), (1, 1), (125,), (16, 16, 16, 16), (44, 39, 32, 23) * 2):
        want = Q.table(sides)
        gmax, cmax, zmax = Q.dims(sides)
        assert ops.tm_ppeg_table_host(sides) == want, sides
        assert len(want) == 4 * len(sides) + 3 + gmax + cmax
        assert sum(sides) <= gmax and Q.chunks(sides) <= cmax and (max(sides) + 7) // 8 <= zmax, sides      # the launches cover the bags
    sides = Q.SIDES[0]
    t = Q.table(sides)
    assert t[:6] == [0, 10, 92, 94, 159, 449] and t[6:11] == list(sides)
    assert t[11:17] == [0, 3, 12, 13, 21, 38] and t[17:23] == [0, 1, 3, 4, 5, 8]
    assert Q.dims(sides) == (47, 10, 3) and t[23 + 47:] == [0, 1, 1, 2, 3, 4, 4, 4, -1, -1]
    assert Q.table((9,)) == [0, 82, 9, 0, 9, 0, 2] + [0] * 9 + [0, 0]
    pk = PackedGeometry(sides, torch.device("cpu"))                  # the geometry of both steppers builds it from the sides
    assert pk.ppeg_table.dev.tolist() == t and pk.ppeg_table.rows == len(pk.unpad_idx) == 449


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--tm_packed_ppeg", "1"]).tm_packed_ppeg == 1
    assert create_arg_parser([]).tm_packed_ppeg == 0
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed=1, tm_packed_ppeg=1)
    ex = build_model(args).extractor_pathology
    assert ex.packed is True and ex.packed_ppeg is True
    args.tm_packed_ppeg = 0
    ex = build_model(args).extractor_pathology
    assert ex.packed is True and ex.packed_ppeg is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", tm_packed=1, tm_packed_ppeg=1))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.packed is True and m.packed_ppeg is True for m in mods)
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_packed_ppeg=1)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set


def test_both_steppers_key_the_packed_ppeg():
    """("packed", "ppeg") ends the key with both switches on and more than one bag; ("packed",) with only the first; nothing new
    for one bag, with `packed` off, or (the image-only stepper) with the attention outputs."""
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.transmil_step import RaggedTransMILStepper
    ex = TransMIL(2)
    model = SimpleNamespace(extractor_pathology=ex, aggregator=ex, training=True, patch_attn=False)
    image = lambda sides: RaggedTransMILStepper.key(SimpleNamespace(model=model, backward=True), sides)        # noqa: E731
    fus_self = SimpleNamespace(model=model, backward=True, sides=lambda lengths: tuple(lengths))
    fusion = lambda lengths: RaggedFusionTransMILStepper.key(fus_self, 1024, lengths)                                   # noqa: E731
    for key, one, two in ((image, (7,), (7, 16)), (fusion, (49,), (49, 256))):
        ex.packed, ex.batch_bags, ex.packed_ppeg = None, None, None
        plain, plain_one = key(two), key(one)
        ex.packed, ex.packed_ppeg = True, True
        assert key(two) == plain + ("packed", "ppeg") and key(one) == plain_one
        ex.packed_ppeg = False
        assert key(two) == plain + ("packed",)
        ex.packed_ppeg = None
        assert key(two) == plain + ("packed",)                  # the environment decides: off
        ex.packed, ex.packed_ppeg = False, True
        assert key(two) == plain and key(one) == plain_one      # without the packed route it changes nothing
        ex.batch_bags = True
        assert key(two) == plain + ("batch_bags",)
    ex.packed, ex.batch_bags, ex.packed_ppeg, model.patch_attn = True, None, True, True
    assert "packed" not in image((7, 16)) and "ppeg" not in image((7, 16))


def test_the_switch_in_the_environment_reaches_the_key(monkeypatch):
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.transmil_step import RaggedTransMILStepper
    ex = TransMIL(2)
    model = SimpleNamespace(extractor_pathology=ex, training=True, patch_attn=False)
    key = lambda: RaggedTransMILStepper.key(SimpleNamespace(model=model, backward=True), (7, 16))        # noqa: E731
    monkeypatch.setenv("MIL_TM_PACKED", "1")
    monkeypatch.delenv("MIL_TM_PACKED_PPEG", raising=False)
    assert key()[-1:] == ("packed",)                            # MIL_TM_PACKED=1 alone: as before
    monkeypatch.setenv("MIL_TM_PACKED_PPEG", "1")
    assert key()[-2:] == ("packed", "ppeg")
    monkeypatch.setenv("MIL_TM_PACKED", "0")
    assert "packed" not in key() and "ppeg" not in key()


# ---- float64: the GPU stage case sees the three mistakes.  The GPU test holds every bag's y and dx to BIT-equality with the
# single-bag entry, a bound of zero; here each mistake has to move y and dx of every bag by 100 x the float64 bound the single-bag
# entry itself is held to (R.hold("ppeg", ..): bound(e32, K_STAGE["ppeg"]) over the bag's rows), so it cannot hide in rounding.
def test_the_restatement_is_the_per_bag_reference():
    sides = Q.SIDES[0]
    runs = Q.per_bag(sides)
    y, dx = Q.packed_ref(sides), Q.packed_ref(sides, flip=True)
    for b in range(len(sides)):
        rows = Q.bag_rows(sides, b)
        assert float((y[rows] - runs[b]["y"]).abs().max()) <= 1e-12 and float((dx[rows] - runs[b]["dx"]).abs().max()) <= 1e-12, b


@pytest.mark.parametrize("plant", ["side", "window", "cls"])
def test_a_planted_mistake_shows_in_every_bag(plant):
    sides = Q.SIDES[0]
    whole = {"all": (Ellipsis,)}
    for flip, name in ((False, "y"), (True, "dx")):
        ref, r32 = Q.packed_ref(sides, flip=flip), Q.packed_ref(sides, torch.float32, flip=flip)
        wrong = Q.packed_ref(sides, flip=flip, plant=plant)
        for b, s in enumerate(sides):
            rows = Q.bag_rows(sides, b)
            e32 = R.block_err(r32[rows], ref[rows], whole)["all"]
            ratio = R.block_err(wrong[rows], ref[rows], whole)["all"] / R.bound(e32, R.K_STAGE["ppeg"])
            print(f"planted {plant}: bag {b} (side {s}) {name} moves by {ratio:.3g} x the bound")
            assert ratio >= FACTOR, (plant, name, b, ratio)
