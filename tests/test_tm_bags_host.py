"""CPU: the host side of the batched landmark-side chain (mil_tm_pinv_init_bags*, ops.nystrom_core_bags, TransMIL.batch_bags)
on the built library, no GPU - the four grouped entries are declared, exported and bound alike; the status entries refuse a
null pointer and a bag count outside [1, 1024] before any launch; the switch resolves keyword, then environment; config.py
parses --tm_batch_bags and build_model sets it; and, in float64, the GPU tests' cases are not blind to the one mistake the
route must not make: a pseudo-inverse scale taken over the whole batch instead of per bag."""
import argparse
import ctypes
import itertools
import os

import pytest
import torch

import tm_bags_ref as G
import transmil_ref as R
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

EINVAL = -22
MARGIN = 10.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in G.NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["mil_tm_pinv_init_bags"][1] == [P, I, P, P, P, P]             # A2, nb, scale, arg, Z0, stream
    for name in ("mil_tm_pinv_init_bwd_bags", "mil_tm_pinv_init_bwd_bags_fixed"):       # dZ0, Z0, scale, arg, nb, dA2, ws, stream
        assert _lib.SIGNATURES[name][1] == [P, P, P, P, I, P, P, P], name
    assert _lib.SIGNATURES["mil_tm_pinv_ws_floats_bags"] == (ctypes.c_size_t, [I])
    # the grouped entry takes its single-bag twin's arguments plus the bag count
    for one, many in (("mil_tm_pinv_init", "mil_tm_pinv_init_bags"), ("mil_tm_pinv_init_bwd", "mil_tm_pinv_init_bwd_bags"),
                      ("mil_tm_pinv_init_bwd_fixed", "mil_tm_pinv_init_bwd_bags_fixed")):
        assert len(_lib.SIGNATURES[many][1]) == len(_lib.SIGNATURES[one][1]) + 1
    assert "mil_tm_pinv_ws_floats_bags" in _lib.VALUE_RETURNING and not set(G.NAMES[:3]) & _lib.VALUE_RETURNING
    assert lib.mil_abi_version() == _lib.ABI_VERSION


def test_status_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                      # never read: the entries return first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for nb in (0, 1025, -1):
        assert lib.mil_tm_pinv_init_bags(p, nb, p, p, p, None) == EINVAL
        assert lib.mil_tm_pinv_init_bwd_bags(p, p, p, p, nb, p, p, None) == EINVAL
        assert lib.mil_tm_pinv_init_bwd_bags_fixed(p, p, p, p, nb, p, p, None) == EINVAL
    for hole in range(4):                                              # A2, scale, arg, Z0
        a = [p] * 4
        a[hole] = None
        assert lib.mil_tm_pinv_init_bags(a[0], 2, a[1], a[2], a[3], None) == EINVAL, hole
    for hole in range(6):                                              # dZ0, Z0, scale, arg, dA2, ws
        a = [p] * 6
        a[hole] = None
        assert lib.mil_tm_pinv_init_bwd_bags(*a[:4], 2, *a[4:], None) == EINVAL, hole
        assert lib.mil_tm_pinv_init_bwd_bags_fixed(*a[:4], 2, *a[4:], None) == EINVAL, hole
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_pinv_init_bags(p, 0, p, p, p, None)
    assert lib.mil_tm_pinv_ws_floats_bags(3) == 768
    assert lib.mil_tm_pinv_ws_floats_bags(1) == lib.mil_tm_pinv_ws_floats() == 256
    assert lib.mil_tm_pinv_ws_floats_bags(1024) == 256 * 1024
    assert lib.mil_tm_pinv_ws_floats_bags(0) == 0 and lib.mil_tm_pinv_ws_floats_bags(1025) == 0


def test_the_switch_keyword_then_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    for kw, env in itertools.product((None, False, True), (None, "", "0", "1")):
        if env is None:
            monkeypatch.delenv("MIL_TM_BATCH_BAGS", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_BATCH_BAGS", env)
        assert ops.tm_batch_bags(kw) is bool(kw if kw is not None else env == "1"), (kw, env)
    assert TransMIL(2).batch_bags is None


def test_nystrom_core_bags_takes_its_keywords():
    from mil_amd import ops
    qkv, w = torch.zeros((256, 1536)), torch.zeros((8, 1, 33, 1))
    with pytest.raises(_lib.MilHipError, match="no CPU path"):         # accepted: it gets as far as the device check
        ops.nystrom_core_bags([qkv, qkv], w, fused_a3=True, fused_a1=True, deterministic=True, pieces=3)
    with pytest.raises(ValueError):
        ops.nystrom_core_bags([qkv], w, pieces=2)


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--tm_batch_bags", "1"]).tm_batch_bags == 1
    assert create_arg_parser([]).tm_batch_bags == 0
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_batch_bags=1)
    assert build_model(args).extractor_pathology.batch_bags is True
    args.tm_batch_bags = 0
    assert build_model(args).extractor_pathology.batch_bags is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", tm_batch_bags=1))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.batch_bags is True for m in mods)             # the aggregator and the unused extractor
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_batch_bags=1)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set


def test_stage_cases_have_distinct_scales():
    """The three bags of tests/test_gpu_tm_bags_stages.py: a kernel that shared one bag's scale, or the batch's maximum, with
    another bag would be off by more than 1 % there; the arg-max columns are the first, an inner and the last of a bag."""
    scales = [float(G.stage_case(i)[2]["scale"][0]) for i in range(3)]
    args = [G.stage_case(i)[2]["arg"] for i in range(3)]
    print("stage case scales", scales, "args", args)
    assert [round(s, 2) for s in scales] == [18.09, 17.22, 16.97]
    assert tuple(args) == G.STAGE_ARGS == (845, 0, 2047)
    for a, b in itertools.combinations(scales, 2):
        assert abs(a - b) / min(a, b) > 0.01, (a, b)


def test_a_scale_shared_across_the_bags_breaks_the_core_bound():
    """The three-bag case of tests/test_gpu_tm_bags_core.py.  Planted error, in float64: every bag's Z0 divided by (largest row
    sum over ALL bags x largest column sum over ALL bags) instead of by its own scale.  On bag 0 and on bag 1 it has to break
    bound(e32, K_STAGE["core"]) by 10 x on at least one block.  Bag 2 holds both maxima and is unaffected by construction."""
    maxima = [G.own_maxima(G.core_ref(i)[0]) for i in range(3)]
    own = [mr * mc for mr, mc in maxima]
    shared = max(mr for mr, _ in maxima) * max(mc for _, mc in maxima)
    print("own scales", own, "shared", shared)
    assert shared == own[2] and own[2] > 2 * max(own[:2])
    for b in (0, 1):
        qkv, w, dO, pad, ref, r32 = G.core_ref(b)
        blocks = R.core_blocks(qkv.shape[0], pad)
        # the restatement with the bag's own scale as a number is the reference's forward (the scale's own gradient aside)
        same = R.flat_err(G.core_scaled_run(qkv, w, dO, own[b]), ref, {"out": blocks["out"]})
        assert max(same.values()) < 1e-12, same
        e32 = R.flat_err(r32, ref, blocks)
        em = R.flat_err(G.core_scaled_run(qkv, w, dO, shared), ref, blocks)
        m = max(em[k] / R.bound(e32[k], R.K_STAGE["core"]) for k in em)
        print(f"planted shared scale: bag {b} margin {m:.3g}x")
        assert m >= MARGIN, (b, m)
