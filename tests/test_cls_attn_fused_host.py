"""CPU: the cls attention on the fused passes (need_attn="cls" with fused_cls; csrc/cls_attn_fused.hip) - its restatement
(tests/cls_attn_fused_ref.py) against the definition on the maps (test_transmil_cls_attn_host.cls_attn_ref), the planted errors
against the GPU bound of tests/test_gpu_cls_attn_fused.py, the C ABI on the built library and the switch.  No GPU."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import transmil_ref as R
from cls_attn_fused_ref import CASES, MUTATIONS, cls_blocks, cls_fused_ref, fused_case
from test_transmil_cls_attn_host import cls_attn_ref, core_pieces

from mil_amd import _lib

MARGIN = 10.0
EINVAL = -22
GPU = "tests/test_gpu_cls_attn_fused.py::"
NAMES = ("mil_tm_cls_attn_fused_ws_floats", "mil_tm_cls_attn_fused")


@pytest.mark.parametrize("n_pad,N,peak", CASES)
def test_restatement_equals_the_definition_on_the_maps(n_pad, N, peak):
    qkv, ops64, ref, r32, g = fused_case(n_pad, N, peak)
    with torch.no_grad():
        want = cls_attn_ref(*core_pieces(qkv), g["pad"], N, g["s"])
    blocks = cls_blocks(N, g["s"])
    e = R.block_err(ref, want, blocks)
    e32 = R.block_err(r32, ref, blocks)
    print(f"n_pad {n_pad} N {N} peak {peak}: restatement {max(e.values()):.1e}, e32 {max(e32.values()):.1e}")
    assert max(e.values()) <= 1e-12, e
    assert max(e32.values()) < 1e-3, e32                   # the float32 yardstick is a yardstick: finite and small


def test_planted_errors_break_the_gpu_bound():
    """Every mutation exceeds bound(e32, K_CAP) by 10 x on a block of at least one of the kernel test's cases."""
    best = {m: (0.0, None) for m in MUTATIONS}
    for n_pad, N, peak in CASES:
        qkv, ops64, ref, r32, g = fused_case(n_pad, N, peak)
        blocks = cls_blocks(N, g["s"])
        e32 = R.block_err(r32, ref, blocks)
        for m in MUTATIONS:
            with torch.no_grad():
                em = R.block_err(cls_fused_ref(qkv, **ops64, pad=g["pad"], N=N, s=g["s"], mutate=m), ref, blocks)
            blk = max(em, key=lambda b: em[b] / R.bound(e32[b], R.K_CAP))
            margin = em[blk] / R.bound(e32[blk], R.K_CAP)
            print(f"planted {m:<9} case n_pad {n_pad} N {N:<5} peak {peak} margin {margin:11.1f}x on {blk:<8} (error {em[blk]:.1e}, "
                  f"e32 {e32[blk]:.1e})  <- {GPU}test_kernel_alone")
            if margin > best[m][0]:
                best[m] = (margin, (n_pad, N, peak))
            if m == "nofold" and g["add"] == 0:
                assert max(em.values()) == 0.0                # nothing to fold: this shape cannot see it
    for m, (margin, case) in best.items():
        assert margin >= MARGIN, (m, margin, case)


# --------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _header_args(name):
    """(return type, [argument types]) of a prototype of include/mil_hip.h, names stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mil_hip.h"
    args = [re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", a.strip()).strip() for a in m.group(2).split(",")]
    return m.group(1).strip(), args


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    assert "mil_tm_cls_attn_fused_ws_floats" in _lib.VALUE_RETURNING      # a size, not a status: no errcheck on it
    assert "mil_tm_cls_attn_fused" not in _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 14 and lib.mil_abi_version() == _lib.ABI_VERSION


def test_status_entry_refuses_bad_arguments_before_any_launch(lib):
    """Host memory stands in for every operand: an entry that launched would fault, one that refuses first never reads it."""
    buf = (ctypes.c_float * 72)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)             # 16-byte aligned, and 4-byte aligned only
    f = lib.mil_tm_cls_attn_fused
    good = dict(n_pad=512, pad=255, s=16, n=250)                          # geometry(250)

    def call(ptrs=None, len_dev=None, bag=0, **kw):
        a = dict(good, **kw)
        q, ql, kl, z, lse, ws, out = ptrs or (p,) * 7
        return f(q, ql, kl, z, lse, a["n_pad"], a["pad"], a["s"], a["n"], len_dev, bag, ws, out, None)

    for n_pad in (0, -256, 100, 257, 500):
        assert call(n_pad=n_pad, pad=n_pad - 257) == EINVAL, n_pad
    for pad in (254, 256, -1):                                            # pad + 1 + s^2 != n_pad
        assert call(pad=pad) == EINVAL, pad
    assert call(s=15) == EINVAL and call(s=0, pad=511) == EINVAL
    for i in range(7):                                                    # each pointer null
        ptrs = [p] * 7
        ptrs[i] = None
        assert call(ptrs=ptrs) == EINVAL, i
    for i in range(3):                                                    # qkv, qL, kL are read as float4
        ptrs = [p] * 7
        ptrs[i] = off
        assert call(ptrs=ptrs) == EINVAL, i
    for n in (225, 257, 0, -3, 5000):                                     # the host length outside ((s - 1)^2, s^2]
        assert call(n=n) == EINVAL, n
    assert call(len_dev=p, bag=-1) == EINVAL
    with pytest.raises(_lib.MilHipError):                                 # and through the checked handle it raises
        _lib.checked().mil_tm_cls_attn_fused(None, p, p, p, p, 512, 255, 16, 250, None, 0, p, p, None)
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_cls_attn_fused(p, p, p, p, p, 512, 255, 16, 257, None, 0, p, p, None)


def test_workspace_stays_below_one_map(lib):
    for n in (512, 2048, 7936, 15872):
        assert 0 < lib.mil_tm_cls_attn_fused_ws_floats(n) < 8 * 256 * n, n
        assert _lib.checked().mil_tm_cls_attn_fused_ws_floats(n) == lib.mil_tm_cls_attn_fused_ws_floats(n)
    for n in (100, 0, -256, 257):
        assert lib.mil_tm_cls_attn_fused_ws_floats(n) == 0, n


# --------------------------------------------------------------------------- the switch
def test_the_switch_truth_table(monkeypatch):
    """_tm_fused_cls over keyword x environment x need_attn: the keyword wins, None reads MIL_TM_FUSED_CLS at the call (default
    off), and the route applies with need_attn "cls" only.  The two pass switches stay off for "cls" and do not reach it."""
    from mil_amd import ops
    for kw, env, need in itertools.product((None, False, True), (None, "", "0", "1"), (False, True, "cls")):
        if env is None:
            monkeypatch.delenv("MIL_TM_FUSED_CLS", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_FUSED_CLS", env)
        on = kw if kw is not None else env == "1"
        assert ops._tm_fused_cls(kw, need) is (bool(on) and need == "cls"), (kw, env, need)
    monkeypatch.setenv("MIL_TM_FUSED_CLS", "0")
    monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
    monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    assert ops._tm_fused_cls(None, "cls") is False
    monkeypatch.setenv("MIL_TM_FUSED_CLS", "1")
    assert ops._tm_fused_cls(None, "cls") is True and ops._tm_fused_cls(None, False) is False
    assert ops._tm_fused_a1(None, "cls") is False and ops._tm_fused_a3(None, "cls") is False


def test_nystrom_core_and_the_module_take_the_switch():
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    qkv, w = torch.zeros((512, 1536)), torch.zeros((8, 1, 33, 1))
    for on in (True, False, None):
        with pytest.raises(_lib.MilHipError, match="no CPU path"):        # accepted: it gets as far as the device check
            ops.nystrom_core(qkv, w, "cls", pad=255, s=16, n=250, fused_cls=on)
    with pytest.raises(_lib.MilHipError, match="no CPU path"):
        ops.nystrom_core(qkv, w, False, fused_cls=True)
    with pytest.raises(ValueError):                                       # the geometry is still asked for
        ops.nystrom_core(qkv, w, "cls", fused_cls=True)
    assert ops.tm_cls_attention_fused is not None
    assert TransMIL(n_classes=2).fused_cls is None
