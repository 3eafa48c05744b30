"""CPU: the C-ABI side of the fused token-query pass (csrc/token_attn.hip) on the built library, no GPU - the three entries are
declared, exported and bound alike; the status entries refuse a bad n_pad or a null pointer before any launch; the workspace
stays below one [8, n_pad, 256] map; and nystrom_core takes the switch."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from mil_amd import _lib

EINVAL = -22
NAMES = ("mil_tm_tok_attn_ws_floats", "mil_tm_tok_attn_fwd", "mil_tm_tok_attn_bwd")


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
    assert "mil_tm_tok_attn_ws_floats" in _lib.VALUE_RETURNING           # a size, not a status: no errcheck on it
    assert _lib.ABI_VERSION >= 13 and lib.mil_abi_version() == _lib.ABI_VERSION


def test_status_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                         # never read: the entries return first
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n_pad in (0, -256, 100, 257):
        assert lib.mil_tm_tok_attn_fwd(p, p, p, n_pad, p, p, p, None) == EINVAL, n_pad
        assert lib.mil_tm_tok_attn_bwd(p, p, p, p, p, n_pad, p, p, p, p, None) == EINVAL, n_pad
    assert lib.mil_tm_tok_attn_fwd(None, p, p, 256, p, p, p, None) == EINVAL
    assert lib.mil_tm_tok_attn_bwd(None, p, p, p, p, 256, p, p, p, p, None) == EINVAL
    assert lib.mil_tm_tok_attn_bwd(p, p, p, p, p, 256, p, p, p, None, None) == EINVAL      # the backward's workspace is not empty
    with pytest.raises(_lib.MilHipError):                                 # and through the checked handle it raises
        _lib.checked().mil_tm_tok_attn_fwd(None, p, p, 256, p, p, p, None)


def test_workspace_stays_below_one_map(lib):
    for n in (512, 2048, 7936, 15872):
        assert 0 < lib.mil_tm_tok_attn_ws_floats(n, 1) < 8 * 256 * n, n
        assert 0 <= lib.mil_tm_tok_attn_ws_floats(n, 0) < 8 * 256 * n, n
    for n in (100, 0, -256, 257):
        assert lib.mil_tm_tok_attn_ws_floats(n, 0) == 0 and lib.mil_tm_tok_attn_ws_floats(n, 1) == 0, n


def test_nystrom_core_takes_the_switch():
    from mil_amd import ops
    qkv, w = torch.zeros((256, 1536)), torch.zeros((8, 1, 33, 1))
    for need_attn in (False, True):
        for a3 in (False, True):
            with pytest.raises(_lib.MilHipError, match="no CPU path"):    # accepted: it gets as far as the device check
                ops.nystrom_core(qkv, w, need_attn, fused_a1=True, fused_a3=a3)
    assert ops.tm_tok_attn is not None and ops.tm_tok_attn_bwd is not None


def test_the_switch_truth_table(monkeypatch):
    """_tm_fused_a1 over keyword x environment x need_attn: the keyword wins, None reads MIL_TM_FUSED_A1 at the call (default
    off), and the route applies with need_attn False only."""
    from mil_amd import ops
    for kw, env, need in itertools.product((None, False, True), (None, "", "0", "1"), (False, True, "cls")):
        if env is None:
            monkeypatch.delenv("MIL_TM_FUSED_A1", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_FUSED_A1", env)
        on = kw if kw is not None else env == "1"
        assert ops._tm_fused_a1(kw, need) is (bool(on) and need is False), (kw, env, need)
    monkeypatch.setenv("MIL_TM_FUSED_A1", "0")
    monkeypatch.setenv("MIL_TM_FUSED_A3", "1")                            # the other switch does not reach this one
    assert ops._tm_fused_a1(None, False) is False and ops._tm_fused_a3(None, False) is True
