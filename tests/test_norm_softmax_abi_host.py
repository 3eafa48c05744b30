"""CPU: the C-ABI side of the LayerNorm, softmax, row-broadcast and token front/back entries on the built library, no GPU -
they are declared, exported and bound alike; a bad argument is refused with MIL_EINVAL before any launch; an empty problem
returns 0 without touching anything; and the workspace size of the column softmax follows its documented plan."""
import ctypes
import os
import re

import pytest

from mil_amd import _lib

EINVAL = -22
NAMES = ("mil_layernorm_fwd", "mil_layernorm_bwd_blocks", "mil_layernorm_bwd", "mil_layernorm_bwd_res", "mil_layernorm_bagrow_fwd",
         "mil_layernorm_bagrow_bwd", "mil_layernorm_bagrow_rows_per_block", "mil_grp_col_softmax", "mil_grp_col_softmax_bwd",
         "mil_grp_col_softmax_workspace_floats", "mil_grp_col_softmax_ws", "mil_grp_col_softmax_bwd_ws", "mil_row_softmax_t",
         "mil_row_softmax_t_bwd", "mil_add_pe", "mil_add_bag_row", "mil_segment_colsum", "mil_embed_tokens", "mil_gather_eot")
VALUES = ("mil_layernorm_bwd_blocks", "mil_layernorm_bagrow_rows_per_block", "mil_grp_col_softmax_workspace_floats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.fixture()
def p():
    """A host buffer that no entry may read or write: every call below returns before a launch.  Filled with a pattern that
    is checked afterwards."""
    buf = (ctypes.c_float * 256)(*([-12345.678] * 256))
    yield ctypes.cast(buf, ctypes.c_void_p)
    assert all(v == buf[0] for v in buf), "a refused or empty call wrote its operand"


def _header_args(name):
    """(return type, [argument types]) of a prototype of include/mil_hip.h, names stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/mil_hip.h"
    args = [re.sub(r"\s*[A-Za-z_][A-Za-z0-9_]*$", "", a.strip()).strip() for a in m.group(2).split(",")]
    return m.group(1).strip(), args


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name in NAMES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
        assert (name in _lib.VALUE_RETURNING) == (name in VALUES), name     # a count or a size, not a status: no errcheck


def _ln_fwd(L, p, rows=4, E=64, x=True, gamma=True, beta=True, y=True):
    q = lambda on: p if on else None                                                         # noqa: E731
    return L.mil_layernorm_fwd(q(x), q(gamma), q(beta), rows, E, 1e-5, q(y), p, None)


def _ln_bagrow_fwd(L, p, rows=4, E=64, o=True, row_bag=True):
    q = lambda on: p if on else None                                                         # noqa: E731
    return L.mil_layernorm_bagrow_fwd(p, q(o), q(row_bag), p, p, rows, E, 1e-5, p, p, None)


def _ln_bwd_res(L, p, rows=4, E=64, x=True, gamma=True, dy=True, stats=True, dx=True, dgamma=True, dbeta=True, ws=True):
    q = lambda on: p if on else None                                                         # noqa: E731
    return L.mil_layernorm_bwd_res(q(x), q(gamma), q(dy), q(stats), None, rows, E, q(dx), q(dgamma), q(dbeta), q(ws), None)


def _ln_bwd(L, p, rows=4, E=64, dgamma=True, dbeta=True, ws=True):
    q = lambda on: p if on else None                                                         # noqa: E731
    return L.mil_layernorm_bwd(p, p, p, p, rows, E, p, q(dgamma), q(dbeta), q(ws), None)


def _ln_bagrow_bwd(L, p, rows=64, E=64, B=2, **off):
    names = ("x", "o", "row_bag", "row_off", "gamma", "dy", "stats", "dx", "d_o", "dgamma", "dbeta", "ws")
    a = {n: (None if off.get(n) is False else p) for n in names}
    return L.mil_layernorm_bagrow_bwd(a["x"], a["o"], a["row_bag"], a["row_off"], B, a["gamma"], a["dy"], a["stats"], rows, E, a["dx"],
                                      a["d_o"], a["dgamma"], a["dbeta"], a["ws"], None)


def test_layernorm_refuses_bad_arguments_before_any_launch(lib, p):
    L = lib
    for name in ("x", "gamma", "beta", "y"):
        assert _ln_fwd(L, p, **{name: False}) == EINVAL, name
    assert _ln_bagrow_fwd(L, p, o=False) == EINVAL and _ln_bagrow_fwd(L, p, row_bag=False) == EINVAL
    for E in (0, 96, 576):                                          # not a positive multiple of 64 up to 512
        assert _ln_fwd(L, p, E=E) == EINVAL and _ln_bagrow_fwd(L, p, E=E) == EINVAL, E
        assert _ln_bwd_res(L, p, E=E) == EINVAL and _ln_bwd(L, p, E=E) == EINVAL and _ln_bagrow_bwd(L, p, E=E) == EINVAL, E
    for rows in (4, 100):                                           # E = 192 has no kernel, forward or backward
        assert _ln_bwd_res(L, p, rows=rows, E=192) == EINVAL and _ln_bwd(L, p, rows=rows, E=192) == EINVAL, rows
    assert _ln_fwd(L, p, E=192) == EINVAL and _ln_bagrow_bwd(L, p, E=192) == EINVAL
    for name in ("x", "gamma", "dy", "stats", "dx"):
        assert _ln_bwd_res(L, p, **{name: False}) == EINVAL, name
    assert _ln_bwd_res(L, p, dbeta=False) == EINVAL and _ln_bwd_res(L, p, dgamma=False) == EINVAL        # one without the other
    assert _ln_bwd_res(L, p, ws=False) == EINVAL and _ln_bwd_res(L, p, rows=100, ws=False) == EINVAL    # trainable: workspace
    assert _ln_bwd(L, p, dgamma=False, dbeta=False) == EINVAL and _ln_bwd(L, p, ws=False) == EINVAL     # the plain entry: all three
    for name in ("x", "o", "row_bag", "row_off", "gamma", "dy", "stats", "dx", "d_o", "dgamma", "dbeta", "ws"):
        assert _ln_bagrow_bwd(L, p, **{name: False}) == EINVAL, name
    assert _ln_fwd(L, p, rows=-1) == EINVAL and _ln_bwd_res(L, p, rows=-1) == EINVAL and _ln_bagrow_bwd(L, p, rows=-1) == EINVAL
    with pytest.raises(_lib.MilHipError):                           # and through the checked handle it raises
        _lib.checked().mil_layernorm_fwd(None, p, p, 4, 64, 1e-5, p, p, None)


def test_softmax_refuses_bad_arguments_before_any_launch(lib, p):
    L = lib
    col = lambda S=p, off=p, ld=32, TH=24, G=1: L.mil_grp_col_softmax(S, ld, off, G, 100, TH, None)                        # noqa: E731
    colw = lambda S=p, off=p, ld=32, TH=24, G=1: L.mil_grp_col_softmax_ws(S, ld, off, G, 100, TH, p, None)                 # noqa: E731
    colb = lambda A=p, dA=p, dS=p, off=p, ld=32, TH=24, G=1: L.mil_grp_col_softmax_bwd(A, dA, ld, off, G, 100, TH, dS, None)  # noqa: E731
    colbw = lambda A=p, dA=p, dS=p, off=p, ld=32, TH=24, G=1: L.mil_grp_col_softmax_bwd_ws(A, dA, ld, off, G, 100, TH, dS, p, None)  # noqa: E731
    for f in (col, colw):
        assert f(S=None) == EINVAL and f(off=None) == EINVAL
    for f in (colb, colbw):
        assert f(A=None) == EINVAL and f(dA=None) == EINVAL and f(dS=None) == EINVAL and f(off=None) == EINVAL
    for f in (col, colw, colb, colbw):
        assert f(TH=33) == EINVAL and f(TH=0) == EINVAL and f(ld=0) == EINVAL and f(G=-1) == EINVAL, f
    row = lambda S=p, ld=128, R=4, T=10, H=8: L.mil_row_softmax_t(S, ld, R, T, H, None)                                      # noqa: E731
    rowb = lambda A=p, dA=p, dS=p, ld=128, R=4, T=10, H=8: L.mil_row_softmax_t_bwd(A, dA, ld, R, T, H, dS, None)             # noqa: E731
    assert row(S=None) == EINVAL and rowb(A=None) == EINVAL and rowb(dA=None) == EINVAL and rowb(dS=None) == EINVAL
    for f in (row, rowb):
        assert f(T=17, ld=256) == EINVAL and f(T=0) == EINVAL and f(T=10, ld=79) == EINVAL and f(T=16, ld=96) == EINVAL, f
        assert f(H=0) == EINVAL and f(R=-1) == EINVAL, f


def test_elementwise_entries_refuse_bad_arguments_before_any_launch(lib, p):
    L = lib
    q = lambda i, j: None if i == j else p                                                   # noqa: E731
    for j in range(5):
        assert L.mil_add_pe(q(0, j), q(1, j), q(2, j), q(3, j), 4, 64, q(4, j), None) == EINVAL, j
    for j in range(4):
        assert L.mil_add_bag_row(q(0, j), q(1, j), q(2, j), 4, 64, q(3, j), None) == EINVAL, j
        assert L.mil_embed_tokens(q(0, j), q(1, j), q(2, j), 2, 5, 64, q(3, j), None) == EINVAL, j
    for j in range(3):
        assert L.mil_segment_colsum(q(0, j), q(1, j), 2, 10, 64, q(2, j), None, None) == EINVAL, j
        assert L.mil_gather_eot(q(0, j), q(1, j), 2, 5, 64, q(2, j), None) == EINVAL, j
    for E in (0, 6, -4):                                            # float4 rows
        assert L.mil_add_pe(p, p, p, p, 4, E, p, None) == EINVAL and L.mil_add_bag_row(p, p, p, 4, E, p, None) == EINVAL, E
        assert L.mil_embed_tokens(p, p, p, 2, 5, E, p, None) == EINVAL, E
    assert L.mil_embed_tokens(p, p, p, 2, 0, 64, p, None) == EINVAL and L.mil_gather_eot(p, p, 2, 0, 64, p, None) == EINVAL
    assert L.mil_segment_colsum(p, p, -1, 10, 64, p, None, None) == EINVAL and L.mil_segment_colsum(p, p, 2, 10, 0, p, None, None) == EINVAL


def test_empty_problems_return_ok_and_touch_nothing(lib, p):
    L = lib
    assert _ln_fwd(L, p, rows=0) == 0 and _ln_bagrow_fwd(L, p, rows=0) == 0                       # rows = 0
    assert L.mil_add_pe(p, p, p, p, 0, 64, p, None) == 0 and L.mil_add_bag_row(p, p, p, 0, 64, p, None) == 0
    assert L.mil_embed_tokens(p, p, p, 0, 5, 64, p, None) == 0 and L.mil_gather_eot(p, p, 0, 5, 64, p, None) == 0
    assert L.mil_grp_col_softmax(p, 32, p, 0, 0, 24, None) == 0 and L.mil_grp_col_softmax_ws(p, 32, p, 0, 4000, 24, p, None) == 0   # G = 0
    assert L.mil_grp_col_softmax_bwd(p, p, 32, p, 0, 0, 24, p, None) == 0
    assert L.mil_grp_col_softmax_bwd_ws(p, p, 32, p, 0, 4000, 24, p, p, None) == 0
    assert L.mil_row_softmax_t(p, 128, 0, 10, 8, None) == 0 and L.mil_row_softmax_t_bwd(p, p, 128, 0, 10, 8, p, None) == 0             # R = 0
    assert L.mil_segment_colsum(p, p, 0, 0, 64, p, p, None) == 0                                                                      # B = 0


def test_col_softmax_workspace_follows_its_plan(lib):
    """0 exactly when the one-launch form is taken (G > 8, max_group_rows <= 2048, ld < 32 or ld > 128), else
    G min(64, ceil(max_group_rows / 256)) 2 ld."""
    f = lib.mil_grp_col_softmax_workspace_floats
    for G in (1, 2, 3, 8, 9, 64):
        for m in (0, 1, 2048, 2049, 2304, 2305, 4000, 16384, 16385, 16500, 40000):
            for ld in (8, 31, 32, 40, 96, 128, 129, 256):
                one_launch = G > 8 or m <= 2048 or ld < 32 or ld > 128
                want = 0 if one_launch else G * min(64, -(-m // 256)) * 2 * ld
                assert f(G, m, ld) == want and (f(G, m, ld) == 0) == one_launch, (G, m, ld)
