"""CPU: the host side of the split-bf16 TransMIL products (mil_tm_bgemm_pieces, ops pieces=3 / MIL_TM_PIECES=3 /
--tm_gemm_pieces 3) on the built library, no GPU - the two entries are declared, exported and bound alike; the keyword, the
attribute, the environment switch and the command-line flag resolve as documented; the route rule names the products it
should; and a float32 emulation of the arithmetic (exact three-piece split, six cross terms, fp32 sums) stays inside the
bound the GPU tests use on the very inputs they use, so that those inputs are fair."""
import argparse
import ctypes
import inspect
import os

import pytest
import torch

import tm_pieces_ref as P
import transmil_ref as R
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

ENTRIES = ("mil_tm_bgemm_pieces", "mil_tm_bgemm_pieces_fixed")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in ENTRIES:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        assert _lib.SIGNATURES[name] == (ctype[res], [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]), name
        assert name not in _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 17 and lib.mil_abi_version() == _lib.ABI_VERSION
    # the arguments of the fp32 twin with `pieces` in front of the workspace / the stream
    for twin, name in (("mil_tm_bgemm", ENTRIES[0]), ("mil_tm_bgemm_fixed", ENTRIES[1])):
        old, new = _lib.SIGNATURES[twin][1], _lib.SIGNATURES[name][1]
        assert new[:21] == old[:21] and new[21] is ctypes.c_int and new[22:] == old[21:], name


def test_keyword_attribute_and_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1.TransMIL import TransLayer, TransMIL
    assert inspect.signature(ops.tm_bgemm).parameters["pieces"].default == 0
    assert inspect.signature(ops.nystrom_core).parameters["pieces"].default is None
    assert inspect.signature(ops._tm_fwd).parameters["pieces"].default == 0
    assert inspect.signature(ops._tm_pinv_bwd).parameters["pieces"].default == 0
    assert "route" in inspect.signature(TransLayer.run).parameters      # the layer takes the step's resolved route ...
    net = TransMIL(2)
    assert net.gemm_pieces is None
    monkeypatch.delenv("MIL_TM_PIECES", raising=False)
    assert ops.tm_route(net, 1, False).pieces == 0                      # ... which carries the attribute, else the environment
    net.gemm_pieces = 3
    assert ops.tm_route(net, 1, False).pieces == 3 and ops.tm_route(net, 2, "cls").pieces == 3
    monkeypatch.setenv("MIL_TM_PIECES", "3")
    net.gemm_pieces = None
    assert ops.tm_route(net, 1, True).pieces == 3
    net.gemm_pieces = 0
    assert ops.tm_route(net, 1, True).pieces == 0
    monkeypatch.delenv("MIL_TM_PIECES")
    assert ops.tm_pieces() == 0 and ops.tm_pieces(3) == 3 and ops.tm_pieces(0) == 0
    monkeypatch.setenv("MIL_TM_PIECES", "3")
    assert ops.tm_pieces() == 3 and ops.tm_pieces(0) == 0               # the keyword wins over the environment
    monkeypatch.setenv("MIL_TM_PIECES", "0")
    assert ops.tm_pieces() == 0
    monkeypatch.setenv("MIL_TM_PIECES", "")
    assert ops.tm_pieces() == 0
    for bad in ("2", "1", "4", "three"):
        monkeypatch.setenv("MIL_TM_PIECES", bad)
        with pytest.raises(ValueError):
            ops.tm_pieces()
        with pytest.raises(ValueError):                                 # read per call, before anything touches the GPU
            ops.nystrom_core(torch.zeros((256, 1536)), torch.zeros((8, 1, 33, 1)))
    monkeypatch.delenv("MIL_TM_PIECES")
    for bad in (2, 1, 4, True):
        with pytest.raises(ValueError):
            ops.tm_pieces(bad)
    with pytest.raises(ValueError):
        ops.tm_bgemm(None, (0, 0, 0), None, (0, 0, 0), None, (0, 0, 0), 1, 1, 1, 1, pieces=2)


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--tm_gemm_pieces", "3"]).tm_gemm_pieces == 3
    assert create_arg_parser([]).tm_gemm_pieces == 0
    with pytest.raises(SystemExit):
        create_arg_parser(["--tm_gemm_pieces", "2"])
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_gemm_pieces=3)
    assert build_model(args).extractor_pathology.gemm_pieces == 3
    args.tm_gemm_pieces = 0
    assert build_model(args).extractor_pathology.gemm_pieces is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", tm_gemm_pieces=3))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.gemm_pieces == 3 for m in mods)
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              tm_gemm_pieces=3)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set


@pytest.mark.parametrize("n", [256, 7936])
def test_route_rule_on_the_products_of_one_core_call(n):
    """(M, N, K) of every product _tm_fwd, _tm_bwd and _tm_pinv_bwd issue at n_pad = n: the K = 64 products stay on the fp32
    kernel, everything else goes to the split-bf16 one."""
    from mil_amd import ops
    m, d = 256, 64
    fp32 = {"A1": (n, m, d), "A2": (m, m, d), "A3": (m, n, d), "dA1": (n, m, d), "dZ": (m, m, d), "dA3": (m, n, d)}
    pieces = {"W": (m, d, n), "pinv": (m, m, m), "U": (m, d, m), "O": (n, d, m), "T": (n, m, m), "attn": (n, n, m), "dU": (m, d, n),
              "dW": (m, d, m), "dv": (n, d, m), "dq": (n, d, m), "dkL": (m, d, n), "dkL2": (m, d, m), "dqL": (m, d, m),
              "dqL3": (m, d, n), "dk": (n, d, m)}
    for name, shape in fp32.items():
        assert ops._tm_pieces_route(*shape) is False, name
    for name, shape in pieces.items():
        assert ops._tm_pieces_route(*shape) is True, name


# --------------------------------------------------------------------------- the arithmetic, emulated in float32 on the CPU
def test_split3_is_exact_and_adds_no_nan():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * torch.logspace(-20, 20, 4096)
    p = P.split3(x)
    assert torch.equal((p[0].double() + p[1].double() + p[2].double()).float(), x)
    for q in p:
        assert torch.equal(q.bfloat16().float(), q)
    assert len(P.TERMS) == 6 and all(a + b <= 2 for a, b in P.TERMS) and P.TERMS[-1] == (0, 0)


@pytest.mark.parametrize("K", [7, 100, 7936])
def test_emulated_product_is_inside_the_bound(K):
    A, B, D = R.bgemm_case(2, 65, 63, K)
    ref, r32, emu = R.bgemm(A, B), R.bgemm(A.float(), B.float()), P.bgemm_split3(A, B)
    blocks = {"C": R.bgemm_blocks(65, 63)}
    e32, ee = R.flat_err({"C": r32}, {"C": ref}, blocks), R.flat_err({"C": emu}, {"C": ref}, blocks)
    for b in ee:
        print(f"RATIO | pieces emulation | 65x63x{K} | {b} | emu {ee[b]:.2e} | e32 {e32[b]:.2e} | {ee[b] / max(e32[b], R.FLOOR):.2f}")
        assert ee[b] <= R.bound(e32[b], P.K_STAGE["bgemm"]), (b, ee[b], e32[b])


def test_emulated_pseudo_inverse_chain_is_inside_the_bound():
    """24 products deep: the six iterations on the emulation against transmil_ref.pinv in float64, per head."""
    a2, _ = R.pinv_case()
    ref, r32, emu = R.pinv(a2), R.pinv(a2.float()), P.pinv_split3(a2)
    e32, ee = R.block_err(r32, ref, P.head_blocks()), R.block_err(emu, ref, P.head_blocks())
    for b in ee:
        print(f"RATIO | pieces emulation | pinv chain | {b} | emu {ee[b]:.2e} | e32 {e32[b]:.2e} | {ee[b] / max(e32[b], R.FLOOR):.2f}")
        assert ee[b] <= R.bound(e32[b], P.K_STAGE["pinv_chain"]), (b, ee[b], e32[b])
