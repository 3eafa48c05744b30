"""CPU: what the replayed TransMIL step is keyed by and what its device-side index kernel must write - the grid-side bucket
function and the per-entry index expression of model/dim1/TransMIL.py against the list `forward` builds - plus the new
switch and the C-ABI entry."""
import argparse
import ctypes
import os

import pytest


def _forward_list(lengths):
    """The list TransMIL.forward has always built on the host, restated literally."""
    import math
    idx, off = [], 0
    for n in lengths:
        s = int(math.ceil(math.sqrt(n)))
        add = s * s - n
        idx += [-2] + list(range(off, off + n)) + list(range(off, off + add))
        off += n
    return idx


def test_bucket_side_is_the_geometry_side_for_every_length():
    from mil_amd.model.dim1.TransMIL import bucket_side, geometry, side_geometry
    for N in range(1, 16001):
        s = bucket_side(N)
        assert (s - 1) ** 2 < N <= s * s, N
        g = geometry(N)
        assert s == g["s"], N
        if N in (1, 2, 7, 250, 1000, 2000, 7600, 15592) or N % 997 == 0:
            sg = side_geometry(s)
            assert all(sg[k] == g[k] for k in ("s", "seq", "n_pad", "l", "pad")), N
    with pytest.raises(ValueError):
        bucket_side(0)


@pytest.mark.parametrize("lengths", [[1], [7], [250], [1000], [1937], [2025], [15592], [7, 1000, 250]])
def test_index_expression_reproduces_the_forward_list(lengths):
    from mil_amd.model.dim1.TransMIL import bucket_side, seq_index, seq_index_entry
    want = _forward_list(lengths)
    assert seq_index(lengths) == want
    got, off = [], 0
    for n in lengths:
        s = bucket_side(n)
        got += [seq_index_entry(j, n, off) for j in range(1 + s * s)]
        off += n
    assert got == want
    assert len(want) == sum(1 + bucket_side(n) ** 2 for n in lengths)
    assert max(want) == sum(lengths) - 1 and min(want) == -2


def test_pad_index_depends_on_the_side_only():
    from mil_amd.model.dim1.TransMIL import geometry, pad_index, side_geometry
    for N in (1937, 1990, 2025):                                  # one side, s = 45
        assert pad_index(geometry(N)) == pad_index(side_geometry(45))
    p = pad_index(side_geometry(16))
    assert p[:255] == [-1] * 255 and p[255:] == list(range(257))


def test_switch_exists_and_defaults_off():
    from mil_amd.config import create_arg_parser
    base = ["--variant", "image_only", "--model_pathology", "TransMIL", "--synthetic", "[300, 768, 6]"]
    assert create_arg_parser(base).transmil_graph == 0
    assert create_arg_parser(base + ["--transmil_graph", "1"]).transmil_graph == 1


def test_switch_is_refused_for_other_models_before_gpu_work(monkeypatch):
    from mil_amd import train_ddp
    monkeypatch.setattr(train_ddp, "env_world", lambda: (1, 0, 0))
    args = argparse.Namespace(variant="image_only", model_pathology="ABMIL", multiprocessing_distributed=False,
                              fused_step=False, hip_graph=0, transmil_graph=1)
    with pytest.raises(ValueError, match="transmil_graph"):
        train_ddp.main_worker(0, 1, args)


def test_abi_declares_and_exports_the_index_entry():
    from mil_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert "mil_tm_seq_index" in _lib.header_symbols() and "mil_tm_seq_index" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "mil_tm_seq_index")


def test_stepper_module_imports_without_a_gpu():
    from mil_amd.transmil_step import DEFAULT_MAX_GRAPHS, RaggedTransMILStepper
    assert callable(RaggedTransMILStepper) and DEFAULT_MAX_GRAPHS >= 1
