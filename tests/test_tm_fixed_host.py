"""CPU: the host side of the fixed-order TransMIL sums (mil_tm_*_fixed) on the built library, no GPU - the entries are declared,
exported and bound alike; the workspace sizes follow their formulas; the status entries refuse bad arguments before any
launch; the two index writers name no source row more than twice (what keeps the gather's backward on its two-term path);
the switch resolves keyword, then attribute, then environment; config.py parses --deterministic and build_model sets it."""
import argparse
import ctypes
import itertools
import os

import pytest
import torch

import tm_fixed_ref as F
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_entries_are_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in F.FIXED + F.WS:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES, name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
        res, args = _header_args(name)
        want = [] if args in ([""], ["void"]) else [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[res], want), (name, res, args)
    assert set(F.WS) <= _lib.VALUE_RETURNING                           # sizes, not statuses: no errcheck on them
    assert not set(F.FIXED) & _lib.VALUE_RETURNING
    assert _lib.ABI_VERSION >= 16 and lib.mil_abi_version() == _lib.ABI_VERSION
    # a fixed entry takes its atomic twin's arguments plus the workspace (the gather: plus the extent of dsrc; the
    # pseudo-inverse's twin has a workspace argument already, one float there, 256 here)
    more = {"mil_tm_row_gather_bwd": 2, "mil_tm_pinv_init_bwd": 0, "mil_tm_resconv_bwd": 1, "mil_tm_ppeg_bwd": 1}
    for name in F.ATOMIC:
        old, new = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_fixed"][1]
        assert len(new) == len(old) + more[name], name
    assert len(_lib.SIGNATURES["mil_tm_bgemm_fixed"][1]) == len(_lib.SIGNATURES["mil_tm_bgemm"][1]) + 1


def test_workspace_sizes_match_their_formulas(lib):
    for batch, M, N, splits in itertools.product((1, 8), (1, 130, 256), (1, 64, 7936), (1, 2, 5, 16)):
        assert lib.mil_tm_bgemm_ws_floats(batch, M, N, splits) == F.ws_floats("mil_tm_bgemm_ws_floats", batch, M, N, splits)
    assert lib.mil_tm_bgemm_ws_floats(8, 256, 64, 16) == 16 * 8 * 256 * 64
    assert lib.mil_tm_bgemm_ws_floats(8, 256, 64, 1) == 0 and lib.mil_tm_bgemm_ws_floats(0, 256, 64, 4) == 0
    for n in (-1, 0, 1, 9, 15592, 16000):
        assert lib.mil_tm_row_gather_ws_floats(n) == F.ws_floats("mil_tm_row_gather_ws_floats", n)
    assert lib.mil_tm_pinv_ws_floats() == 256
    for n in (-256, 0, 1, 255, 256, 257, 512, 1280, 15872):
        assert lib.mil_tm_resconv_ws_floats(n) == F.ws_floats("mil_tm_resconv_ws_floats", n), n
    assert lib.mil_tm_resconv_ws_floats(1280) == 5 * 8 * 33
    for s in (-1, 0, 1, 3, 8, 9, 18, 125):
        assert lib.mil_tm_ppeg_ws_floats(s) == F.ws_floats("mil_tm_ppeg_ws_floats", s), s
    assert lib.mil_tm_ppeg_ws_floats(9) == 2 * 50 * 512


def test_status_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                      # never read: the entries return first
    p = ctypes.cast(buf, ctypes.c_void_p)
    st = (64, 8, 1)
    assert lib.mil_tm_bgemm_fixed(p, *st, p, *st, p, *st, None, 1, 8, 8, 8, 1.0, 0.0, 0.0, 2, None, None) == EINVAL    # no workspace
    assert lib.mil_tm_bgemm_fixed(p, *st, p, *st, p, *st, None, 1, 8, 8, 8, 1.0, 0.0, 0.0, 0, p, None) == EINVAL
    assert lib.mil_tm_bgemm_fixed(None, *st, p, *st, p, *st, None, 1, 8, 8, 8, 1.0, 0.0, 0.0, 1, None, None) == EINVAL  # via mil_tm_bgemm
    assert lib.mil_tm_bgemm_fixed(p, *st, p, *st, p, *st, None, 2, 8, 8, 8, 1.0, 0.0, 0.0, 32768, p, None) == EINVAL
    assert lib.mil_tm_row_gather_bwd_fixed(p, p, 4, 8, p, 0, None, p, None) == EINVAL
    assert lib.mil_tm_row_gather_bwd_fixed(p, p, 4, 8, p, 4, None, None, None) == EINVAL
    assert lib.mil_tm_row_gather_bwd_fixed(p, p, 0, 8, p, 4, None, p, None) == EINVAL
    assert lib.mil_tm_pinv_init_bwd_fixed(p, p, p, p, p, None, None) == EINVAL
    assert lib.mil_tm_resconv_bwd_fixed(p, p, p, 256, p, p, None, None) == EINVAL
    assert lib.mil_tm_resconv_bwd_fixed(p, p, p, 0, p, p, p, None) == EINVAL
    assert lib.mil_tm_ppeg_bwd_fixed(p, p, 3, p, p, p, p, p, p, None, None) == EINVAL
    assert lib.mil_tm_ppeg_bwd_fixed(p, p, 0, p, p, p, p, p, p, p, None) == EINVAL
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_tm_ppeg_bwd_fixed(p, p, 3, p, p, p, p, p, p, None, None)


def test_index_writers_name_no_source_row_more_than_twice():
    """seq_index over every N in 1 .. 16 000 (add = s^2 - N <= N rows are repeated once), segment_table's index for bags cut
    into pieces: the count the gather's backward meets per source row is 0, 1 or 2, never more."""
    from mil_amd.model.dim1.TransMIL import bucket_side, seq_index, seq_index_segments
    for N in range(1, 16001):
        s = bucket_side(N)
        add = s * s - N
        assert 0 <= add <= N, N                                        # (s - 1)^2 < N: s^2 - N < 2 s - 1 <= N for every N >= 1
    for N in list(range(1, 300)) + [1000, 2000, 7600, 15592, 16000]:
        idx = seq_index([N])
        assert idx.count(-2) == 1 and F.max_naming(idx, N) <= 2, N
    lengths = [7, 300, 250, 1, 2]
    assert F.max_naming(seq_index(lengths), sum(lengths)) <= 2
    for N in list(range(1, 120)) + [1000, 15592]:
        cut = [N // 3, N // 2]                                         # three pieces, out of order in memory
        segs = [[(cut[1], N - cut[1]), (0, cut[0]), (cut[0], cut[1] - cut[0])]]
        idx = seq_index_segments(segs, x_rows=N)
        assert F.max_naming(idx, N) <= 2 and idx.count(-2) == 1, N


def test_the_switch_keyword_then_attribute_then_environment(monkeypatch):
    from mil_amd import ops
    from mil_amd.model.dim1 import TransMIL
    for kw, env in itertools.product((None, False, True), (None, "", "0", "1")):
        if env is None:
            monkeypatch.delenv("MIL_TM_DETERMINISTIC", raising=False)
        else:
            monkeypatch.setenv("MIL_TM_DETERMINISTIC", env)
        assert ops.tm_deterministic(kw) is bool(kw if kw is not None else env == "1"), (kw, env)
    # the module resolves the switch once per forward - the attribute, else the environment as it stands at that call - and
    # hands every op that one bool as the keyword.  The ops are replaced by shape-only stand-ins that note it: one eval forward
    # on the CPU reaches the sequence gather, both layers' pad gather and core, and PPEG.
    net = TransMIL(n_classes=2, L=768).eval()
    assert net.deterministic is None
    seen = []

    def gather(src, extra, idx, deterministic=None):
        seen.append(("gather", deterministic))
        return torch.zeros((idx.numel(), src.shape[1]))

    def core(qkv, w, need_attn=False, deterministic=None, **kw):
        seen.append(("core", deterministic))
        return torch.zeros((qkv.shape[0], 512)), None

    def ppeg(x, s, W7, b7, W5, b5, W3, b3, deterministic=None):
        seen.append(("ppeg", deterministic))
        return x

    monkeypatch.setattr(ops, "tm_row_gather", gather)
    monkeypatch.setattr(ops, "nystrom_core", core)
    monkeypatch.setattr(ops, "tm_ppeg", ppeg)
    monkeypatch.setattr(ops, "layer_norm", lambda x, w, b, eps: x)
    monkeypatch.setattr(ops, "linear_act", lambda x, W, b, act=None, residual=None, rows_dev=None: torch.zeros((x.shape[0], W.shape[0])))
    for attr, env in itertools.product((None, True, False), ("0", "1")):
        net.deterministic = attr
        monkeypatch.setenv("MIL_TM_DETERMINISTIC", env)
        want = attr if attr is not None else env == "1"
        seen.clear()
        net(torch.zeros((7, 768)), [7])
        assert seen == [(k, want) for k in ("gather", "gather", "core", "ppeg", "gather", "core")], (attr, env, seen)
        assert all(v is want for _, v in seen)                          # a bool, never None: no op reads the environment again


def test_ops_take_the_keyword():
    from mil_amd import ops
    qkv, w = torch.zeros((256, 1536)), torch.zeros((8, 1, 33, 1))
    for det in (None, False, True):
        with pytest.raises(_lib.MilHipError, match="no CPU path"):     # accepted: it gets as far as the device check
            ops.nystrom_core(qkv, w, deterministic=det)
        with pytest.raises(_lib.MilHipError, match="no CPU path"):
            ops.tm_row_gather(torch.zeros((4, 8)), None, torch.zeros(4, dtype=torch.int32), deterministic=det)
        with pytest.raises(_lib.MilHipError, match="no CPU path"):
            ops.tm_ppeg(torch.zeros((10, 512)), 3, *[torch.zeros(1)] * 6, deterministic=det)


def test_config_parses_the_flag_and_build_model_sets_it():
    from mil_amd.config import create_arg_parser
    from mil_amd.train_ddp import build_model
    from test_gpu_fusion_transmil import make_args
    assert create_arg_parser(["--deterministic", "1"]).deterministic == 1
    assert create_arg_parser([]).deterministic == 0
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only",
                              deterministic=1)
    assert build_model(args).extractor_pathology.deterministic is True
    args.deterministic = 0
    assert build_model(args).extractor_pathology.deterministic is None
    fus = build_model(make_args(variant="fusion", model_pathology="TransMIL", deterministic=1))
    mods = [m for m in fus.modules() if type(m).__name__ == "TransMIL"]
    assert len(mods) == 2 and all(m.deterministic is True for m in mods)          # the aggregator and the unused extractor
    args = argparse.Namespace(modality=["pathology"], model_pathology="ABMIL", num_classes=2, patch_dim=768, variant="image_only",
                              deterministic=1)
    assert not [m for m in build_model(args).modules() if type(m).__name__ == "TransMIL"]      # accepted, nothing to set
