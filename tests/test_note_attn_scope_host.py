"""CPU: the host side of `model.note_attn = "all"` / --note_attn_scope all - the flag and what it lifts, build_model, the new
entry mil_bag_softmax_rows declared, exported and bound alike at ABI 23 and refusing bad arguments before any launch, its
restatement (tests/note_attn_bucket_ref.py) against note_attn_ref.bag_softmax, what the per-block bound of
tests/test_gpu_bag_softmax_rows.py sees of two planted errors, and the steppers' keys."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import note_attn_bucket_ref as Q
import note_attn_ref as R
from mil_amd import _lib
from test_token_attn_abi_host import _header_args

EINVAL = -22
NAME = "mil_bag_softmax_rows"
ARGV = ["--variant", "fusion", "--clip_layers", "1"]
CT_PTH = ["--modality", "['CT', 'pathology']"]
TM = ["--aggregator", "TransMIL", "--fusion_transmil", "1", "--fusion_transmil_graph", "1", "--flat_adam", "1"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# --------------------------------------------------------------------------- the flag
def test_the_scope_defaults_to_pathology():
    from mil_amd.config import create_arg_parser
    assert create_arg_parser(ARGV).note_attn_scope == "pathology"
    assert create_arg_parser([*ARGV, "--note_attn_scope", "all"]).note_attn_scope == "all"
    with pytest.raises(SystemExit):
        create_arg_parser([*ARGV, "--note_attn_scope", "CT"])


def test_scope_all_lifts_the_three_refusals(tmp_path):
    from mil_amd.config import create_arg_parser
    save = ["--save_note_attn", str(tmp_path / "attn"), "--note_attn_scope", "all"]
    for modality in ("['pathology']", "['CT']", "['CT', 'pathology']"):
        args = create_arg_parser([*ARGV, "--modality", modality, *save])
        assert args.save_note_attn == str(tmp_path / "attn") and args.note_attn_scope == "all"
    args = create_arg_parser([*ARGV, *CT_PTH, "--hip_graph", "1", *save])
    assert args.hip_graph == 1                                   # the weights come out of the replayed forward: it stays on
    assert create_arg_parser([*ARGV, "--modality", "['pathology']", "--hip_graph", "1", *save]).hip_graph == 1
    for modality in ("['pathology']", "['CT', 'pathology']"):
        args = create_arg_parser([*ARGV, "--modality", modality, *TM, *save])
        assert args.fusion_transmil_graph == 1 and args.save_note_attn


@pytest.mark.parametrize("extra", [["--variant", "image_only"], ["--modality", "['CI']"]])
def test_scope_all_still_refuses_ci_and_image_only(extra, tmp_path):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    with pytest.raises(ValueError, match="save_note_attn"):
        create_arg_parser([*ARGV, "--modality", "['pathology']", *extra, "--save_note_attn", str(tmp_path / "a"),
                           "--note_attn_scope", "all"])
    args = create_arg_parser([*ARGV, "--modality", "['pathology']", *extra, "--note_attn_scope", "all"])
    args.save_note_attn = str(tmp_path / "a")
    with pytest.raises(ValueError, match="save_note_attn"):
        train_ddp.build_model(args)


def test_build_model_sets_the_scope(tmp_path):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    base = [*ARGV, "--modality", "['pathology']", "--save_note_attn", str(tmp_path / "attn")]
    model = train_ddp.build_model(create_arg_parser([*base, "--note_attn_scope", "all"]))
    assert model.note_attn == "all" and model._note_all() and (tmp_path / "attn").is_dir()
    assert model.last_note_attn is None and model.last_note_attn_ct is None and model.last_bag_attn is None
    model = train_ddp.build_model(create_arg_parser(base))
    assert model.note_attn is True and not model._note_all()       # the default scope: today's switch
    args = create_arg_parser([*ARGV, "--modality", "['pathology']", "--note_attn_scope", "all"])
    assert train_ddp.build_model(args).note_attn is False          # the scope alone exports nothing


# --------------------------------------------------------------------------- the entry
def test_entry_is_declared_exported_and_bound_alike(lib):
    ctype = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    assert NAME in _lib.header_symbols() and NAME in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported"
    res, args = _header_args(NAME)
    want = [ctypes.c_void_p if a.endswith("*") else ctype[a] for a in args]
    assert _lib.SIGNATURES[NAME] == (ctype[res], want), (res, args)
    ptr, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES[NAME][1] == [ptr, ptr, ptr, i, ptr, i, i, ptr, ptr]     # scores, map, off, T, row_bag, B, R, w, stream
    assert NAME not in _lib.VALUE_RETURNING                        # a status: checked() raises on it
    assert _lib.ABI_VERSION >= 23 and lib.mil_abi_version() == _lib.ABI_VERSION


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_float * 64)()                                  # never read: the entry returns first
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = [p, p, p, 4, p, 1, 33, p, None]
    for hole in (0, 1, 2, 4, 7):
        a = list(good)
        a[hole] = None
        assert lib.mil_bag_softmax_rows(*a) == EINVAL, hole
    for at, bad in ((3, -1), (5, -1), (5, 1025), (6, -1)):
        a = list(good)
        a[at] = bad
        assert lib.mil_bag_softmax_rows(*a) == EINVAL, (at, bad)
    with pytest.raises(_lib.MilHipError):
        _lib.checked().mil_bag_softmax_rows(p, p, p, 4, p, 1025, 33, p, None)


def test_ops_bag_softmax_takes_the_bucket_face():
    """On the CPU the bucket face gets as far as the device check: it used to raise NotImplementedError for its lengths."""
    from mil_amd import ops
    face = SimpleNamespace(device_lengths=True, lengths=None, B=1, R=257, T=9, tile_map=torch.zeros((9, 4), dtype=torch.int32),
                           bag_tile_off=torch.zeros(2, dtype=torch.int32), row_bag=lambda: torch.zeros(257, dtype=torch.int32))
    with pytest.raises(_lib.MilHipError, match="no CPU path"):
        ops.bag_softmax(torch.zeros(257), face)


# --------------------------------------------------------------------------- the restatement
def test_restatement_is_the_per_bag_softmax_on_a_two_segment_layout():
    """[cap patch rows | B token rows]: gathered bag by bag, the restatement is note_attn_ref.bag_softmax of the gathered scores."""
    cap, tail, lengths = 256, [1], [130, 70]
    rb = Q.row_bag(cap, tail, lengths)
    assert rb.numel() == 258 and rb[:200].tolist() == [0] * 130 + [1] * 70 and bool((rb[200:256] == -1).all())
    assert rb[256:].tolist() == [0, 1]
    perm, off = Q.bag_order(rb, 2)
    assert off == [0, 131, 202] and perm[130] == 256 and perm[-1] == 257
    for dt, tol in ((torch.float64, 1e-15), (torch.float32, 1e-7)):
        s = Q.scores_for("normal", rb, 2, 1).to(dt)
        w = Q.bag_softmax_rows(s, rb, 2)
        assert w.dtype == dt and bool((w[rb < 0] == 0).all()) and bool(torch.isfinite(w).all())
        want = R.bag_softmax(s[perm], off)
        assert float((w[perm] - want).abs().max()) <= tol
        assert float((torch.stack([w[rb == b].sum() for b in range(2)]) - 1).abs().max()) <= 2 * tol * 131
    # the four-segment bag of CT + pathology: patches, CT-side text token, CT tokens, pathology-side text token
    rb = Q.row_bag(512, [1, 4, 1], [130, 70, 200])
    perm, off = Q.bag_order(rb, 3)
    assert off == [0, 136, 212, 418] and perm[130:136].tolist() == [512, 515, 516, 517, 518, 527]


@pytest.mark.parametrize("mutate", Q.MUTATIONS)
@pytest.mark.parametrize("kind", ["normal", "equal"])
def test_planted_errors_break_the_stage_bound(mutate, kind):
    """Each planted error leaves some block of the GPU test's check 10 x or more beyond k x max(e32, 1e-7)."""
    cap, tail, lengths = Q.CASES[2]
    B = len(lengths)
    rb = Q.row_bag(cap, tail, lengths)
    perm, off = Q.bag_order(rb, B)
    s = Q.scores_for(kind, rb, B, 2)
    ref = Q.bag_softmax_rows(s, rb, B)[perm]
    r32 = Q.bag_softmax_rows(s.float(), rb, B)[perm].double()
    bad = Q.bag_softmax_rows(s, rb, B, mutate=mutate)[perm]
    blocks = R.softmax_blocks(off)
    e32, em = R.block_err(r32, ref, blocks), R.block_err(bad, ref, blocks)
    assert all(e <= R.bound(e32[n], R.K_NOTE) for n, e in e32.items())
    worst = max(em[n] / R.bound(e32[n], R.K_NOTE) for n in em)
    print(f"{mutate} {kind}: {worst:.1f} x the bound")
    assert worst >= 10


# --------------------------------------------------------------------------- the steppers' keys
def test_the_export_never_shares_a_graph_key():
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1 import TransMIL
    agg = TransMIL(2)
    model = SimpleNamespace(aggregator=agg, training=False, note_attn=False)
    me = SimpleNamespace(model=model, backward=False, sides=lambda lengths: tuple(lengths))
    key = lambda: RaggedFusionTransMILStepper.key(me, 256, (15,))      # noqa: E731
    off = key()
    assert "note_attn" not in off
    model.note_attn = True                                         # today's switch never reaches the stepper
    assert key() == off
    model.note_attn = "all"
    assert key() != off and key()[:len(off)] == off and key()[-2:] == ("note_attn", "all")
    me.backward = True                                             # the training step is not touched
    on_train = key()
    model.note_attn = False
    assert key() == on_train and "note_attn" not in on_train
    me.backward, model.training, model.note_attn = False, True, "all"
    assert "note_attn" not in key()
