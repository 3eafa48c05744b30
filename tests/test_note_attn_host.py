"""CPU: the note's per-patch attention weights (model.note_attn; csrc/absorbed_attn.hip: mil_absorbed_pool_attn,
csrc/attn_pool.hip: mil_bag_softmax) as a definition - the restatement of tests/note_attn_ref.py against a plain softmax of
the unabsorbed scores, what the per-block bound of tests/test_gpu_note_attn.py sees, and the --save_note_attn flag."""
import math

import pytest
import torch

import note_attn_ref as R

LENS = [1, 63, 64, 65, 130]


def _unabsorbed_weights(c):
    """softmax over the bag of q_h . k_proj(keys + pe)_h / sqrt(C) (attn_ref.unabsorbed's kp; the projection's bias is a
    constant per softmax row and left out) -> [N, H]."""
    C, off = c["C"], c["k_off"]
    kp = (c["keys"] + R._pe_rows(c["pe"], off)) @ c["Wk"].t()
    out = torch.zeros((c["keys"].shape[0], R.H), dtype=torch.float64)
    for b in range(len(off) - 1):
        n = off[b + 1] - off[b]
        s = torch.einsum("hc,nhc->hn", c["qp"][b].reshape(R.H, C), kp[off[b]:off[b + 1]].reshape(n, R.H, C)) / math.sqrt(C)
        out[off[b]:off[b + 1]] = s.softmax(-1).t()
    return out


@pytest.mark.parametrize("C", [32, 64])
def test_restatement_is_the_softmax_of_the_unabsorbed_scores(C):
    c = R.absorbed_case(LENS, C)
    Qp = torch.einsum("bhc,hce->bhe", c["qp"].reshape(-1, R.H, C), c["Wk"].reshape(R.H, C, -1))
    _, lse = R.absorbed_pool(c["keys"], c["pe"], Qp, c["k_off"], C)
    got = R.absorbed_attention(c["keys"], c["pe"], Qp, lse, c["k_off"], C)
    assert float((got - _unabsorbed_weights(c)).abs().max()) <= 1e-12
    assert float((R.head_sums(got, c["k_off"]) - 1).abs().max()) <= 1e-12


def test_bag_softmax_restatement():
    off = R.offsets([1, 2, 1023])
    s = torch.randn(off[-1], generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    w = R.bag_softmax(s, off)
    assert float((w[1:3] - s[1:3].softmax(0)).abs().max()) <= 1e-15 and float(w[0]) == 1.0
    w = R.bag_softmax(s, off, [1, 1, 1000])
    assert float(w[2]) == 0.0 and bool((w[off[2] + 1000:] == 0).all()) and abs(float(w[off[2]:].sum()) - 1) <= 1e-12


@pytest.mark.parametrize("mutate,C", [(m, C) for m in R.MUTATIONS for C in (32, 64) if not (m == "scale_eh" and C == R.E // R.H)])
def test_planted_errors_break_the_stage_bound(mutate, C):
    """Each planted error leaves some (bag, tile, head) block 10 x or more beyond k x max(e32, 1e-7).  ("scale_eh" at C = 32
    only: 1 / sqrt(E / H) is the right scale when C = E / H.)"""
    c = R.absorbed_case(LENS, C)
    Qp, lse = R.fed(c)
    args = (c["pe"], Qp, lse, c["k_off"], C)
    ref = R.absorbed_attention(c["keys"], *args)
    r32 = R.absorbed_attention(c["keys"].float(), c["pe"].float(), Qp.float(), lse.float(), c["k_off"], C)
    bad = R.absorbed_attention(c["keys"], *args, mutate=mutate, prev_keys=c["dkeys_acc"])
    blocks = R.attn_blocks(c["k_off"])
    e32, em = R.block_err(r32, ref, blocks), R.block_err(bad, ref, blocks)
    assert all(e <= R.bound(e32[n], R.K_NOTE) for n, e in R.block_err(r32, ref, blocks).items())
    worst = max(em[n] / R.bound(e32[n], R.K_NOTE) for n in em)
    print(f"{mutate} C {C}: {worst:.1f} x the bound")
    assert worst >= 10


# --------------------------------------------------------------------------- the flag
ARGV = ["--variant", "fusion", "--modality", "['pathology']", "--clip_layers", "1"]


def test_config_accepts_save_note_attn_for_the_fusion_pathology_model(tmp_path):
    from mil_amd.config import create_arg_parser
    args = create_arg_parser([*ARGV, "--save_note_attn", str(tmp_path / "attn")])
    assert args.save_note_attn == str(tmp_path / "attn")
    assert create_arg_parser(ARGV).save_note_attn == ""
    # the weights come out of the eager forward: the flag switches the replayed evaluation off
    assert create_arg_parser([*ARGV, "--hip_graph", "1", "--save_note_attn", str(tmp_path / "attn")]).hip_graph == 0
    assert create_arg_parser([*ARGV, "--hip_graph", "1"]).hip_graph == 1


@pytest.mark.parametrize("extra", [["--variant", "image_only"], ["--modality", "['CT', 'pathology']"], ["--modality", "['CI']"]])
def test_config_refuses_save_note_attn_elsewhere(extra, tmp_path):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    with pytest.raises(ValueError, match="save_note_attn"):
        create_arg_parser([*ARGV, *extra, "--save_note_attn", str(tmp_path / "attn")])
    args = create_arg_parser([*ARGV, *extra])
    args.save_note_attn = str(tmp_path / "attn")
    if args.variant == "image_only" or "CT" not in args.modality:       # builds on the CPU: refused by build_model too
        with pytest.raises(ValueError, match="save_note_attn"):
            train_ddp.build_model(args)


def test_build_model_sets_the_switch(tmp_path):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    args = create_arg_parser([*ARGV, "--save_note_attn", str(tmp_path / "attn")])
    model = train_ddp.build_model(args)
    assert model.note_attn and model.last_note_attn is None and model.last_bag_attn is None and (tmp_path / "attn").is_dir()
    model.flush_note_attn()                               # nothing kept: nothing written
    assert not list((tmp_path / "attn").iterdir())
    args.save_note_attn = ""
    assert not train_ddp.build_model(args).note_attn
