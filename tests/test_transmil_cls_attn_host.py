"""CPU: the per-patch cls-token attention of TransMIL (need_attn="cls", csrc/transmil.hip: mil_tm_cls_attn) as a definition.

With P = A1 Z A3 the [8, n_pad, n_pad] map of one Nystrom layer (tests/transmil_ref.py: core), pad = n_pad - s^2 - 1 the cls row:
    a[h, i] = P[h, pad, pad + 1 + i] + (i < add ? P[h, pad, pad + 1 + N + i] : 0),   0 <= i < N, add = s^2 - N
cls_attn_ref states that from the three factors without the map; here it is held against the folded cls row of the float64
restatement's own map, the planted errors of the project's sensitivity convention (test_transmil_sensitivity_host.py) are shown
to break the GPU bound of tests/test_gpu_transmil_cls_attn.py by 10 x, and the entry point's flag is refused where it has no
meaning.  The helpers are shared with the GPU test; nothing here reads the code under test except the CLI check."""
import functools

import pytest
import torch
import torch.nn.functional as F

import transmil_ref as R

MARGIN = 10.0
GPU = "tests/test_gpu_transmil_cls_attn.py::"
MUTATIONS = ("nofold", "row", "shift", "zT")


def cls_attn_ref(a1, z, a3, pad, N, s, mutate=None):
    """a1 [8, n_pad, 256], z [8, 256, 256], a3 [8, 256, n_pad] (any float dtype) -> [8, N].  mutate: a planted error -
    "nofold": the repeats' keys dropped; "row": row pad - 1 instead of the cls row; "shift": columns one to the left, so the
    cls column leaks in; "zT": Z transposed."""
    assert mutate is None or mutate in MUTATIONS, mutate
    add = s * s - N
    assert pad + 1 + s * s == a3.shape[-1] and 0 <= add < 2 * s
    row = pad - 1 if mutate == "row" else pad
    zz = z.transpose(-1, -2) if mutate == "zT" else z
    t = torch.einsum("hk,hkj->hj", a1[:, row], zz)
    r = torch.einsum("hm,hmc->hc", t, a3)
    c0 = pad if mutate == "shift" else pad + 1
    out = r[:, c0:c0 + N].clone()
    if mutate != "nofold":
        out[:, :add] += r[:, c0 + N:c0 + N + add]
    return out


def fold_cls_row(P, pad, N, s):
    """The same out of a whole map P [8, n_pad, n_pad]."""
    row = P[:, pad, pad + 1:]
    assert row.shape[-1] == s * s
    out = row[:, :N].clone()
    out[:, :s * s - N] += row[:, N:]
    return out


def cls_blocks(N, s):
    """[8, N]: each head, the first and last 16 patches, the patches the square padding repeats (i < add)."""
    out = {f"head{h}": (h,) for h in range(R.H)}
    out.update({"first16": (slice(None), slice(0, min(16, N))), "last16": (slice(None), slice(max(0, N - 16), N)),
                "folded": (slice(None), slice(0, s * s - N))})
    return out


def core_pieces(qkv):
    """(a1, z, a3) by the formulas of R.core."""
    n_pad = qkv.shape[0]
    q, k, _ = qkv.chunk(3, dim=-1)
    q, k = (t.reshape(-1, R.H, R.DH).transpose(0, 1) for t in (q, k))
    q = q * R.DH ** -0.5
    l = n_pad // R.M
    qL = q.reshape(R.H, R.M, l, R.DH).sum(2) / l
    kL = k.reshape(R.H, R.M, l, R.DH).sum(2) / l
    a1 = (q @ kL.transpose(-1, -2)).softmax(-1)
    a2 = (qL @ kL.transpose(-1, -2)).softmax(-1)
    a3 = (qL @ k.transpose(-1, -2)).softmax(-1)
    return a1, R.pinv(a2), a3


def transmil_cls(xb, p, keeps=None):
    """R.transmil layer by layer with the cls attention taken from the factors: (h [512], [a0, a1]) in xb's dtype."""
    N = xb.shape[0]
    g = R.geometry(N)
    h = F.relu(xb @ p["_fc1.0.weight"].t() + p["_fc1.0.bias"])
    h = torch.cat([p["cls_token"].reshape(1, -1), h, h[:g["add"]]], 0)
    attns = []
    for i, layer in enumerate(("layer1", "layer2")):
        if i == 1:
            h = R.ppeg(h, g["s"], p)
        ln = F.layer_norm(h, (h.shape[1],), p[f"{layer}.norm.weight"], p[f"{layer}.norm.bias"], 1e-5)
        qkv = F.pad(ln, (0, 0, g["pad"], 0)) @ p[f"{layer}.attn.to_qkv.weight"].t()
        attns.append(cls_attn_ref(*core_pieces(qkv), g["pad"], N, g["s"]))
        o, _ = R.nystrom(ln, p[f"{layer}.attn.to_qkv.weight"], p[f"{layer}.attn.to_out.0.weight"], p[f"{layer}.attn.to_out.0.bias"],
                         p[f"{layer}.attn.res_conv.weight"], None if keeps is None else keeps[i])
        h = h + o
    return F.layer_norm(h[:1], (h.shape[1],), p["norm.weight"], p["norm.bias"], 1e-5)[0], attns


def restated(x, p, keeps=None, dtype=torch.float64):
    """[a0, a1] of one bag: the folded cls rows of R.transmil's own maps, everything in `dtype` (float64: the reference;
    float32: e32 of the GPU bound)."""
    N, g = x.shape[0], R.geometry(x.shape[0])
    pp = {k: v.to(dtype) for k, v in p.items()}
    kk = None if keeps is None else [k.to(dtype) for k in keeps]
    with torch.no_grad():
        _, maps = R.transmil(x.to(dtype), pp, kk, return_attn=True)
    return [fold_cls_row(m, g["pad"], N, g["s"]) for m in maps]


def cls_case(n_pad, N):
    """Inputs of the kernel-alone test, float32-exact and held in float64: row-softmaxed randn A1 and A3, Z randn / 16
    (spectral norm about 2)."""
    g = torch.Generator().manual_seed(7 * n_pad + N)
    a1 = torch.randn((R.H, n_pad, R.M), generator=g).softmax(-1)
    a3 = torch.randn((R.H, R.M, n_pad), generator=g).softmax(-1)
    z = torch.randn((R.H, R.M, R.M), generator=g) / 16
    return a1.double(), z.double(), a3.double()


# (n_pad, N): l = 1, 2, 5; pad = 246, 255 (n_pad 256 / 512 / 1280); add = 2, 6, 0, 24 and the side's maximum 62 (N = 962)
KERNEL_SHAPES = [(256, 7), (512, 250), (512, 256), (1280, 1000), (1280, 962)]


@functools.lru_cache(maxsize=None)
def kernel_case(n_pad, N):
    g = R.geometry(N)
    assert g["n_pad"] == n_pad
    a1, z, a3 = cls_case(n_pad, N)
    ref = cls_attn_ref(a1, z, a3, g["pad"], N, g["s"])
    r32 = cls_attn_ref(a1.float(), z.float(), a3.float(), g["pad"], N, g["s"])
    return (a1, z, a3), ref, r32, g


def test_shapes_cover_what_the_kernel_branches_on():
    geo = [R.geometry(N) for _, N in KERNEL_SHAPES]
    assert [g["n_pad"] for g in geo] == [n for n, _ in KERNEL_SHAPES]
    assert {g["l"] for g in geo} == {1, 2, 5} and {g["pad"] for g in geo} == {246, 255}
    assert [g["add"] for g in geo] == [2, 6, 0, 24, 62] and geo[4]["add"] == 2 * geo[4]["s"] - 2
    assert {g["s"] % 2 for g in geo} == {0, 1} and any(g["n_pad"] % 512 for g in geo)      # 16-byte and 4-byte loads


@functools.lru_cache(maxsize=None)
def _bag(N):
    from mil_amd import synthetic as syn
    p = {k: v.double() for k, v in syn.transmil_params(11, 768, 2).items()}
    return torch.randn((N, 768), generator=torch.Generator().manual_seed(N), dtype=torch.float64), p


@pytest.mark.parametrize("N", [7, 250, 256, 1000])
def test_restatement_from_the_factors_equals_the_folded_cls_row_of_the_map(N):
    x, p = _bag(N)
    with torch.no_grad():
        h, got = transmil_cls(x, p)
        h_ref, _ = R.transmil(x, p)
    ref = restated(x, p)
    assert float((h - h_ref).abs().max()) <= 1e-12 * float(h_ref.abs().max())
    for layer in range(2):
        assert got[layer].shape == (R.H, N)
        e = R.block_err(got[layer], ref[layer], cls_blocks(N, R.geometry(N)["s"]))
        print(f"N {N} layer {layer}: {max(e.values()):.1e}, sum over patches {float(ref[layer].sum(-1).mean()):.3f}, "
              f"min {float(ref[layer].min()):.2e}")
        assert max(e.values()) <= 1e-12, e


def test_planted_errors_break_the_gpu_bound():
    """Every mutation exceeds k_cap x max(e32, 1e-7) by 10 x on a block of at least one of the kernel test's shapes."""
    best = {m: (0.0, None) for m in MUTATIONS}
    for n_pad, N in KERNEL_SHAPES:
        (a1, z, a3), ref, r32, g = kernel_case(n_pad, N)
        blocks = cls_blocks(N, g["s"])
        e32 = R.block_err(r32, ref, blocks)
        for m in MUTATIONS:
            em = R.block_err(cls_attn_ref(a1, z, a3, g["pad"], N, g["s"], mutate=m), ref, blocks)
            blk = max(em, key=lambda b: em[b] / R.bound(e32[b], R.K_CAP))
            margin = em[blk] / R.bound(e32[blk], R.K_CAP)
            print(f"planted {m:<7} case n_pad {n_pad} N {N:<5} margin {margin:9.1f}x on {blk:<8} (error {em[blk]:.1e}, "
                  f"e32 {e32[blk]:.1e})  <- {GPU}test_kernel_alone")
            if margin > best[m][0]:
                best[m] = (margin, (n_pad, N))
            if m == "nofold" and g["add"] == 0:
                assert max(em.values()) == 0.0                # nothing to fold: this shape cannot see it
    for m, (margin, case) in best.items():
        assert margin >= MARGIN, (m, margin, case)


@pytest.mark.parametrize("extra", [["--variant", "image_only", "--model_pathology", "ABMIL"],
                                   ["--variant", "fusion", "--model_pathology", "ABMIL"],
                                   ["--variant", "fusion", "--model_pathology", "TransMIL"]])
def test_save_patch_attn_is_refused_outside_image_only_transmil(extra, tmp_path, monkeypatch):
    """The flag is refused where the arguments are read (config.create_arg_parser, which test_ddp.py's entry calls first) and
    again by build_model for arguments built by hand - both before anything touches the GPU."""
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flag must be refused before any GPU work"))
    argv = [*extra, "--synthetic", "[300, 768, 4]"]
    with pytest.raises(ValueError, match="save_patch_attn"):
        create_arg_parser([*argv, "--save_patch_attn", str(tmp_path / "attn")])
    args = create_arg_parser(argv)
    assert args.save_patch_attn == ""
    args.save_patch_attn = str(tmp_path / "attn")
    if args.model_pathology == "ABMIL":                   # the pinned refusals of aggregator="TransMIL" come first otherwise
        with pytest.raises(ValueError, match="save_patch_attn"):
            train_ddp.build_model(args)
    assert not (tmp_path / "attn").exists()


def test_build_model_with_save_patch_attn_sets_the_model_up(tmp_path):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    args = create_arg_parser(["--variant", "image_only", "--model_pathology", "TransMIL", "--synthetic", "[300, 768, 4]",
                              "--save_patch_attn", str(tmp_path / "attn")])
    model = train_ddp.build_model(args)
    assert model.patch_attn and (tmp_path / "attn").is_dir()
    model.flush_patch_attn()                               # nothing kept: nothing written
    assert list((tmp_path / "attn").iterdir()) == []
    args.save_patch_attn = ""
    assert not train_ddp.build_model(args).patch_attn
