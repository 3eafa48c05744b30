"""CPU: what the per-block bounds of tests/test_gpu_transmil_stages.py can see.

The GPU bound of a block is k x max(e32, 1e-7), k <= 16, with e32 the error of the float32 restatement of the same stage
on the CPU against float64 (tests/transmil_ref.py).  Here every planted error (the mutate= switches of the restatement: a
backward branch dropped, a tap lost, a border treated wrongly ...) is measured in float64 against the clean float64 result
with the GPU tests' own inputs and blocks, and has to exceed the bound at the cap k = 16 by a factor of 10 on at least one
block - so a kernel that made that error could not pass.  COVER names the GPU test that holds each planted error; the
printout (pytest -s) lists the achieved margins.  Nothing here reads the code under test."""
import math

import pytest
import torch

import transmil_ref as R

MARGIN = 10.0
STAGES = "tests/test_gpu_transmil_stages.py::"


def margin(mut, ref, r32, blocks):
    """(largest planted error / bound at the cap over the blocks, that block)"""
    e32 = R.flat_err(r32, ref, blocks)
    em = R.flat_err(mut, ref, blocks)
    best = max(em, key=lambda b: em[b] / R.bound(e32[b], R.K_CAP))
    return em[best] / R.bound(e32[best], R.K_CAP), best, em[best], e32[best]


def report(rows):
    for name, cover, case, m, blk, em, e32 in rows:
        print(f"planted {name:<22} case {case:<14} margin {m:9.1f}x on {blk:<16} (error {em:.1e}, e32 {e32:.1e})  <- {cover}")


# planted error of the whole core -> the shapes of test_nystrom_core at which it must show
CORE_COVER = {
    "pinv_detach": (256, 512, 2048, 7936),      # whole pseudo-inverse backward dropped
    "z0_detach": (256, 512, 2048, 7936),        # Z0 backward dropped (mil_tm_pinv_init_bwd, both halves)
    "qL_detach": (256, 512, 2048, 7936),        # landmark backward of q dropped
    "kL_detach": (256, 512, 2048, 7936),        # landmark backward of k dropped
    "scale_detach": (256,),                     # gradient of the pinv scale dropped: elsewhere held by test_pinv_init
    "scale_per_head": (2048,),                  # forward: scale per head instead of over the 8 heads
}


@pytest.mark.parametrize("n_pad", [256, 512, 2048, 7936])
def test_core_planted_errors_break_the_block_bounds(n_pad):
    qkv, w, dO, pad = R.core_case(n_pad)
    blocks = R.core_blocks(n_pad, pad)
    ref, r32 = R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32)
    rows = []
    for mut, shapes in CORE_COVER.items():
        m, blk, em, e32 = margin(R.core_run(qkv, w, dO, mutate=mut), ref, r32, blocks)
        rows.append((mut, STAGES + f"test_nystrom_core[{n_pad}-1.0]", f"n_pad {n_pad}", m, blk, em, e32))
        if n_pad in shapes:
            assert m >= MARGIN, (mut, n_pad, m, blk)
    report(rows)
    # the whole-tensor norm these blocks stand next to: dv dwarfs dq and dk, so one norm over dqkv is a statement about dv
    g = ref["dqkv"]
    assert g[:, 1024:].norm() > 5 * g[:, :512].norm()


@pytest.mark.parametrize("n_pad", [512, 7936])
def test_peaked_core_case_is_well_posed(n_pad):
    """The input with q and k scaled by PEAK: the A1 rows are visibly peaked, the float32 restatement stays accurate, and
    the six pseudo-inverse iterations get as far as on the unscaled input (residual of A2 Z A2 = A2 0.03 .. 0.10 there)."""
    qkv, w, dO, pad = R.core_case(n_pad, R.PEAK)
    qL, kL = R.landmarks(qkv, n_pad // R.M)
    q = qkv[:, :512].reshape(-1, R.H, R.DH).transpose(0, 1) * R.DH ** -0.5
    a1 = (q[:, pad:] @ kL.transpose(-1, -2)).softmax(-1)
    a2 = (qL @ kL.transpose(-1, -2)).softmax(-1)
    z = R.pinv(a2)
    res = float((a2 @ z @ a2 - a2).norm() / a2.norm())
    peak = float(a1.amax(-1).mean())
    e32 = R.flat_err(R.core_run(qkv, w, dO, torch.float32), R.core_run(qkv, w, dO), R.core_blocks(n_pad, pad))
    print(f"peaked n_pad {n_pad}: mean row max of A1 {peak:.3f} (uniform: {1 / 256:.4f}), pinv residual {res:.3f}, "
          f"worst e32 {max(e32.values()):.1e}")
    assert peak > 20 / 256 and res < 0.11 and max(e32.values()) < 1e-4


def test_pinv_init_planted_errors():
    a2, dZ = R.pinv_case()
    blocks = {"Z0": R.whole(), "dS2": R.whole()}
    ref, r32 = R.pinv_run(a2, dZ), R.pinv_run(a2, dZ, torch.float32)
    assert ref["arg"] == 3 * 256 + 77 and r32["arg"] == ref["arg"]
    rows = []
    for mut in ("scale_detach", "z0_detach", "scale_per_head"):
        m, blk, em, e32 = margin(R.pinv_run(a2, dZ, mutate=mut), ref, r32, blocks)
        rows.append((mut, STAGES + "test_pinv_init", "A2 softmaxed", m, blk, em, e32))
        assert m >= MARGIN, (mut, m, blk)
    report(rows)
    # the row-sum factor: its gradient is constant along a row and leaves with the softmax backward (the kernel omits it)
    a = a2.clone().requires_grad_(True)
    s = a.abs().sum(-2).max()                                   # column sums only
    (a.transpose(-1, -2) / (a.abs().sum(-1).max().detach() * s)).backward(dZ)
    only_col = R.softmax_rows_bwd(a2, a.grad)
    assert R.block_err(only_col, ref["dS2"], R.whole())["all"] < 1e-6


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 257, 7936])
def test_softmax_bwd_planted_error(cols):
    rows = []
    for nrows in (1, 5):
        x, dp = R.softmax_case(nrows, cols)
        p = R.softmax_rows(x)
        assert torch.isfinite(p).all() and bool((p[torch.isinf(x)] == 0).all())
        ref = {"dp": R.softmax_rows_bwd(p, dp)}
        p32 = R.softmax_rows(x.float())
        r32 = {"dp": R.softmax_rows_bwd(p32, dp.float())}
        m, blk, em, e32 = margin({"dp": R.softmax_rows_bwd(p, dp, mutate="nodot")}, ref, r32, {"dp": R.whole()})
        rows.append(("softmax_bwd nodot", STAGES + "test_softmax_rows", f"{nrows} x {cols}", m, blk, em, e32))
        assert m >= MARGIN
    report(rows)


@pytest.mark.parametrize("n", [1, 16, 33, 255, 256, 257, 600, 7936])
def test_resconv_planted_errors(n):
    c = R.resconv_case(n)
    ref, r32 = R.resconv_run(c), R.resconv_run(c, torch.float32)
    rows = []
    for mut in ("tap", "lastrow"):
        m, blk, em, e32 = margin(R.resconv_run(c, mutate=mut), ref, r32, R.resconv_blocks(n))
        rows.append(("resconv " + mut, STAGES + "test_resconv", f"n {n}", m, blk, em, e32))
        if mut == "lastrow" or n >= 16:                       # tap 5 reads row i - 11: no such row below n = 12
            assert m >= MARGIN, (mut, n, m)
    report(rows)
    # the explicit taps against autograd of the reference's own form of the layer
    qkv = c["qkv"].clone().requires_grad_(True)
    w = c["w"].clone().requires_grad_(True)
    v = qkv[:, 1024:].reshape(-1, R.H, R.DH).transpose(0, 1)
    out = torch.nn.functional.conv2d(v.unsqueeze(0), w.reshape(R.H, 1, R.CONV, 1), padding=(R.CONV // 2, 0), groups=R.H)[0]
    out = out.transpose(0, 1).reshape(n, 512)
    out.backward(c["dout"])
    _, dv, dw = R.resconv_bwd(c["dout"], c["qkv"], c["w"])
    assert torch.allclose(out, R.resconv(c["qkv"], c["w"]), rtol=0, atol=1e-12)
    assert torch.allclose(dv, qkv.grad[:, 1024:], rtol=0, atol=1e-12) and torch.allclose(dw, w.grad, rtol=0, atol=1e-9)


@pytest.mark.parametrize("s", [1, 2, 3, 7, 8, 9, 16, 17, 125])
def test_ppeg_planted_errors(s):
    p, x, dy = R.ppeg_case(s)
    blocks = R.ppeg_all_blocks(s)
    ref, r32 = R.ppeg_run(p, x, dy, s), R.ppeg_run(p, x, dy, s, torch.float32)
    assert torch.allclose(ref["y"], R.ppeg(x, s, p), rtol=0, atol=1e-12)     # the folded form is the layer
    rows = []
    for mut in ("offcentre", "clamp"):
        m, blk, em, e32 = margin(R.ppeg_run(p, x, dy, s, mutate=mut), ref, r32, blocks)
        rows.append(("ppeg " + mut, STAGES + "test_ppeg", f"s {s}", m, blk, em, e32))
        assert m >= MARGIN, (mut, s, m)
    report(rows)
    if s >= 7:
        assert set(R.block_err(ref["y"], ref["y"], blocks["y"])) == {"cls", "ring", "interior"}


@pytest.mark.parametrize("K", [1, 7, 17, 100, 64, 7936])
def test_bgemm_planted_error(K):
    rows = []
    for Mr, Nc in ((1, 1), (63, 65), (130, 130)):
        A, B, D = R.bgemm_case(2, Mr, Nc, K)
        ref = {"C": R.bgemm(A, B, 0.5, -7.0, D, 15.0)}
        r32 = {"C": R.bgemm(A.float(), B.float(), 0.5, -7.0, D.float(), 15.0)}
        m, blk, em, e32 = margin({"C": R.bgemm(A, B, 0.5, -7.0, D, 15.0, mutate="ktail")}, ref, r32,
                                 {"C": R.bgemm_blocks(Mr, Nc)})
        rows.append(("bgemm ktail", STAGES + "test_bgemm", f"{Mr}x{Nc}x{K}", m, blk, em, e32))
        assert m >= MARGIN, (K, Mr, Nc, m)
    report(rows)


def test_block_err_and_seq_index():
    ref = torch.zeros(4, 4, dtype=torch.float64)
    ref[0, 0] = 2.0
    got = ref.clone()
    got[3, 3] = 1e-3
    e = R.block_err(got, ref, {"all": (Ellipsis,), "tail": (slice(2, 4),), "none": (slice(0, 0),)})
    assert e["all"] == 5e-4 and math.isinf(e["tail"]) and "none" not in e      # an all-zero block must be met exactly
    assert R.block_err(ref, ref, {"tail": (slice(2, 4),)})["tail"] == 0.0
    assert R.seq_index([7, 250], [3, 16]) == ([-2] + list(range(7)) + [0, 1] + [-2] + list(range(7, 257)) + list(range(7, 13)), 257, 0)
    assert R.seq_index([3], [3]) == ([-2] + list(range(5)) + list(range(4)), 5, 1)      # below the bucket: clamped, flagged
