"""Test-side helpers of the split-bf16 TransMIL products (mil_tm_bgemm_pieces, ops pieces=3) that tests/transmil_ref.py does
not hold: the stage bounds, a float32 CPU emulation of the arithmetic (exact three-piece split, six cross terms, fp32 sums) and
the pseudo-inverse chain on that emulation."""
import torch

import transmil_ref as R

# k of bound(e32, k) per stage, by transmil_ref's rule: every stage started at K_CAP = 16; after the first full run on an
# MI355X each k is the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) seen, never above K_CAP
# (docs/lab_notes.md, "TransMIL split-bf16 products: ratio table").  That run's largest ratios: bgemm 3.13 (K = 7936, split-K
# with an empty split), bgemm_fixed 2.38, pinv_chain 1.93 (Z, head 5), core 8.80 (n_pad 2048, the first 16 rows of out, whose
# e32 is 2.6e-7) -> 8, 8, 4 and 2 x 8.80 -> 32 -> the cap.  A ratio that needs more than 16 is a defect to find, not grounds
# to lift the cap.
K_STAGE = {"bgemm": 8, "bgemm_fixed": 8, "pinv_chain": 4, "core": 16}
assert max(K_STAGE.values()) <= R.K_CAP


def hold(stage, tag, got, ref, r32, blocks):
    """transmil_ref.hold with this file's K_STAGE: every block within bound(e32, k), each ratio printed first."""
    e32, eg = R.flat_err(r32, ref, blocks), R.flat_err(got, ref, blocks)
    bad, worst = [], 0.0
    for b, e in eg.items():
        ratio = e / max(e32[b], R.FLOOR)
        worst = max(worst, ratio)
        print(f"RATIO | pieces {stage} | {tag} | {b} | gpu {e:.2e} | e32 {e32[b]:.2e} | {ratio:.2f}")
        if not e <= R.bound(e32[b], K_STAGE[stage]):
            bad.append((b, e, e32[b]))
    assert not bad, (stage, tag, bad)
    return worst


def split3(x):
    """float32 x -> (p0, p1, p2) float32 tensors holding bf16 values, p0 + p1 + p2 == x exactly (gp_split3: round to nearest
    even at every step)."""
    x = x.float()
    p0 = x.bfloat16().float()
    r = x - p0
    p1 = r.bfloat16().float()
    p2 = (r - p1).bfloat16().float()
    return p0, p1, p2


TERMS = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))      # (p, q), p + q <= 2, smallest first


def matmul_split3(A, B):
    """A @ B in float32 from the six cross terms of the three-piece splits, added smallest first."""
    a, b = split3(A), split3(B)
    C = None
    for p, q in TERMS:
        t = a[p] @ b[q]
        C = t if C is None else C + t
    return C


def bgemm_split3(A, B, alpha=1.0, beta=0.0, D=None, diag=0.0):
    """transmil_ref.bgemm on the emulated product, float32 throughout."""
    C = alpha * matmul_split3(A, B)
    if beta != 0.0:
        C = C + beta * D.float()
    if diag != 0.0:
        C = C + diag * torch.eye(A.shape[-2], B.shape[-1], dtype=torch.float32)
    return C


def pinv_split3(a2):
    """transmil_ref.pinv in float32 with every product of the six iterations on the emulation, in the order ops._tm_pinv_fwd
    issues them: X = A2 Z, T2 = X X - 7 X + 15 I, T3 = 13 I - X T2, Z = Z T3 / 4."""
    a = a2.float()
    z = R.z0(a)["Z0"]
    for _ in range(R.ITERS):
        x = bgemm_split3(a, z)
        t2 = bgemm_split3(x, x, 1.0, -7.0, x, 15.0)
        t3 = bgemm_split3(x, t2, -1.0, 0.0, None, 13.0)
        z = bgemm_split3(z, t3, 0.25)
    return z


def pinv_grad(a2, dZ, dtype=torch.float64):
    """(Z, dA2) of transmil_ref.pinv by autograd, dZ the gradient of the last iterate."""
    a = a2.detach().to(dtype).clone().requires_grad_(True)
    z = R.pinv(a)
    z.backward(dZ.to(dtype))
    return z.detach(), a.grad


def head_blocks():
    return {f"head{h}": (h,) for h in range(R.H)}
