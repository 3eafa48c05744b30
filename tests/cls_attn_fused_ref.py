"""The cls token's per-patch attention from the operands of the two fused passes (csrc/cls_attn_fused.hip:
mil_tm_cls_attn_fused), restated for any float dtype.  With P = A1 Z A3 the map of one Nystrom layer and the cls token at padded
row `pad`:
    a1[h, m]  = softmax_m(64^-0.5 q[pad, h, :] . kL[h, m, :])
    t[h, :]   = a1[h, :] Z[h]
    r[h, j]   = sum_m t[h, m] exp(qL[h, m, :] . k[j, h, :] - lse3[h, m])            j over the n_pad keys
    out[h, i] = r[h, pad + 1 + i] + (i < s^2 - N ? r[h, pad + 1 + N + i] : 0)       i < N
Nothing of size 256 x n_pad per head is an operand.  Shared by tests/test_cls_attn_fused_host.py, which holds it against
test_transmil_cls_attn_host.cls_attn_ref on the maps, and tests/test_gpu_cls_attn_fused.py.  Nothing here touches the GPU or the
package."""
import functools

import torch

import transmil_ref as R
from test_transmil_cls_attn_host import KERNEL_SHAPES, cls_blocks

MUTATIONS = ("nofold", "row", "shift", "zT", "qscale", "lse_nopad", "lse_head")
PEAKS = (1.0, R.PEAK)
CASES = [(n_pad, N, peak) for peak in PEAKS for n_pad, N in KERNEL_SHAPES]


def heads(cols):
    """[n, 512] merged-head columns -> [8, n, 64]."""
    return cols.reshape(cols.shape[0], R.H, R.DH).transpose(0, 1)


def operands(qkv):
    """What the fused core holds when the cls attention is formed, by the formulas of R.core: qL (scaled) and kL [8, 256, 64],
    Z [8, 256, 256] the pseudo-inverse iterate, lse3 [8, 256] = logsumexp(qL k^T) over ALL n_pad keys."""
    qL, kL = R.landmarks(qkv, qkv.shape[0] // R.M)
    k = heads(qkv[:, R.H * R.DH:2 * R.H * R.DH])
    Z = R.pinv((qL @ kL.transpose(-1, -2)).softmax(-1))
    return dict(qL=qL, kL=kL, Z=Z, lse3=(qL @ k.transpose(-1, -2)).logsumexp(-1))


def cls_fused_ref(qkv, qL, kL, Z, lse3, pad, N, s, mutate=None):
    """-> [8, N] in the operands' dtype.  mutate: a planted error - "nofold": the repeats' keys dropped; "row": row pad - 1
    instead of the cls row; "shift": columns one to the left, so the cls column leaks in; "zT": Z transposed; "qscale": the
    cls query not scaled; "lse_nopad": the normaliser over the sequence keys only, the zero front-pad keys dropped;
    "lse_head": lse3 of the neighbouring head."""
    assert mutate is None or mutate in MUTATIONS, mutate
    n_pad, add = qkv.shape[0], s * s - N
    assert pad + 1 + s * s == n_pad and 0 <= add < 2 * s
    row = pad - 1 if mutate == "row" else pad
    q = qkv[row, :R.H * R.DH].reshape(R.H, R.DH) * (1.0 if mutate == "qscale" else R.DH ** -0.5)
    a1 = torch.einsum("hd,hmd->hm", q, kL).softmax(-1)
    t = torch.einsum("hk,hkj->hj", a1, Z.transpose(-1, -2) if mutate == "zT" else Z)
    s3 = qL @ heads(qkv[:, R.H * R.DH:2 * R.H * R.DH]).transpose(-1, -2)              # [8, 256, n_pad]
    lse = lse3.reshape(R.H, R.M)
    if mutate == "lse_nopad":
        lse = s3[..., pad:].logsumexp(-1)
    elif mutate == "lse_head":
        lse = lse.roll(1, 0)
    r = torch.einsum("hm,hmj->hj", t, (s3 - lse.unsqueeze(-1)).exp())
    c0 = pad if mutate == "shift" else pad + 1
    out = r[:, c0:c0 + N].clone()
    if mutate != "nofold":
        out[:, :add] += r[:, c0 + N:c0 + N + add]
    return out


def fused_qkv(n_pad, N, peak):
    """qkv [n_pad, 1536] float32-exact, held in float64: randn with the front pad rows zero and the q | k columns x peak."""
    g = R.geometry(N)
    assert g["n_pad"] == n_pad
    qkv = torch.randn((n_pad, 1536), generator=torch.Generator().manual_seed(13 * n_pad + N + int(100 * peak)))
    qkv[:g["pad"]] = 0
    qkv[:, :2 * R.H * R.DH] *= peak
    return qkv.double()


@functools.lru_cache(maxsize=None)
def fused_case(n_pad, N, peak):
    """(qkv, the operands in float64, the float64 reference [8, N], the restatement in float32 on those operands cast to
    float32 - what the kernel is given -, the geometry): computed once per case and left unchanged."""
    g = R.geometry(N)
    qkv = fused_qkv(n_pad, N, peak)
    with torch.no_grad():
        ops64 = operands(qkv)
        ref = cls_fused_ref(qkv, **ops64, pad=g["pad"], N=N, s=g["s"])
        r32 = cls_fused_ref(qkv.float(), **{k: v.float() for k, v in ops64.items()}, pad=g["pad"], N=N, s=g["s"])
    return qkv, ops64, ref, r32, g


__all__ = ["MUTATIONS", "PEAKS", "CASES", "KERNEL_SHAPES", "cls_blocks", "heads", "operands", "cls_fused_ref", "fused_qkv",
           "fused_case"]
