"""The per-patch cls attention of a packed step's bags (csrc/cls_attn_fused.hip: mil_tm_cls_attn_packed, ops.tm_cls_attention_packed)
restated for any float dtype: per bag cls_attn_fused_ref.cls_fused_ref on that bag's rows of the packed qkv and its slices of the
operands stacked [nb, 8, 256, .], each bag's [8, s_b^2] - zeros from N_b on - at float 8 off_b of one flat buffer.  The geometry
table's host values are restated here too, and the mistakes a packed kernel can make silently are planted in a second
restatement that addresses the packed rows the way the kernel does (packed_out), which test_tm_cls_packed_host.py first holds
against the per-bag one.  Shared by tests/test_tm_cls_packed_host.py and tests/test_gpu_tm_cls_packed.py; nothing here touches
the GPU or the package."""
import functools

import torch

import transmil_ref as R
from cls_attn_fused_ref import PEAKS, cls_blocks, cls_fused_ref, fused_case, heads

NAMES = ("mil_tm_cls_attn_packed_ws_floats", "mil_tm_cls_attn_packed")
# 250 and 256: pad 255, the whole first block lies in front of the cls column; 7: a one-block bag in the middle; 1500: pad 14,
# tile 0 straddles the cls column; 256: add 0, nothing folds
LENGTHS = (250, 7, 1500, 256)
SIDES = (16, 3, 39, 16)
BLOCKS = (2, 1, 6, 2)
ROWS = 256 * sum(BLOCKS)
MUTATIONS = ("t0", "pad0", "nooff", "len_next")


def offsets(counts):
    off = [0]
    for k in counts:
        off.append(off[-1] + k)
    return off


def cls_table(sides):
    """side [nb] | off [nb + 1], off[b] = the patches of the bags in front of bag b - restated, not imported from the code under test."""
    return list(sides) + offsets([s * s for s in sides])


def ws_floats(total_blocks, nb):
    """The workspace formula of include/mil_hip.h, restated: t [nb, 8, 256] | r [8, 256 total_blocks]."""
    return nb * R.H * R.M + R.H * 256 * total_blocks


def clamp(n, s):
    """A device length as the fold reads it: into the side's bucket ((s - 1)^2, s^2]."""
    return min(max(int(n), (s - 1) * (s - 1) + 1), s * s)


@functools.lru_cache(maxsize=None)
def packed_case(peak, lengths=LENGTHS):
    """The bags' fused_case inputs as the packed route holds them, float32-exact in float64: qkv [256 sum blocks, 1536] the bags'
    rows one after another, qL, kL [nb, 8, 256, 64], Z [nb, 8, 256, 256], lse3 [nb, 8, 256] stacked; plus the geometries.  Computed
    once per peak and left unchanged."""
    geo = [R.geometry(n) for n in lengths]
    cases = [fused_case(g["n_pad"], n, peak) for g, n in zip(geo, lengths)]
    ops64 = {k: torch.stack([c[1][k] for c in cases]) for k in ("qL", "kL", "Z", "lse3")}
    return dict(qkv=torch.cat([c[0] for c in cases], 0), geo=geo, lengths=tuple(lengths), **ops64)


def _cast(c, dtype):
    return {k: c[k].to(dtype) for k in ("qkv", "qL", "kL", "Z", "lse3")}


def per_bag_ref(c, dtype=torch.float64, lengths=None):
    """[one [8, s_b^2] per bag, zeros from N_b on]: cls_fused_ref on bag b's rows and slices.  lengths: other lengths of the same
    sides (default: the case's own)."""
    t = _cast(c, dtype)
    outs, row = [], 0
    for b, g in enumerate(c["geo"]):
        N = g["N"] if lengths is None else int(lengths[b])
        a = cls_fused_ref(t["qkv"][row:row + g["n_pad"]], t["qL"][b], t["kL"][b], t["Z"][b], t["lse3"][b], pad=g["pad"], N=N, s=g["s"])
        outs.append(torch.cat([a, a.new_zeros((R.H, g["s"] ** 2 - N))], 1))
        row += g["n_pad"]
    return outs


def packed_flat(outs):
    """The per-bag [8, s_b^2] in the layout of the entry's output: bag b's contiguous block at float 8 off_b."""
    return torch.cat([a.reshape(-1) for a in outs])


def packed_out(c, dtype=torch.float64, mutate=None):
    """The flat output [8 sum s_b^2] formed the way the kernels address the packed rows: bag b's cls query at packed row
    256 c0_b + pad_b, its keys the s_b^2 packed rows behind that, its length clamped into the bucket, its block written at float
    8 off_b.  mutate: a planted error - "t0": every bag uses bag 0's t (its cls row, kL and Z); "pad0": bag 0's pad for all bags;
    "nooff": every bag written at offset 0, in bag order; "len_next": the fold with the next bag's length (the last: the first's)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    t = _cast(c, dtype)
    geo, nb = c["geo"], len(c["geo"])
    c0 = offsets([g["l"] for g in geo])
    off = offsets([g["s"] ** 2 for g in geo])
    out = torch.zeros(R.H * off[-1], dtype=dtype)
    k_all = heads(t["qkv"][:, R.H * R.DH:2 * R.H * R.DH])                        # [8, rows, 64]
    for b, g in enumerate(geo):
        s, S2 = g["s"], g["s"] ** 2
        tb = 0 if mutate == "t0" else b
        pad = geo[0]["pad"] if mutate == "pad0" else g["pad"]
        N = clamp(c["lengths"][(b + 1) % nb], s) if mutate == "len_next" else g["N"]
        q = t["qkv"][256 * c0[tb] + (geo[0]["pad"] if mutate == "t0" else pad), :R.H * R.DH].reshape(R.H, R.DH) * R.DH ** -0.5
        tt = torch.einsum("hk,hkj->hj", torch.einsum("hd,hmd->hm", q, t["kL"][tb]).softmax(-1), t["Z"][tb])
        first = 256 * c0[b] + pad + 1
        keys = k_all[:, [j % t["qkv"].shape[0] for j in range(first, first + S2)]]      # a wrong pad runs into the next bag's rows
        r = torch.einsum("hm,hmj->hj", tt, (t["qL"][b] @ keys.transpose(-1, -2) - t["lse3"][b].reshape(R.H, R.M, 1)).exp())
        a = torch.zeros((R.H, S2), dtype=dtype)
        a[:, :N] = r[:, :N]
        a[:, :S2 - N] += r[:, N:]
        at = 0 if mutate == "nooff" else R.H * off[b]
        out[at:at + R.H * S2] = a.reshape(-1)
    return out


def bag_views(flat, sides=SIDES):
    off = offsets([s * s for s in sides])
    return [flat[R.H * o:R.H * (o + s * s)].reshape(R.H, s * s) for o, s in zip(off, sides)]


__all__ = ["NAMES", "LENGTHS", "SIDES", "BLOCKS", "ROWS", "MUTATIONS", "PEAKS", "cls_blocks", "offsets", "cls_table", "ws_floats",
           "clamp", "packed_case", "per_bag_ref", "packed_flat", "packed_out", "bag_views"]
