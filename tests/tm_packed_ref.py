"""Test-side helpers of the packed sequence (mil_tm_*_packed, ops.nystrom_core_packed, TransMIL.packed) that tests/transmil_ref.py
and tests/tm_fixed_ref.py do not hold: the entries' names, the shared stage case, and the three planted mistakes in float64."""
import functools

import torch

import transmil_ref as R

NAMES = ("mil_tm_landmarks_packed", "mil_tm_landmarks_bwd_packed", "mil_tm_lmk_attn_packed_ws_floats", "mil_tm_lmk_attn_fwd_packed",
         "mil_tm_lmk_attn_bwd_packed", "mil_tm_tok_attn_packed_ws_floats", "mil_tm_tok_attn_fwd_packed", "mil_tm_tok_attn_bwd_packed",
         "mil_tm_resconv_packed_ws_floats", "mil_tm_resconv_packed", "mil_tm_resconv_bwd_packed", "mil_tm_resconv_bwd_packed_fixed")
SIZES = tuple(n for n in NAMES if n.endswith("_ws_floats"))
STATUS = tuple(n for n in NAMES if n not in SIZES)
# the single-bag token-side entries a packed step must not launch
SINGLE = ("mil_tm_landmarks", "mil_tm_landmarks_bwd", "mil_tm_lmk_attn_fwd", "mil_tm_lmk_attn_bwd", "mil_tm_tok_attn_fwd",
          "mil_tm_tok_attn_bwd", "mil_tm_resconv", "mil_tm_resconv_bwd", "mil_tm_resconv_bwd_fixed")

# a first bag, a one-block bag between larger ones, bags of 1, 2 and 3 forward chunks (2, 4 and 6 backward chunks); and one bag alone
BLOCKS = ((1, 2, 1, 3), (2,))
SMALL = R.H * R.M * R.DH                               # elements of one bag's [8, 256, 64] operand


def offsets(blocks):
    off = [0]
    for k in blocks:
        off.append(off[-1] + k)
    return off


def table(blocks):
    """blk_off [nb + 1], then bag_of_blk [total_blocks] - restated, not imported from the code under test."""
    return offsets(blocks) + [b for b, k in enumerate(blocks) for _ in range(k)]


@functools.lru_cache(maxsize=None)
def stage_case(blocks):
    """float32 CPU inputs of the per-kernel tests, random in ALL rows (the pad rows included, so a leak across a bag boundary
    shows): packed qkv [R, 1536], dO [R, 512], dqkv0 [R, 1536] (what the += entries find), the stacked small operands
    [nb, 8, 256, 64] (qL scaled as the landmarks leave it, kL, U, dW, dqL, dkL), and the conv weight."""
    nb, rows = len(blocks), 256 * sum(blocks)
    g = torch.Generator().manual_seed(4000 + 17 * rows + nb)
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float32)        # noqa: E731
    c = dict(qkv=rn(rows, 1536), dO=rn(rows, 512), dqkv0=rn(rows, 1536), out0=rn(rows, 512))
    for k in ("qL", "kL", "U", "dW", "dqL", "dkL"):
        c[k] = rn(nb, R.H, R.M, R.DH)
    c["qL"] = c["qL"] * R.DH ** -0.5
    c["w"] = (torch.rand((R.H, R.CONV), generator=g, dtype=torch.float32) * 2 - 1) / R.CONV ** 0.5
    return c


def bag_rows(blocks, b):
    off = offsets(blocks)
    return slice(256 * off[b], 256 * off[b + 1])


# ---- the three mistakes a packed kernel can make silently, in float64 on the stage case
def conv_ref(c, blocks, dtype=torch.float64, leak=False):
    """The conv's addend [R, 512]: per bag, clipped at the bag's own rows; leak: one window over all packed rows."""
    qkv, w = c["qkv"].to(dtype), c["w"].to(dtype)
    if leak:
        return R.resconv(qkv, w)
    return torch.cat([R.resconv(qkv[bag_rows(blocks, b)], w) for b in range(len(blocks))], 0)


def landmarks_ref(c, blocks, dtype=torch.float64, neighbour=False):
    """(qL, kL) stacked [nb, 8, 256, 64] with every bag's own l; neighbour: bag b's means taken with the l of the next bag
    (the last one: of the one before), from its first row on, clamped into the packed rows."""
    qkv = c["qkv"].to(dtype)
    out = []
    for b, l in enumerate(blocks):
        lw = blocks[(b + 1) % len(blocks)] if b + 1 < len(blocks) else blocks[b - 1]
        l = lw if neighbour else l
        r0 = bag_rows(blocks, b).start
        rows = qkv[r0:r0 + 256 * l]
        if rows.shape[0] < 256 * l:                       # the wrong l reaches past the end: the kernel would too; wrap for the test
            rows = torch.cat([rows, qkv[:256 * l - rows.shape[0]]], 0)
        out.append(R.landmarks(rows, l))
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def lmk_w_ref(c, blocks, dtype=torch.float64, all_chunks=False):
    """W [nb, 8, 256, 64] = softmax(qL k^T) v over the bag's keys; all_chunks: over every packed key (a merge that does not stop
    at the bag)."""
    qkv, qL = c["qkv"].to(dtype), c["qL"].to(dtype)
    out = []
    for b in range(len(blocks)):
        rows = qkv if all_chunks else qkv[bag_rows(blocks, b)]
        k = rows[:, 512:1024].reshape(-1, R.H, R.DH).transpose(0, 1)
        v = rows[:, 1024:].reshape(-1, R.H, R.DH).transpose(0, 1)
        out.append((qL[b] @ k.transpose(-1, -2)).softmax(-1) @ v)
    return torch.stack(out)
