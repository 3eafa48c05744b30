"""Float64 torch restatement of TransMIL (model/dim1/TransMIL.py of the reference) with the Nystrom attention of the
nystrom_attention package its TransLayer builds (8 heads x 64, 256 landmarks, 6 pseudo-inverse iterations, 33-tap residual
conv on v, zero pad at the front).  Test-side helper shared by the CPU and GPU tests; parameters are a state_dict-style
dict (synthetic.transmil_params), one bag at a time."""
import math

import torch
import torch.nn.functional as F

H, DH, M, ITERS, CONV = 8, 64, 256, 6, 33


def geometry(N):
    s = int(math.ceil(math.sqrt(N)))
    seq = s * s + 1
    n_pad = M * -(-seq // M)
    return dict(N=N, s=s, add=s * s - N, seq=seq, n_pad=n_pad, l=n_pad // M, pad=n_pad - seq)


def pinv(x, iters=ITERS):
    """Moore-Penrose iteration of nystrom_attention; the scale's max over all of x (one bag: its 8 heads)."""
    abs_x = x.abs()
    col = abs_x.sum(dim=-1)
    row = abs_x.sum(dim=-2)
    z = x.transpose(-1, -2) / (torch.max(col) * torch.max(row))
    I = torch.eye(x.shape[-1], dtype=x.dtype, device=x.device)
    for _ in range(iters):
        xz = x @ z
        z = 0.25 * z @ (13 * I - (xz @ (15 * I - (xz @ (7 * I - xz)))))
    return z


def nystrom(x, Wqkv, Wo, bo, Wconv, keep=None, return_attn=False):
    """x [n, 512] (one bag) -> to_out(Nystrom(x))[last n rows]; keep: to_out's Dropout(0.1) mask [n, 512] (None = eval)."""
    n = x.shape[0]
    m = M
    pad = (m - n % m) % m
    xp = F.pad(x, (0, 0, pad, 0))
    out, attn = core(xp @ Wqkv.t(), Wconv, return_attn)
    out = out @ Wo.t() + bo
    out = out[-n:]
    if keep is not None:
        out = out * keep / 0.9
    return out, attn


def core(qkv, Wconv, return_attn=False):
    """qkv [n_pad, 1536] (front-zero-padded rows through to_qkv) -> (merged-head output [n_pad, 512], attn or None)."""
    n_pad = qkv.shape[0]
    q, k, v = qkv.chunk(3, dim=-1)
    q, k, v = (t.reshape(-1, H, DH).transpose(0, 1) for t in (q, k, v))
    q = q * DH ** -0.5
    l = n_pad // M
    qL = q.reshape(H, M, l, DH).sum(2) / l
    kL = k.reshape(H, M, l, DH).sum(2) / l
    a1 = (q @ kL.transpose(-1, -2)).softmax(-1)
    a2 = (qL @ kL.transpose(-1, -2)).softmax(-1)
    a3 = (qL @ k.transpose(-1, -2)).softmax(-1)
    z = pinv(a2)
    out = (a1 @ z) @ (a3 @ v)
    out = out + F.conv2d(v.unsqueeze(0), Wconv, padding=(CONV // 2, 0), groups=H)[0]
    out = out.transpose(0, 1).reshape(n_pad, H * DH)
    attn = (a1 @ z @ a3) if return_attn else None
    return out, attn


def ppeg(x, s, p, prefix="pos_layer."):
    C = x.shape[1]
    cls, feat = x[:1], x[1:]
    f = feat.t().reshape(1, C, s, s)
    y = f
    for name, kk in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        y = y + F.conv2d(f, p[prefix + name + ".weight"], p[prefix + name + ".bias"], padding=kk // 2, groups=C)
    return torch.cat([cls, y.reshape(C, s * s).t()], 0)


def transmil(xb, p, keeps=None, return_attn=False):
    """One bag xb [N, L] -> (h [512], [attn0, attn1]); keeps: (mask layer1, mask layer2) or None."""
    N = xb.shape[0]
    g = geometry(N)
    h = F.relu(xb @ p["_fc1.0.weight"].t() + p["_fc1.0.bias"])
    h = torch.cat([p["cls_token"].reshape(1, -1), h, h[:g["add"]]], 0)
    attns = []
    for i, layer in enumerate(("layer1", "layer2")):
        if i == 1:
            h = ppeg(h, g["s"], p)
        ln = F.layer_norm(h, (h.shape[1],), p[f"{layer}.norm.weight"], p[f"{layer}.norm.bias"], 1e-5)
        o, a = nystrom(ln, p[f"{layer}.attn.to_qkv.weight"], p[f"{layer}.attn.to_out.0.weight"],
                       p[f"{layer}.attn.to_out.0.bias"], p[f"{layer}.attn.res_conv.weight"],
                       None if keeps is None else keeps[i], return_attn)
        h = h + o
        attns.append(a)
    out = F.layer_norm(h[:1], (h.shape[1],), p["norm.weight"], p["norm.bias"], 1e-5)[0]
    return out, attns


def unpack_bits(bits, cols):
    """[rows, cols / 32] int32 keep words -> float64 0/1 mask [rows, cols] (bit c & 31 of word c >> 5)."""
    b = bits.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, dtype=torch.int64)
    return ((b.unsqueeze(-1) >> sh) & 1).reshape(bits.shape[0], cols).to(torch.float64)
