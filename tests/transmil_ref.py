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


def pinv(x, iters=ITERS, mutate=None):
    """Moore-Penrose iteration of nystrom_attention; the scale's max over all of x (one bag: its 8 heads)."""
    z = z0(x, mutate)["Z0"]
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


CORE_MUTATIONS = ("pinv_detach", "z0_detach", "qL_detach", "kL_detach", "scale_detach", "scale_per_head")


def core(qkv, Wconv, return_attn=False, mutate=None):
    """qkv [n_pad, 1536] (front-zero-padded rows through to_qkv) -> (merged-head output [n_pad, 512], attn or None).
    mutate: one of CORE_MUTATIONS, a planted error (tests/test_transmil_sensitivity_host.py) - None is the operation."""
    assert mutate is None or mutate in CORE_MUTATIONS, mutate
    n_pad = qkv.shape[0]
    q, k, v = qkv.chunk(3, dim=-1)
    q, k, v = (t.reshape(-1, H, DH).transpose(0, 1) for t in (q, k, v))
    q = q * DH ** -0.5
    l = n_pad // M
    qL = q.reshape(H, M, l, DH).sum(2) / l
    kL = k.reshape(H, M, l, DH).sum(2) / l
    if mutate == "qL_detach":
        qL = qL.detach()
    if mutate == "kL_detach":
        kL = kL.detach()
    a1 = (q @ kL.transpose(-1, -2)).softmax(-1)
    a2 = (qL @ kL.transpose(-1, -2)).softmax(-1)
    a3 = (qL @ k.transpose(-1, -2)).softmax(-1)
    z = pinv(a2, mutate=mutate)
    if mutate == "pinv_detach":
        z = z.detach()
    out = (a1 @ z) @ (a3 @ v)
    # the residual conv as resconv() states it (F.conv2d(v, Wconv, padding=(16, 0), groups=8) to 1e-14 in float64: its
    # float32 weight gradient on the CPU is off by up to 5e-2, which would make the float32 yardstick of dw useless)
    out = out.transpose(0, 1).reshape(n_pad, H * DH) + resconv(qkv, Wconv)
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


# --------------------------------------------------------------------------- the single stages of csrc/transmil.hip
# Each is written for any float dtype: float64 is the reference, the same code in float32 on the CPU gives `e32`, the error
# that the number format alone costs, and the GPU bound of a block is bound(e32, k).  mutate= plants one error per stage:
# the sensitivity test (tests/test_transmil_sensitivity_host.py) asserts that each of them breaks such a bound by 10 x.
FLOOR, K_CAP = 1e-7, 16
PEAK = 3.0          # scale of q and k in the peaked whole-core case (test_transmil_sensitivity_host.py shows it is well posed)


def bound(e32, k):
    return k * max(e32, FLOOR)


def block_err(got, ref, blocks):
    """{name: max|got - ref| / max|ref| over that block} (step_ref.max_err per block).  blocks: {name: index}, an index
    being whatever ref[...] accepts; empty blocks are left out.  A block whose reference is all zero must be met exactly."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = {}
    for name, ix in blocks.items():
        g, r = got[ix], ref[ix]
        if r.numel() == 0:
            continue
        d, top = float((g - r).abs().max()), float(r.abs().max())
        if not math.isfinite(d):
            out[name] = math.inf
        else:
            out[name] = d / top if top > 0 else (0.0 if d == 0 else math.inf)
    return out


def whole():
    return {"all": (Ellipsis,)}


def qkv_blocks(n, pad=0):
    """[n, 1536] q|k|v rows (qkv, dqkv): the three column groups, each also over the front pad rows and the conv halo."""
    out = {}
    for i, c in enumerate("qkv"):
        cols = slice(512 * i, 512 * (i + 1))
        out[c] = (slice(None), cols)
        out[c + "_pad"] = (slice(0, pad), cols)
        out[c + "_first16"] = (slice(0, min(16, n)), cols)
        out[c + "_last16"] = (slice(max(0, n - 16), n), cols)
    return out


def row_blocks(n, pad=0):
    """[n, 512] rows (out, dout): all, the front pad rows, the first and last 16 rows (conv halo)."""
    return {"all": (slice(None),), "pad": (slice(0, pad),), "first16": (slice(0, min(16, n)),),
            "last16": (slice(max(0, n - 16), n),)}


def ppeg_blocks(s):
    """[1 + s^2, 512] rows: cls, the outer ring of width 3 of the s x s grid, the interior."""
    i = torch.arange(s)
    edge = (i < 3) | (i >= s - 3)
    ring = (edge[:, None] | edge[None, :]).reshape(-1)
    f = torch.zeros(1, dtype=torch.bool)
    return {"cls": torch.cat([~f, torch.zeros(s * s, dtype=torch.bool)]), "ring": torch.cat([f, ring]),
            "interior": torch.cat([f, ~ring])}


def wqkv_blocks():
    """to_qkv.weight [1536, 512] and its gradient: the q, k and v row blocks."""
    return {c: (slice(512 * i, 512 * (i + 1)),) for i, c in enumerate("qkv")}


def bgemm_blocks(Mr, Nc):
    """[batch, M, N]: all, and the last (partial) 64-tile in M and in N."""
    return {"all": (Ellipsis,), "m_tail": (slice(None), slice(64 * ((Mr - 1) // 64), Mr)),
            "n_tail": (slice(None), slice(None), slice(64 * ((Nc - 1) // 64), Nc))}


def bgemm(A, B, alpha=1.0, beta=0.0, D=None, diag=0.0, mutate=None):
    """alpha A B + beta D + diag I, A [b, M, K], B [b, K, N].  mutate "ktail": the last 16-slice of K dropped."""
    K = A.shape[-1]
    if mutate == "ktail":
        K = 16 * ((K - 1) // 16)
    C = alpha * (A[..., :K] @ B[..., :K, :])
    if beta != 0.0:
        C = C + beta * D
    if diag != 0.0:
        C = C + diag * torch.eye(A.shape[-2], B.shape[-1], dtype=A.dtype)
    return C


def landmarks(qkv, l):
    """(qL, kL) [8, 256, 64]: the means of l consecutive rows of q (times 64^-0.5) and of k."""
    def mean(cols):
        return cols[:M * l].reshape(M, l, H, DH).sum(1).transpose(0, 1) / l
    return mean(qkv[:, :H * DH]) * DH ** -0.5, mean(qkv[:, H * DH:2 * H * DH])


def landmarks_bwd(dqL, dkL, l):
    """[256 l, 1024]: what the landmark gradients add to the q and k columns of dqkv."""
    def spread(d, coef):
        return d.transpose(0, 1).reshape(M, H * DH).repeat_interleave(l, 0) * coef
    return torch.cat([spread(dqL, DH ** -0.5 / l), spread(dkL, 1.0 / l)], 1)


def softmax_rows(x):
    return x.softmax(-1)


def softmax_rows_bwd(p, dp, mutate=None):
    """p (dp - <p, dp>) per row.  mutate "nodot": the <p, dp> term dropped."""
    if mutate == "nodot":
        return p * dp
    return p * (dp - (p * dp).sum(-1, keepdim=True))


def z0(a2, mutate=None):
    """Start of the pseudo-inverse on a2 [8, 256, 256]: Z0 = a2^T / (largest row abs-sum x largest column abs-sum, both over
    all 8 heads), with the maxima per head and arg = head * 256 + column of the largest column sum (first on ties).
    mutate "scale_per_head": the maxima per head; "scale_detach": no gradient through the scale; "z0_detach": none at all."""
    a = a2.abs()
    rsum, csum = a.sum(-1), a.sum(-2)                         # [8, 256] each: per row, per column
    mr, mc = rsum.max(), csum.max()
    if mutate == "scale_per_head":
        mr, mc = rsum.amax(-1).reshape(-1, 1, 1), csum.amax(-1).reshape(-1, 1, 1)
    s = mr * mc
    if mutate == "scale_detach":
        s = s.detach()
    Z = a2.transpose(-1, -2) / s
    if mutate == "z0_detach":
        Z = Z.detach()
    flat = csum.detach().reshape(-1)
    arg = int((flat == flat.max()).nonzero()[0])
    return {"Z0": Z, "scale": torch.stack([rsum.max() * csum.max(), rsum.max(), csum.max()]).detach(),
            "row_max": rsum.amax(-1).detach(), "col_max": csum.amax(-1).detach(), "arg": arg}


def _conv_taps(w, dtype):
    return w.reshape(H, CONV).to(dtype).repeat_interleave(DH, 0)          # [512, 33]: the head's taps for each channel


def resconv(qkv, w, mutate=None):
    """[n, 512]: sum_t w[head][t] v[i + t - 16] (v = columns 1024.. of qkv, zero outside).  mutate "tap": tap 5 dropped,
    "lastrow": the last row left zero."""
    n = qkv.shape[0]
    wc = _conv_taps(w, qkv.dtype)
    vp = F.pad(qkv[:, 2 * H * DH:], (0, 0, CONV // 2, CONV // 2))
    out = torch.zeros((n, H * DH), dtype=qkv.dtype)
    for t in range(CONV):
        if not (mutate == "tap" and t == 5):
            out = out + wc[:, t] * vp[t:t + n]
    if mutate == "lastrow":
        out = torch.cat([out[:-1], torch.zeros_like(out[-1:])], 0)
    return out


def resconv_bwd(dout, qkv, w):
    """The three gradients of out += resconv(qkv, w): (of the out that came in [n, 512], of v [n, 512], of w [8, 33])."""
    n = qkv.shape[0]
    wc = _conv_taps(w, qkv.dtype)
    vp = F.pad(qkv[:, 2 * H * DH:], (0, 0, CONV // 2, CONV // 2))
    dp = F.pad(dout, (0, 0, CONV // 2, CONV // 2))
    dv = torch.zeros_like(dout)
    dw = []
    for t in range(CONV):
        dv = dv + wc[:, t] * dp[CONV - 1 - t:CONV - 1 - t + n]
        dw.append((dout * vp[t:t + n]).reshape(n, H, DH).sum((0, 2)))
    return dout, dv, torch.stack(dw, 1)


def ppeg_folded(x, s, p, prefix="pos_layer.", mutate=None):
    """ppeg() as the one depthwise 7 x 7 the kernel runs: W7 + pad(W5) + pad(W3) + delta, bias b7 + b5 + b3.  mutate
    "offcentre": the 3 x 3 weights folded one tap to the right; "clamp": the border replicated instead of zero."""
    C = x.shape[1]
    W7, W5, W3 = (p[prefix + n + ".weight"] for n in ("proj", "proj1", "proj2"))
    delta = torch.zeros((7, 7), dtype=x.dtype)
    delta[3, 3] = 1
    Wf = W7 + F.pad(W5, (1, 1, 1, 1)) + F.pad(W3, (3, 1, 2, 2) if mutate == "offcentre" else (2, 2, 2, 2)) + delta
    bias = p[prefix + "proj.bias"] + p[prefix + "proj1.bias"] + p[prefix + "proj2.bias"]
    f = x[1:].t().reshape(1, C, s, s)
    f = F.pad(f, (3, 3, 3, 3), mode="replicate") if mutate == "clamp" else F.pad(f, (3, 3, 3, 3))
    y = F.conv2d(f, Wf, bias, groups=C)
    return torch.cat([x[:1], y.reshape(C, s * s).t()], 0)


def seq_index(lengths, sides):
    """Index of the sequence assembly of bags packed back to back: per bag [-2 | its rows | its first s^2 - N rows again],
    a length clamped into its side's bucket ((s - 1)^2, s^2] -> (idx, rows, flag) as mil_tm_seq_index leaves them."""
    idx, off, flag = [], 0, 0
    for n, s in zip(lengths, sides):
        c = min(max(n, (s - 1) * (s - 1) + 1), s * s)
        flag |= int(c != n)
        idx += [-2] + list(range(off, off + c)) + list(range(off, off + s * s - c))
        off += c
    return idx, off, flag


# --------------------------------------------------------------------------- shared cases of the stage tests
def flat_err(got, ref, blocks):
    """{tensor.block: error} over a dict of tensors; blocks: {tensor name: {block name: index}}."""
    return {f"{t}.{b}": e for t in blocks for b, e in block_err(got[t], ref[t], blocks[t]).items()}


def core_case(n_pad, peak=1.0):
    """Inputs of the whole-core test (float64): randn qkv with the front pad rows zero, res_conv weight, randn dO.
    peak > 1 scales q and k, which sharpens the rows of the three softmax maps."""
    g = torch.Generator().manual_seed(n_pad)
    pad = 37 if n_pad > 256 else 3
    qkv = torch.randn((n_pad, 1536), generator=g, dtype=torch.float64)
    qkv[:pad] = 0
    qkv[:, :1024] *= peak
    w = (torch.rand((H, 1, CONV, 1), generator=g, dtype=torch.float64) * 2 - 1) / CONV ** 0.5
    dO = torch.randn((n_pad, 512), generator=g, dtype=torch.float64)
    dO[:pad] = 0
    return qkv, w, dO, pad


def core_run(qkv, w, dO, dtype=torch.float64, mutate=None):
    q, wr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (qkv, w))
    out, _ = core(q, wr, mutate=mutate)
    out.backward(dO.to(dtype))
    return {"out": out.detach(), "dqkv": q.grad, "dw": wr.grad.reshape(H, CONV)}


def core_blocks(n_pad, pad):
    return {"out": row_blocks(n_pad, pad), "dqkv": qkv_blocks(n_pad, pad), "dw": whole()}


def pinv_case(seed=5, col_head=3, col=77, row_head=None, row=11):
    """A2 [8, 256, 256] float32-exact (held in float64): row-softmaxed randn logits, one column of head col_head raised so
    that the largest column sum lies there; row_head: one of its rows scaled by 1 + 2^-10, so that the largest row sum lies
    there (forward checks only: such a row is no softmax output).  dZ0 randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((H, M, M), generator=g, dtype=torch.float64)
    x[col_head, :, col] += 3.0
    a2 = x.float().softmax(-1)
    if row_head is not None:
        a2[row_head, row] *= 1 + 2.0 ** -10
    dZ = torch.randn((H, M, M), generator=g, dtype=torch.float64).float().double()
    return a2.double(), dZ


def pinv_run(a2, dZ, dtype=torch.float64, mutate=None):
    """Z0 and, through autograd of a2^T / (max x max), dS2 = softmax_rows_bwd(a2, dA2): the row-sum factor's gradient is a
    constant along a row, which the softmax backward removes."""
    a = a2.detach().to(dtype).clone().requires_grad_(True)
    r = z0(a, mutate)
    if r["Z0"].requires_grad:
        r["Z0"].backward(dZ.to(dtype))
    dA2 = a.grad if a.grad is not None else torch.zeros_like(a)
    return {"Z0": r["Z0"].detach(), "dS2": softmax_rows_bwd(a.detach(), dA2), "scale": r["scale"], "row_max": r["row_max"],
            "col_max": r["col_max"], "arg": r["arg"]}


def resconv_case(n, seed=0):
    g = torch.Generator().manual_seed(1000 + n + seed)
    qkv = torch.randn((n, 1536), generator=g, dtype=torch.float64)
    w = (torch.rand((H, CONV), generator=g, dtype=torch.float64) * 2 - 1) / CONV ** 0.5
    out0 = torch.randn((n, 512), generator=g, dtype=torch.float64)       # what the buffers hold before: the stages add
    dout = torch.randn((n, 512), generator=g, dtype=torch.float64)
    dqkv0 = torch.randn((n, 1536), generator=g, dtype=torch.float64)
    dw0 = torch.randn((H, CONV), generator=g, dtype=torch.float64)
    return dict(qkv=qkv, w=w, out0=out0, dout=dout, dqkv0=dqkv0, dw0=dw0)


def resconv_run(c, dtype=torch.float64, mutate=None):
    c = {k: v.to(dtype) for k, v in c.items()}
    _, dv, dw = resconv_bwd(c["dout"], c["qkv"], c["w"])
    return {"out": c["out0"] + resconv(c["qkv"], c["w"], mutate), "dv": c["dqkv0"][:, 1024:] + dv, "dw": c["dw0"] + dw}


def resconv_blocks(n):
    return {"out": row_blocks(n), "dv": row_blocks(n), "dw": whole()}


PPEG_NAMES = ("proj.weight", "proj.bias", "proj1.weight", "proj1.bias", "proj2.weight", "proj2.bias")


def ppeg_case(s, seed=0):
    g = torch.Generator().manual_seed(2000 + s + seed)
    p = {}
    for name, kk in (("proj", 7), ("proj1", 5), ("proj2", 3)):
        p[f"pos_layer.{name}.weight"] = (torch.rand((512, 1, kk, kk), generator=g, dtype=torch.float64) * 2 - 1) / kk
        p[f"pos_layer.{name}.bias"] = (torch.rand(512, generator=g, dtype=torch.float64) * 2 - 1) / kk
    x = torch.randn((1 + s * s, 512), generator=g, dtype=torch.float64)
    dy = torch.randn((1 + s * s, 512), generator=g, dtype=torch.float64)
    return p, x, dy


def ppeg_run(p, x, dy, s, dtype=torch.float64, mutate=None):
    pr = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    y = ppeg_folded(xr, s, pr, mutate=mutate)
    y.backward(dy.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad}
    out.update({"d" + n: pr["pos_layer." + n].grad for n in PPEG_NAMES})
    return out


def ppeg_all_blocks(s):
    out = {"y": ppeg_blocks(s), "dx": ppeg_blocks(s)}
    out.update({"d" + n: whole() for n in PPEG_NAMES})
    return out


def softmax_case(rows, cols, seed=0):
    """Logits with rows of every kind: randn, magnitude +-80, a constant row, some -inf entries (never a whole row)."""
    g = torch.Generator().manual_seed(3000 + 7 * rows + cols + seed)
    x = torch.randn((rows, cols), generator=g, dtype=torch.float64)
    x[0::4] *= 80.0 / 3.0
    x[1 % rows] = 0.375
    ninf = torch.rand((rows, cols), generator=g) < 0.2
    ninf[:, 0] = False
    ninf[1::2] = False
    x[ninf] = -math.inf
    dp = torch.randn((rows, cols), generator=g, dtype=torch.float64)
    return x.float().double(), dp.float().double()


def bgemm_case(batch, Mr, Nc, K, seed=0):
    g = torch.Generator().manual_seed(4000 + 131 * Mr + 17 * Nc + K + seed)
    A = torch.randn((batch, Mr, K), generator=g, dtype=torch.float64).float().double()
    B = torch.randn((batch, K, Nc), generator=g, dtype=torch.float64).float().double()
    D = torch.randn((batch, Mr, Nc), generator=g, dtype=torch.float64).float().double()
    return A, B, D


# k of bound(e32, k) per stage: the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) that the first
# full run on an MI355X showed (docs/lab_notes.md has the tables), capped at K_CAP
K_STAGE = {"bgemm": 8, "softmax": 4, "landmarks": 8, "pinv_init": 16, "resconv": 4, "ppeg": 8, "core": 8, "module": 8}


def hold(stage, tag, got, ref, r32, blocks):
    """Every block of every tensor of `got` within bound(e32, K_STAGE[stage]) of `ref`; prints each ratio first."""
    e32, eg = flat_err(r32, ref, blocks), flat_err(got, ref, blocks)
    bad = []
    for b, e in eg.items():
        print(f"RATIO | {stage} | {tag} | {b} | gpu {e:.2e} | e32 {e32[b]:.2e} | {e / max(e32[b], FLOOR):.2f}")
        if not e <= bound(e32[b], K_STAGE[stage]):
            bad.append((b, e, e32[b]))
    assert not bad, (stage, tag, bad)
