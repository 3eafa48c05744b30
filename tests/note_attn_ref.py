"""Restatements, for any float dtype, of the two entries behind `model.note_attn` (csrc/absorbed_attn.hip:
mil_absorbed_pool_attn; csrc/attn_pool.hip: mil_bag_softmax) and of the token->image attention weights of
model/sam/transformer.py at its three sites.  float64 is the reference, the same code in float32 on the CPU gives `e32`;
mutate= plants one error (tests/test_note_attn_host.py shows that the per-block bound sees each of them).  Test-side helper:
nothing here reads the code under test."""
import math

import torch
import torch.nn.functional as F

from attn_ref import E, H, TILE, absorbed_case, absorbed_pool, offsets, _pe_rows  # noqa: F401  (re-exported)
from transmil_ref import FLOOR, K_CAP, block_err, bound

K_NOTE = K_CAP                       # 16: the project's cap; the measured ratios are in docs/lab_notes.md
MUTATIONS = ("nope", "scale_eh", "lse_head", "lasttile", "prev_keys")
PEAK = 30.0


def absorbed_attention(keys, pe, Qp, lse, k_off, C, mutate=None, prev_keys=None):
    """attn [N, H]: attn[n][h] = exp(Qp[b][h] . (keys_n + pe_n) / sqrt(C) - lse[b][h]) - attn_ref.absorbed_pool without the
    value sum, the normaliser taken from `lse`.  mutate: "nope" the PE left out of the score, "scale_eh" 1 / sqrt(E / H) for
    1 / sqrt(C), "lse_head" the lse of heads 0 and 1 swapped, "lasttile" the last key of every partial 64-key tile dropped
    (weight 0), "prev_keys" the scores from `prev_keys` instead of the site's own keys."""
    assert mutate is None or mutate in MUTATIONS, mutate
    src = prev_keys.to(keys.dtype) if mutate == "prev_keys" else keys
    kin = src if mutate == "nope" else src + _pe_rows(pe, k_off).to(keys.dtype)
    sc = 1.0 / math.sqrt(E / H if mutate == "scale_eh" else C)
    if mutate == "lse_head":
        lse = lse[:, [1, 0] + list(range(2, H))]
    out = torch.zeros((keys.shape[0], H), dtype=keys.dtype)
    for b in range(len(k_off) - 1):
        rows = slice(k_off[b], k_off[b + 1])
        out[rows] = (kin[rows] @ Qp[b].t() * sc - lse[b][None, :]).exp()
        n = k_off[b + 1] - k_off[b]
        if mutate == "lasttile" and n % TILE:
            out[k_off[b + 1] - 1] = 0
    return out


def head_sums(attn, k_off):
    """[B, H]: the sum of every head's weights over the bag."""
    return torch.stack([attn[k_off[b]:k_off[b + 1]].sum(0) for b in range(len(k_off) - 1)])


def peak(c, size=PEAK):
    """One key per bag (key 13 mod n) moved along the bag's query vectors so that its score lies about `size` above the
    rest on every head: most of the other weights underflow towards 0.  Returns the case with new keys (float32-exact)."""
    C, off = c["C"], c["k_off"]
    Qp = torch.einsum("bhc,hce->bhe", c["qp"].reshape(-1, H, C), c["Wk"].reshape(H, C, -1))
    keys = c["keys"].clone()
    for b in range(len(off) - 1):
        u = (Qp[b] * (size * math.sqrt(C) / (Qp[b] * Qp[b]).sum(-1, keepdim=True))).sum(0)
        keys[off[b] + 13 % (off[b + 1] - off[b])] += u
    out = dict(c)
    out["keys"] = keys.float().double()
    return out


def fed(c):
    """(Qp, lse) of the float64 forward, rounded to float32 and held in float64: what the kernel and both restatements take."""
    C = c["C"]
    Qp = torch.einsum("bhc,hce->bhe", c["qp"].reshape(-1, H, C), c["Wk"].reshape(H, C, -1)).float().double()
    _, lse = absorbed_pool(c["keys"], c["pe"], Qp, c["k_off"], C)
    return Qp, lse.float().double()


def attn_blocks(k_off):
    """[N, H]: every (bag, 64-key tile, head)."""
    out = {}
    for b in range(len(k_off) - 1):
        for t, r0 in enumerate(range(k_off[b], k_off[b + 1], TILE)):
            for h in range(H):
                out[f"bag{b}.t{t}.h{h}"] = (slice(r0, min(r0 + TILE, k_off[b + 1])), h)
    return out


def sum_blocks(B):
    return {f"bag{b}.h{h}": (b, h) for b in range(B) for h in range(H)}


def hold(stage, tag, got, ref, r32, blocks, k=K_NOTE):
    """Every block of `got` within k x max(e32, 1e-7) of `ref`, errors relative to the block's largest reference value;
    prints each ratio first.  Returns the largest ratio gpu_err / max(e32, 1e-7)."""
    e32, eg = block_err(r32, ref, blocks), block_err(got, ref, blocks)
    bad, top = [], 0.0
    for name, e in eg.items():
        ratio = e / max(e32[name], FLOOR)
        top = max(top, ratio)
        print(f"RATIO | {stage} | {tag} | {name} | got {e:.2e} | e32 {e32[name]:.2e} | {ratio:.2f}")
        if not e <= bound(e32[name], k):
            bad.append((name, e, e32[name]))
    print(f"TOP | {stage} | {tag} | {top:.2f}")
    assert not bad, (stage, tag, bad[:8])
    return top


def bag_softmax(scores, off, lens=None):
    """w [R]: the softmax of `scores` over the rows [off[b], off[b] + lens[b]) of each bag (lens = the whole slot when None),
    0 on the rows behind the length inside the slot."""
    w = torch.zeros_like(scores)
    for b in range(len(off) - 1):
        n = off[b + 1] - off[b] if lens is None else int(lens[b])
        if n > 0:
            w[off[b]:off[b] + n] = scores[off[b]:off[b] + n].softmax(0)
    return w


def softmax_blocks(off, size=256):
    out = {}
    for b in range(len(off) - 1):
        out[f"bag{b}"] = (slice(off[b], off[b + 1]),)
        for t, r0 in enumerate(range(off[b], off[b + 1], size)):
            out[f"bag{b}.c{t}"] = (slice(r0, min(r0 + size, off[b + 1])),)
    return out


# --------------------------------------------------------------------------- model/sam/transformer.py, the three sites
def _ln(x, p, name):
    return F.layer_norm(x, (x.shape[-1],), p[name + ".weight"], p[name + ".bias"], 1e-5)


def _attention(q, k, v, p, name):
    """sam/transformer.py:428-450 for one bag -> (out_proj(attn v), weights [H, Tq, Tk])."""
    q = F.linear(q, p[name + ".q_proj.weight"], p[name + ".q_proj.bias"])
    k = F.linear(k, p[name + ".k_proj.weight"], p[name + ".k_proj.bias"])
    v = F.linear(v, p[name + ".v_proj.weight"], p[name + ".v_proj.bias"])
    c = q.shape[1] // H
    qh, kh, vh = (t.reshape(t.shape[0], H, c).transpose(0, 1) for t in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(c), dim=-1)
    out = (w @ vh).transpose(0, 1).reshape(q.shape[0], H * c)
    return F.linear(out, p[name + ".out_proj.weight"], p[name + ".out_proj.bias"]), w


def _mlp(x, p, name):
    return F.linear(torch.relu(F.linear(x, p[name + ".lin1.weight"], p[name + ".lin1.bias"])), p[name + ".lin2.weight"],
                    p[name + ".lin2.bias"])


def twoway_note_attention(image, image_pe, point, p, name, depth=2):
    """sam/transformer.py:100-120, 278-309 for one bag: image [N, E], image_pe [N, E], point [T, E] -> (the token->image
    softmax weights [H, T, N] of block 0, block 1 and the final attention, queries [T, E], keys [N, E])."""
    sites = []
    queries, keys = point, image
    for i in range(depth):
        b = f"{name}.layers.{i}"
        if i == 0:
            queries = _attention(queries, queries, queries, p, b + ".self_attn")[0]
        else:
            q = queries + point
            queries = queries + _attention(q, q, queries, p, b + ".self_attn")[0]
        queries = _ln(queries, p, b + ".norm1")
        o, w = _attention(queries + point, keys + image_pe, keys, p, b + ".cross_attn_token_to_image")
        sites.append(w)
        queries = _ln(queries + o, p, b + ".norm2")
        queries = _ln(queries + _mlp(queries, p, b + ".mlp"), p, b + ".norm3")
        keys = _ln(keys + _attention(keys + image_pe, queries + point, queries, p, b + ".cross_attn_image_to_token")[0], p,
                   b + ".norm4")
    o, w = _attention(queries + point, keys + image_pe, keys, p, name + ".final_attn_token_to_image")
    sites.append(w)
    return sites, _ln(queries + o, p, name + ".norm_final_attn"), keys
