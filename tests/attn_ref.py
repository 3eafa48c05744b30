"""Restatements of the fusion model's attention kernels (csrc/attention.hip, csrc/absorbed_attn.hip) for any float dtype:
softmax(q k^T / sqrt(C)) v per bag and per head (model/sam/transformer.py:428-450 of the reference after the projections,
clip/model.py:171-184 with the causal mask), its closed-form backward, and the one-text-token path with the k / v
projections absorbed into H query vectors and H pooled key vectors.  float64 is the reference, the same code in float32
on the CPU gives `e32`; mutate= plants one error (tests/test_attn_sensitivity_host.py shows that the per-block bounds of
tests/test_gpu_attn_stages.py see each of them).  Test-side helper: nothing here reads the code under test."""
import math

import torch

from transmil_ref import FLOOR, K_CAP, block_err, bound, flat_err  # noqa: F401  (re-exported to the two test files)

H, E = 8, 512
TILE, BLOCK = 64, 32                 # keys per pool tile, query rows per block of the rows-form backward
INF = math.inf

FWD_MUTATIONS = ("lasttile", "causal_off1", "head")
BWD_MUTATIONS = ("nodelta", "lasttile", "noscale", "causal_off1", "head")
ABSORBED_MUTATIONS = ("pe_in_value", "noacc", "cdot")


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


def f32exact(t):
    return t.float().double()


def _heads(x, nh):
    return x.reshape(x.shape[0], nh, -1).transpose(0, 1)                 # [rows, H C] -> [H, rows, C]


def _scores(qh, kh, C, causal, mutate):
    s = qh @ kh.transpose(-1, -2) / math.sqrt(C)
    if causal:
        i = torch.arange(s.shape[-2])[:, None]
        j = torch.arange(s.shape[-1])[None, :]
        s = s.masked_fill(j > i + (1 if mutate == "causal_off1" else 0), -INF)
    return s


def _keep(nk, mutate, dtype):
    """1 for the keys that enter the softmax sum.  "lasttile": those of the last partial 64-tile (behind a full one) do not."""
    w = torch.ones(nk, dtype=dtype)
    if mutate == "lasttile" and nk > TILE and nk % TILE:
        w[TILE * (nk // TILE):] = 0
    return w


def _swap_heads(lse):
    return lse[:, [1, 0] + list(range(2, lse.shape[1]))]


def attn(q, k, v, q_off, k_off, nh, causal=False, mutate=None):
    """q [Tq, H C], k, v [Tk, H C]; rows [q_off[b], q_off[b + 1]) attend to keys [k_off[b], k_off[b + 1]) -> (o [Tq, H C],
    lse [Tq, H]).  A bag without keys gives o = 0 and lse = -inf (the guard of k_attn_rows_fwd)."""
    assert mutate is None or mutate in FWD_MUTATIONS, mutate
    Tq, I = q.shape
    C = I // nh
    o = torch.zeros_like(q)
    lse = torch.full((Tq, nh), -INF, dtype=q.dtype)
    for b in range(len(q_off) - 1):
        q0, q1, k0, k1 = q_off[b], q_off[b + 1], k_off[b], k_off[b + 1]
        if q1 == q0 or k1 == k0:
            continue
        s = _scores(_heads(q[q0:q1], nh), _heads(k[k0:k1], nh), C, causal, mutate)          # [H, nq, nk]
        m = s.amax(-1, keepdim=True)
        p = (s - m).exp()
        l = (p * _keep(k1 - k0, mutate, q.dtype)).sum(-1, keepdim=True)
        o[q0:q1] = ((p @ _heads(v[k0:k1], nh)) / l).transpose(0, 1).reshape(q1 - q0, I)
        lse[q0:q1] = (m + l.log())[..., 0].t()
    if mutate == "head":
        lse = _swap_heads(lse)
    return o, lse


def attn_bwd(q, k, v, dO, q_off, k_off, nh, causal=False, mutate=None, o=None, lse=None):
    """(dq, dk, dv) in closed form: p = exp(s - lse), D = dO . O, ds = p (dO . v - D), dq = ds k / sqrt(C),
    dk = ds^T q / sqrt(C), dv = p^T dO.  One key: dq = dk = 0 exactly.  o, lse: the forward's (computed here if not given;
    given ones are cast to q's dtype, so a float32 rounding of the float64 forward can be fed to both dtypes).
    mutate: "nodelta" D dropped, "lasttile" the keys of the last partial 64-tile left out, "noscale" dk without 1 / sqrt(C),
    "causal_off1" the mask one further, "head" the lse of heads 0 and 1 swapped."""
    assert mutate is None or mutate in BWD_MUTATIONS, mutate
    if o is None:
        o, lse = attn(q, k, v, q_off, k_off, nh, causal, mutate if mutate in ("lasttile", "causal_off1") else None)
    o, lse = o.to(q.dtype), lse.to(q.dtype)
    if mutate == "head":
        lse = _swap_heads(lse)
    I = q.shape[1]
    C = I // nh
    sc = 1.0 / math.sqrt(C)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(len(q_off) - 1):
        q0, q1, k0, k1 = q_off[b], q_off[b + 1], k_off[b], k_off[b + 1]
        if q1 == q0 or k1 == k0:
            continue
        qh, kh, vh, gh, oh = (_heads(t, nh) for t in (q[q0:q1], k[k0:k1], v[k0:k1], dO[q0:q1], o[q0:q1]))
        s = _scores(qh, kh, C, causal, mutate)
        p = (s - lse[q0:q1].t()[..., None]).exp() * _keep(k1 - k0, mutate, q.dtype)
        D = 0.0 if mutate == "nodelta" else (gh * oh).sum(-1, keepdim=True)
        ds = p * (gh @ vh.transpose(-1, -2) - D)
        if k1 - k0 == 1:
            ds = torch.zeros_like(ds)
        merge = lambda t: t.transpose(0, 1).reshape(t.shape[1], I)                           # noqa: E731
        dq[q0:q1] = merge(ds @ kh) * sc
        dk[k0:k1] = merge(ds.transpose(-1, -2) @ qh) * (1.0 if mutate == "noscale" else sc)
        dv[k0:k1] = merge(p.transpose(-1, -2) @ gh)
    return dq, dk, dv


# --------------------------------------------------------------------------- block makers
def _span(off, b):
    return slice(off[b], off[b + 1])


def col_groups(nh, C, width=None):
    """Column groups of [rows, H C]: one per head, or per `width` columns (32 or 64)."""
    w = C if width is None else width
    return {f"c{i}": slice(w * i, w * (i + 1)) for i in range(nh * C // w)}


def bag_head_blocks(off, nh, C):
    """[rows, H C]: every (bag, head)."""
    return {f"bag{b}.h{h}": (_span(off, b), slice(C * h, C * (h + 1))) for b in range(len(off) - 1) for h in range(nh)}


def bag_blocks(off):
    return {f"bag{b}": (_span(off, b),) for b in range(len(off) - 1)}


def lse_blocks(off, nh, skip=()):
    """[rows, H]: every (bag, head) but the bags in `skip` (those without keys: -inf, compared exactly by the test)."""
    return {f"bag{b}.h{h}": (_span(off, b), h) for b in range(len(off) - 1) if b not in skip for h in range(nh)}


def slot_blocks(q_off, nh, C):
    """[rows, H C]: query slot t of every bag that has one, per head."""
    out = {}
    for t in range(max(q_off[b + 1] - q_off[b] for b in range(len(q_off) - 1))):
        rows = torch.tensor([q_off[b] + t for b in range(len(q_off) - 1) if q_off[b + 1] - q_off[b] > t])
        for h in range(nh):
            out[f"t{t}.h{h}"] = (rows, slice(C * h, C * (h + 1)))
    return out


def tail_blocks(off, size, name):
    """The last partial group of `size` rows of every bag (32: a block of the rows-form backward, 64: a key tile)."""
    out = {}
    for b in range(len(off) - 1):
        n = off[b + 1] - off[b]
        if n % size:
            out[f"bag{b}.{name}"] = (slice(off[b] + size * (n // size), off[b + 1]),)
    return out


def edge_rows(off):
    """First and last row of every bag."""
    out = {}
    for b in range(len(off) - 1):
        if off[b + 1] > off[b]:
            out[f"bag{b}.first"] = (slice(off[b], off[b] + 1),)
            out[f"bag{b}.last"] = (slice(off[b + 1] - 1, off[b + 1]),)
    return out


def key_rows(off):
    """Every single key row (the rows form: at most 16 per bag)."""
    return {f"bag{b}.k{r - off[b]}": (slice(r, r + 1),) for b in range(len(off) - 1) for r in range(off[b], off[b + 1])}


def q_blocks(c):
    """o, dq [Tq, H C]: per (bag, head), per query slot where bags are short (pool form), last partial 32-row block, first /
    last row per bag."""
    off, C = c["q_off"], c["C"]
    out = dict(bag_head_blocks(off, H, C))
    if max(off[b + 1] - off[b] for b in range(len(off) - 1)) <= 16:
        out.update(slot_blocks(off, H, C))
    out.update(tail_blocks(off, BLOCK, "blk32"))
    out.update(edge_rows(off))
    return out


def k_blocks(c):
    """dk, dv [Tk, H C]: per (bag, head), per bag, the last partial 64-key tile, first / last row; every key row where bags
    have at most 16 keys."""
    off, C = c["k_off"], c["C"]
    out = dict(bag_head_blocks(off, H, C))
    out.update(bag_blocks(off))
    out.update(tail_blocks(off, TILE, "tile64"))
    out.update(edge_rows(off))
    if max(off[b + 1] - off[b] for b in range(len(off) - 1)) <= 16:
        out.update(key_rows(off))
    return out


def fwd_blocks(c):
    nokeys = [b for b in range(len(c["k_off"]) - 1) if c["k_off"][b + 1] == c["k_off"][b]]
    return {"o": q_blocks(c), "lse": lse_blocks(c["q_off"], H, nokeys)}


def one_key_bags(c):
    return [b for b in range(len(c["k_off"]) - 1) if c["k_off"][b + 1] - c["k_off"][b] == 1]


def bwd_blocks(c, causal=False, exact=False):
    """exact: the entry states dq = dk = 0 of a one-key bag as exact zeros (the rows form's nk == 1 branch).  The other
    forms compute ds = p (dO . v - D) there with p = 1 and D = dO . v summed in another order: zero in exact arithmetic,
    rounding noise of the two terms in float32.  Their dq, dk blocks of a one-key bag - and, under the causal mask, dq of the
    first row of every sequence, which sees one key - are left out here and held by cancel_noise()."""
    out = {"dq": q_blocks(c), "dk": k_blocks(c), "dv": k_blocks(c)}
    if not exact:
        one = [f"bag{b}" for b in one_key_bags(c)]
        keep = lambda n: n.split(".")[0] not in one                                             # noqa: E731
        out["dq"] = {n: ix for n, ix in out["dq"].items() if keep(n) and not (causal and n.endswith(".first"))}
        out["dk"] = {n: ix for n, ix in out["dk"].items() if keep(n)}
    return out


NOISE_K = 16


def noise_bound(C):
    """A float32 dot product of C terms is off by about sqrt(C) 2^-24 of its size; ds is the difference of two."""
    return NOISE_K * math.sqrt(C) * 2.0 ** -23


def cancel_noise(c, got, causal=False):
    """{name: max|block| / (the size of the terms that cancel in it)} over the blocks bwd_blocks(exact=False) leaves out:
    |dq_i| against max_h|dO_i . v_0| max|k_0| / sqrt(C), |dk_0| against max|dO . v_0| max|q| / sqrt(C)."""
    C, q_off, k_off = c["C"], c["q_off"], c["k_off"]
    sc = 1.0 / math.sqrt(C)
    g = {n: t.detach().double().cpu() for n, t in got.items()}
    out = {}
    for b in range(len(q_off) - 1):
        q0, q1, k0, k1 = q_off[b], q_off[b + 1], k_off[b], k_off[b + 1]
        if q1 == q0 or k1 == k0 or not (k1 - k0 == 1 or causal):
            continue
        rows = slice(q0, q1) if k1 - k0 == 1 else slice(q0, q0 + 1)
        dp = (c["dO"][rows].reshape(-1, H, C) * c["v"][k0].reshape(H, C)).sum(-1).abs().max()
        out[f"dq.bag{b}"] = float(g["dq"][rows].abs().max()) / float(sc * dp * c["k"][k0].abs().max())
        if k1 - k0 == 1:
            out[f"dk.bag{b}"] = float(g["dk"][k0].abs().max()) / float(sc * dp * c["q"][rows].abs().max())
    return out


def expected_zero(c, tensor, name):
    """Is block `name` of `tensor` zero by construction?  o / dq of a bag without keys; dq, dk of a one-key bag; dk, dv of a
    bag without query rows.  (Blocks over several bags - the query slots - are never all zero.)"""
    if not name.startswith("bag"):
        return False
    b = int(name[3:].split(".")[0])
    nq, nk = c["q_off"][b + 1] - c["q_off"][b], c["k_off"][b + 1] - c["k_off"][b]
    if tensor in ("o", "dq"):
        return nk == 0 or (tensor == "dq" and nk == 1)
    if tensor == "dk":
        return nq == 0 or nk == 1
    return nq == 0


# --------------------------------------------------------------------------- the cases (shared by the host and GPU tests)
ROWS_BAGS = [(1, 1), (31, 2), (32, 15), (33, 16), (70, 10), (0, 5), (5, 0)]        # (query rows, keys)
ROWS_BWD_BAGS = ROWS_BAGS[:-1]
CAUSAL_LENS = [1, 7, 16]
GEN_BAGS = [(17, 40), (160, 70), (1, 300), (40, 17)]
POOL_RAGGED = [(1, 1), (2, 3), (10, 63), (16, 64), (3, 65), (16, 130), (1, 200)]  # (T, keys), Tmax 16
POOL_SINGLE = [(10, 200)]
POOL_PEAKED = [(16, 130), (3, 200), (1, 65)]
SEQ_LENS = [1, 17, 31, 32, 33, 77, 96]
ABS_BAGS = [1, 63, 64, 65, 130, 700]
ABS_SINGLE = [130]
PEAK_Q, PEAK_SHIFT, PEAK_KEY = 3.0, 80.0, 14.0


def attn_case(bags, C, seed=0, peaked=False):
    """float32-exact inputs held in float64: q, dO [Tq, H C], k, v [Tk, H C] randn.  peaked: q times PEAK_Q; per bag and head
    a common vector along that head's first query is added to all keys (that query's scores move to +PEAK_SHIFT on even
    heads, -PEAK_SHIFT on odd ones) and key (64 h + 13) mod n gets PEAK_KEY more, so that the largest score of head h lies
    in another tile per head."""
    g = torch.Generator().manual_seed(9000 + 97 * seed + C + 13 * len(bags) + sum(a * 3 + b for a, b in bags))
    q_off, k_off = offsets(a for a, _ in bags), offsets(b for _, b in bags)
    I = H * C
    q = torch.randn((q_off[-1], I), generator=g, dtype=torch.float64)
    k = torch.randn((k_off[-1], I), generator=g, dtype=torch.float64)
    v = torch.randn((k_off[-1], I), generator=g, dtype=torch.float64)
    dO = torch.randn((q_off[-1], I), generator=g, dtype=torch.float64)
    if peaked:
        q = f32exact(q * PEAK_Q)
        for b in range(len(bags)):
            n = k_off[b + 1] - k_off[b]
            for h in range(H):
                cols = slice(C * h, C * (h + 1))
                u = q[q_off[b], cols]
                u = u * math.sqrt(C) / float(u @ u)                       # q0 . u / sqrt(C) = 1
                shift = PEAK_SHIFT if h % 2 == 0 else -PEAK_SHIFT
                k[k_off[b]:k_off[b + 1], cols] += shift * u
                r = k_off[b] + (TILE * h + 13) % n                        # that key scores +-PEAK_SHIFT + PEAK_KEY
                k[r, cols] += (shift + PEAK_KEY - float(q[q_off[b], cols] @ k[r, cols]) / math.sqrt(C)) * u
    return dict(q=f32exact(q), k=f32exact(k), v=f32exact(v), dO=f32exact(dO), q_off=q_off, k_off=k_off, C=C)


def seq_case(lens, C, seed=0):
    return attn_case([(n, n) for n in lens], C, seed + 50)


def fwd_run(c, dtype=torch.float64, causal=False, mutate=None):
    o, lse = attn(c["q"].to(dtype), c["k"].to(dtype), c["v"].to(dtype), c["q_off"], c["k_off"], H, causal, mutate)
    return {"o": o, "lse": lse}


def bwd_run(c, dtype=torch.float64, causal=False, mutate=None, fwd=None):
    """fwd: {"o", "lse"} to take as the forward's result (the GPU tests feed the float32 rounding of the float64 forward to
    the entry and to the float32 restatement alike); None: the restatement's own forward in `dtype`."""
    o, lse = (None, None) if fwd is None else (fwd["o"].float(), fwd["lse"].float())
    dq, dk, dv = attn_bwd(c["q"].to(dtype), c["k"].to(dtype), c["v"].to(dtype), c["dO"].to(dtype), c["q_off"], c["k_off"], H,
                          causal, mutate, o, lse)
    return {"dq": dq, "dk": dk, "dv": dv}


# --------------------------------------------------------------------------- the one-token absorbed path
def absorbed_case(lens, C, seed=0):
    """keys [N, E], pe a table of max(lens) + 9 rows (row = position in the bag), qp, dO [B, H C], Wk, Wv [H C, E], bv [H C],
    dkeys_acc [N, E]: float32-exact, in float64."""
    g = torch.Generator().manual_seed(7000 + 31 * seed + C + sum(lens))
    B, N, I = len(lens), sum(lens), H * C
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    c = dict(keys=r(N, E), pe=0.5 * r(max(lens) + 9, E), qp=r(B, I), Wk=r(I, E) / math.sqrt(E), Wv=r(I, E) / math.sqrt(E),
             bv=r(I), dO=r(B, I), dkeys_acc=r(N, E))
    c = {n: f32exact(t) for n, t in c.items()}
    c.update(k_off=offsets(lens), C=C)
    return c


def _pe_rows(pe, k_off):
    return torch.cat([pe[:k_off[b + 1] - k_off[b]] for b in range(len(k_off) - 1)], 0)


def unabsorbed(c, acc=True):
    """float64 autograd of sam/transformer.py:428-450 with one query row per bag: k = k_proj(keys + pe) (its bias is a
    constant per softmax row and left out), v = v_proj(keys) -> o and the gradients of keys (+ dkeys_acc if acc), qp, Wk,
    Wv, bv under dO."""
    C, k_off = c["C"], c["k_off"]
    t = {n: c[n].detach().clone().requires_grad_(True) for n in ("keys", "qp", "Wk", "Wv", "bv")}
    kp = (t["keys"] + _pe_rows(c["pe"], k_off)) @ t["Wk"].t()
    vp = t["keys"] @ t["Wv"].t() + t["bv"]
    o = []
    for b in range(len(k_off) - 1):
        n = k_off[b + 1] - k_off[b]
        s = torch.einsum("hc,nhc->hn", t["qp"][b].reshape(H, C), kp[k_off[b]:k_off[b + 1]].reshape(n, H, C)) / math.sqrt(C)
        o.append(torch.einsum("hn,nhc->hc", s.softmax(-1), vp[k_off[b]:k_off[b + 1]].reshape(n, H, C)).reshape(-1))
    o = torch.stack(o)
    o.backward(c["dO"])
    out = {"o": o.detach(), "dkeys": t["keys"].grad + (c["dkeys_acc"] if acc else 0), "dqp": t["qp"].grad, "dWk": t["Wk"].grad,
           "dWv": t["Wv"].grad, "dbv": t["bv"].grad}
    return out


def absorb_query(qp, Wk, C):
    """Qp[b][h] = Wk_h^T qp[b][h]   [B, H, E]"""
    B = qp.shape[0]
    return torch.einsum("bhc,hce->bhe", qp.reshape(B, H, C), Wk.reshape(H, C, -1))


def absorb_query_bwd(qp, Wk, dQp, C):
    B = qp.shape[0]
    dqp = torch.einsum("bhe,hce->bhc", dQp, Wk.reshape(H, C, -1)).reshape(B, H * C)
    dWk = torch.einsum("bhc,bhe->hce", qp.reshape(B, H, C), dQp).reshape(H * C, -1)
    return dqp, dWk


def absorbed_pool(keys, pe, Qp, k_off, C, mutate=None):
    """pooled[b][h] = sum_n softmax_n(Qp[b][h] . (keys_n + pe_n) / sqrt(C)) keys_n, lse [B, H]."""
    kin = keys + _pe_rows(pe, k_off).to(keys.dtype)
    val = kin if mutate == "pe_in_value" else keys
    pooled, lse = [], []
    for b in range(len(k_off) - 1):
        s = Qp[b] @ kin[k_off[b]:k_off[b + 1]].t() / math.sqrt(C)                            # [H, n]
        m = s.amax(-1, keepdim=True)
        p = (s - m).exp()
        l = p.sum(-1, keepdim=True)
        pooled.append((p @ val[k_off[b]:k_off[b + 1]]) / l)
        lse.append((m + l.log())[:, 0])
    return torch.stack(pooled), torch.stack(lse)


def absorbed_pool_bwd(keys, pe, Qp, lse, dpooled, pooled, k_off, C, dkeys_acc=None, mutate=None):
    """a = exp(scale Qp . kin - lse), da = dpooled . keys, cdot = dpooled . pooled, ds = a (da - cdot);
    dkeys_n = sum_h a dpooled_h + scale ds Qp_h (+ dkeys_acc), dQp_h = scale sum_n ds kin_n."""
    sc = 1.0 / math.sqrt(C)
    kin = keys + _pe_rows(pe, k_off).to(keys.dtype)
    dkeys, dQp = torch.zeros_like(keys), torch.zeros_like(Qp)
    for b in range(len(k_off) - 1):
        rows = slice(k_off[b], k_off[b + 1])
        a = (Qp[b] @ kin[rows].t() * sc - lse[b][:, None]).exp()                             # [H, n]
        da = dpooled[b] @ keys[rows].t()
        cdot = 0.0 if mutate == "cdot" else (dpooled[b] * pooled[b]).sum(-1, keepdim=True)
        ds = a * (da - cdot)
        dkeys[rows] = a.t() @ dpooled[b] + sc * ds.t() @ Qp[b]
        dQp[b] = sc * ds @ kin[rows]
    if dkeys_acc is not None and mutate != "noacc":
        dkeys = dkeys + dkeys_acc
    return dkeys, dQp


def value_proj(pooled, Wv, bv, C):
    B = pooled.shape[0]
    return torch.einsum("bhe,hce->bhc", pooled, Wv.reshape(H, C, -1)).reshape(B, H * C) + bv


def value_proj_bwd(dO, Wv, pooled, C):
    B = dO.shape[0]
    g = dO.reshape(B, H, C)
    return (torch.einsum("bhc,hce->bhe", g, Wv.reshape(H, C, -1)), torch.einsum("bhc,bhe->hce", g, pooled).reshape(H * C, -1),
            dO.sum(0))


def absorbed(c, dtype=torch.float64, given=None, acc=True, mutate=None):
    """The absorbed arithmetic, stage by stage, in `dtype`.  given: a result of this function (the float64 one) whose
    float32 rounding every stage takes as its inputs instead of this run's own intermediates - one entry under test at a
    time, for the kernels and for the float32 restatement alike."""
    assert mutate is None or mutate in ABSORBED_MUTATIONS, mutate
    C, k_off = c["C"], c["k_off"]
    t = {n: c[n].to(dtype) for n in ("keys", "pe", "qp", "Wk", "Wv", "bv", "dO", "dkeys_acc")}
    src = (lambda n, own: own) if given is None else (lambda n, own: given[n].float().to(dtype))   # noqa: E731
    r = {}
    r["Qp"] = absorb_query(t["qp"], t["Wk"], C)
    Qp = src("Qp", r["Qp"])
    r["pooled"], r["lse"] = absorbed_pool(t["keys"], t["pe"], Qp, k_off, C, mutate)
    pooled, lse = src("pooled", r["pooled"]), src("lse", r["lse"])
    r["o"] = value_proj(pooled, t["Wv"], t["bv"], C)
    r["dpooled"], r["dWv"], r["dbv"] = value_proj_bwd(t["dO"], t["Wv"], pooled, C)
    dpooled = src("dpooled", r["dpooled"])
    r["dkeys"], r["dQp"] = absorbed_pool_bwd(t["keys"], t["pe"], Qp, lse, dpooled, pooled, k_off, C,
                                             t["dkeys_acc"] if acc else None, mutate)
    r["dqp"], r["dWk"] = absorb_query_bwd(t["qp"], t["Wk"], src("dQp", r["dQp"]), C)
    return r


def absorbed_ref(c, acc=True):
    """The reference of every tensor of the path: o and the parameter / input gradients from the unabsorbed float64 formula,
    the intermediates that only the absorbed form has (Qp, pooled, lse, dpooled, dQp) from its float64 run."""
    r = absorbed(c, acc=acc)
    r.update(unabsorbed(c, acc))
    return r


def absorbed_blocks(c):
    """[N, E] rows per bag + last partial 64-key tile + first / last row; [B, H, E] per (bag, head); [B, H C] per (bag, head);
    [H C, E] and [H C] per head.  dQp of a one-key bag is left out: it is a difference of two equal dot products (ds = a (da -
    cdot) with a = 1, pooled = keys), zero in exact arithmetic and rounding noise in any float32 order - onekey_noise(); so
    is dqp of that bag, the product of Wk with that noise."""
    C, off = c["C"], c["k_off"]
    B = len(off) - 1
    one = [b for b in range(B) if off[b + 1] - off[b] == 1]
    rows = dict(bag_blocks(off))
    rows.update(tail_blocks(off, TILE, "tile64"))
    rows.update(edge_rows(off))
    bhe = {f"bag{b}.h{h}": (b, h) for b in range(B) for h in range(H)}
    bh = {f"bag{b}.h{h}": (b, h) for b in range(B) for h in range(H)}
    bic = {f"bag{b}.h{h}": (b, slice(C * h, C * (h + 1))) for b in range(B) for h in range(H)}
    w = {f"h{h}": (slice(C * h, C * (h + 1)),) for h in range(H)}
    many = lambda d: {n: ix for n, ix in d.items() if ix[0] not in one}                     # noqa: E731
    return {"Qp": bhe, "pooled": bhe, "lse": bh, "o": bic, "dpooled": bhe, "dWv": w, "dbv": w, "dkeys": rows,
            "dQp": many(bhe), "dqp": many(bic), "dWk": w}


def onekey_noise(c, ref, got):
    """{bag: max|dQp[bag]| / (scale max_h|dpooled_h . keys_0| max|kin_0|)} for the one-key bags: the size of dQp there
    relative to the two terms that cancel - float32 rounding leaves a few 1e-7 of them."""
    off, C = c["k_off"], c["C"]
    out = {}
    for b in range(len(off) - 1):
        if off[b + 1] - off[b] == 1:
            key = c["keys"][off[b]]
            norm = float((ref["dpooled"][b] @ key).abs().max()) * float((key + c["pe"][0]).abs().max()) / math.sqrt(C)
            out[b] = float(got["dQp"][b].detach().double().cpu().abs().max()) / norm
    return out


# k of bound(e32, k) per stage: the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) that the first
# full run on an MI355X showed (the table "fusion attention stages" in docs/lab_notes.md), capped at K_CAP
K_STAGE = {"rows_fwd": 8, "rows_bwd": 8, "gen_bwd": 16, "pool_fwd": 16, "pool_bwd": 16, "seq_fwd": 16, "seq_bwd": 8,
           "absorb": 4, "absorbed_pool": 8}


def hold(stage, tag, got, ref, r32, blocks):
    """Every block of every tensor of `got` within bound(e32, K_STAGE[stage]) of `ref`; prints each ratio first."""
    blocks = {t: blocks[t] for t in got}
    e32, eg = flat_err(r32, ref, blocks), flat_err(got, ref, blocks)
    bad = []
    for b, e in eg.items():
        print(f"RATIO | {stage} | {tag} | {b} | gpu {e:.2e} | e32 {e32[b]:.2e} | {e / max(e32[b], FLOOR):.2f}")
        if not e <= bound(e32[b], K_STAGE[stage]):
            bad.append((b, e, e32[b]))
    assert not bad, (stage, tag, bad)
