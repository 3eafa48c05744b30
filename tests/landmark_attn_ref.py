"""Float64 torch restatement of the landmark-query pass of the Nystrom core (csrc/landmark_attn.hip: mil_tm_lmk_attn_fwd / _bwd),
in the style of transmil_ref.py: per head Q = qL [256, 64] (already scaled), K / V the k / v columns of the [n_pad, 1536] rows,
every row a key - W = softmax(Q K^T) V, lse = logsumexp(Q K^T), and from dW the gradients dkv [n_pad, 1024] (dk | dv, merged
heads) and dqL.  Written for any float dtype: float64 is the reference, float32 on the CPU gives e32, and a block of a GPU
result is held to transmil_ref.bound(e32, k).  mutate= plants one error (tests/test_landmark_attn_sensitivity_host.py)."""
import functools
import math

import torch

import fused_attn_common as C
import transmil_ref as R
from fused_attn_common import H, DH, M, D, heads, merged, pad_rows, ratios  # noqa: F401  (the tests reach them through here)

CHUNK = 256                      # keys per chunk of the chunked forms below
SIZES = (256, 512, 768, 1280)    # one chunk (the merge of a single partial), two, three, an odd number above
CASES = ("randn", "ramp_up", "ramp_down", "hot")
MUTATIONS = ("no_rescale", "lse_chunk0", "delta_zero", "pad_skipped", "dqL_last")
HOT = 110.0
# k of bound(e32, k): the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) of the first full run on
# an MI355X, capped at transmil_ref.K_CAP (docs/lab_notes.md has the tables).  "stage": the two entries through the C ABI,
# largest ratio 4.49 (hot, n_pad 1280, dkv.v_pad) -> 16; "core": nystrom_core(fused_a3=True) over transmil_ref.core_blocks,
# largest ratio 4.20 (n_pad 256, peak 3, dqkv.k_pad; the materialised route reads 2.76 there) -> 16.  Why the stage reads
# above the 1.5 of the chunked float32 restatement: the lab notes.
K_LMK = {"stage": 16, "core": 16}
hold = functools.partial(C.hold, "lmk", K_LMK)      # hold(stage, tag, got, ref, r32, blks, k=None): `RATIO | lmk_<stage> | ..`


def scores(qkv, qL):
    return qL @ heads(qkv[:, D:2 * D]).transpose(-1, -2)


_cases = {}


def case(name, n_pad):
    """(qkv [n_pad, 1536], qL [8, 256, 64], dW [8, 256, 64], pad), float64 holding float32 values; made once and shared."""
    key = (name, n_pad)
    if key not in _cases:
        assert name in CASES, name
        g = torch.Generator().manual_seed(7000 + n_pad)
        pad = pad_rows(n_pad)
        qkv = torch.randn((n_pad, 3 * D), generator=g, dtype=torch.float64)
        dW = torch.randn((H, M, DH), generator=g, dtype=torch.float64).float().double()
        qkv[:pad] = 0
        ramp = torch.linspace(0.5, 4.0, n_pad, dtype=torch.float64).reshape(-1, 1)
        if name == "ramp_up":
            qkv[:, D:2 * D] *= ramp
        elif name == "ramp_down":
            qkv[:, D:2 * D] *= ramp.flip(0)
        qkv = qkv.float().double()
        qL = R.landmarks(qkv, n_pad // M)[0].float().double()
        if name == "hot":
            qkv[:, D:2 * D] *= HOT / float(scores(qkv, qL).abs().max())
            qkv = qkv.float().double()
            top = float(scores(qkv, qL).abs().max())
            assert 100.0 <= top <= 120.0, top
        _cases[key] = (qkv, qL, dW, pad)
    return _cases[key]


def online(S, V):
    """softmax(S) V and logsumexp(S) chunk by chunk (CHUNK keys): a running maximum m and sum l, the sum and the output so far
    rescaled by exp(m_old - m_new) at every chunk - the forward as the kernels evaluate it, differentiable."""
    n = S.shape[-1]
    m = l = O = None
    for a in range(0, n, CHUNK):
        Sc = S[..., a:a + CHUNK]
        mc = Sc.detach().amax(-1)
        mn = mc if m is None else torch.maximum(m, mc)
        Pc = (Sc - mn[..., None]).exp()
        if m is None:
            l, O = Pc.sum(-1), Pc @ V[:, a:a + CHUNK]
        else:
            so = (m - mn).exp()
            l, O = l * so + Pc.sum(-1), O * so[..., None] + Pc @ V[:, a:a + CHUNK]
        m = mn
    return O / l[..., None], m + l.log()


def run(qkv, qL, dW, dtype=torch.float64, chunked=False):
    """The stage as it is defined: softmax over all keys, gradients through autograd.  chunked: the forward through online()."""
    x, q = (t.detach().to(dtype).clone().requires_grad_(True) for t in (qkv, qL))
    S = scores(x, q)
    if chunked:
        W, lse = online(S, heads(x[:, 2 * D:]))
    else:
        W, lse = S.softmax(-1) @ heads(x[:, 2 * D:]), S.logsumexp(-1)
    W.backward(dW.to(dtype))
    return {"W": W.detach(), "lse": lse.detach(), "dkv": x.grad[:, D:].clone(), "dqL": q.grad}


def run_formulas(qkv, qL, dW, dtype=torch.float64, pad=0, mutate=None, chunked=False):
    """The same through the formulas the kernels implement: P = exp(S - lse), delta = rowsum(dW o W), dV = P^T dW,
    dS = P o (dW V^T - delta), dK = dS^T Q, dqL = dS K.  chunked: the forward chunk by chunk (CHUNK keys) with a running
    maximum and sum, the backward chunk by chunk against the saved lse - what the kernels do, in `dtype`.  mutate: one of
    MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS, mutate
    qkv, Q, dW = qkv.to(dtype), qL.to(dtype), dW.to(dtype)
    n = qkv.shape[0]
    K, V = heads(qkv[:, D:2 * D]), heads(qkv[:, 2 * D:])
    S = Q @ K.transpose(-1, -2)
    if mutate == "pad_skipped":
        S = S.clone()
        S[..., :pad] = -math.inf
    cuts = [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)]
    if chunked or mutate == "no_rescale":
        m = torch.full((H, M), -math.inf, dtype=dtype)
        l = torch.zeros((H, M), dtype=dtype)
        O = torch.zeros((H, M, DH), dtype=dtype)
        for a, b in cuts:
            mc = S[..., a:b].amax(-1)
            Pc = (S[..., a:b] - mc[..., None]).exp()
            mn = torch.maximum(m, mc)
            so, sn = ((m - mn).exp(), (mc - mn).exp()) if mutate != "no_rescale" else (torch.ones_like(m), torch.ones_like(m))
            l = l * so + Pc.sum(-1) * sn
            O = O * so[..., None] + (Pc @ V[:, a:b]) * sn[..., None]
            m = mn
        W, lse = O / l[..., None], m + l.log()
    else:
        lse = S.logsumexp(-1)
        W = (S - lse[..., None]).exp() @ V
    if mutate == "lse_chunk0":
        lse = S[..., :CHUNK].logsumexp(-1)
    delta = (dW * W).sum(-1, keepdim=True)
    if mutate == "delta_zero":
        delta = torch.zeros_like(delta)
    dK, dV = torch.empty_like(K), torch.empty_like(V)
    dqL = torch.zeros_like(Q)
    for a, b in (cuts if chunked else [(0, n)]):
        P = (S[..., a:b] - lse[..., None]).exp()
        dV[:, a:b] = P.transpose(-1, -2) @ dW
        dS = P * (dW @ V[:, a:b].transpose(-1, -2) - delta)
        dK[:, a:b] = dS.transpose(-1, -2) @ Q
        part = dS @ K[:, a:b]
        dqL = part if (mutate == "dqL_last" and chunked) else dqL + part
    if mutate == "dqL_last" and not chunked:
        P = (S[..., n - CHUNK:] - lse[..., None]).exp()
        dqL = (P * (dW @ V[:, n - CHUNK:].transpose(-1, -2) - delta)) @ K[:, n - CHUNK:]
    return {"W": W, "lse": lse, "dkv": torch.cat([merged(dK), merged(dV)], 1), "dqL": dqL}


def blocks(n_pad, pad):
    """W, lse, dqL: all and each head.  dkv: the k and v column groups, each over all rows, the pad rows, the first and last
    16 rows and every 256-row chunk - a lost or doubled chunk shows in a block of its own."""
    dkv = {}
    for i, c in enumerate("kv"):
        for name, ix in C.row_blocks(n_pad, pad, CHUNK, (slice(D * i, D * (i + 1)),)).items():
            dkv[c if name == "all" else f"{c}_{name}"] = ix
    return {"W": C.per_head(), "lse": C.per_head(), "dkv": dkv, "dqL": C.per_head()}
