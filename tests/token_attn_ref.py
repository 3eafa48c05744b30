"""Float64 torch restatement of the token-query pass of the Nystrom core (csrc/token_attn.hip: mil_tm_tok_attn_fwd / _bwd), in
the style of landmark_attn_ref.py: per head Q = the q columns of the [n_pad, 1536] rows (every row a query), K = kL [256, 64]
(not scaled), V = U [256, 64] - S = 64^-0.5 Q kL^T, O = softmax(S) U [n_pad, 512] with the heads merged, lse = logsumexp(S)
[8, n_pad], and from dO [n_pad, 512] the gradients dq [n_pad, 512], dU and dkL [8, 256, 64].  Written for any float dtype:
float64 is the reference, float32 on the CPU gives e32, and a block of a GPU result is held to transmil_ref.bound(e32, k).
mutate= plants one error (tests/test_token_attn_sensitivity_host.py)."""
import functools

import torch

import fused_attn_common as C
import transmil_ref as R
from fused_attn_common import H, DH, M, D, heads, merged, pad_rows, ratios  # noqa: F401  (the tests reach them through here)

QSCALE = DH ** -0.5
CHUNK = 256                      # rows per chunk of the backward's two sums over the rows
SIZES = (256, 512, 768, 1280)    # one row chunk (the reduce of a single partial), two, three, an odd number above
CASES = ("randn", "ramp_up", "ramp_down", "hot")
MUTATIONS = ("lse_half", "delta_zero", "scale_missing", "dU_last", "dkL_last", "pad_skipped")
HOT = 110.0
# k of bound(e32, k): the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) of the first full run on
# an MI355X, capped at transmil_ref.K_CAP (docs/lab_notes.md has the tables).  "stage": the two entries through the C ABI,
# largest ratio 3.40 (ramp_down, n_pad 768, dq.last16) -> 8; "core": nystrom_core with fused_a1 x fused_a3 in all four
# combinations over transmil_ref.core_blocks, largest ratio 4.20 (n_pad 256, peak 3, dqkv.k_pad, with fused_a1 off and fused_a3
# on, as landmark_attn_ref has it; 3.27 on the same block with both on, 3.24 on dqkv.q_pad with fused_a1 alone) -> 16.
K_TOK = {"stage": 8, "core": 16}
hold = functools.partial(C.hold, "tok", K_TOK)      # hold(stage, tag, got, ref, r32, blks, k=None): `RATIO | tok_<stage> | ..`


def scores(qkv, kL):
    return QSCALE * (heads(qkv[:, :D]) @ kL.transpose(-1, -2))


_cases = {}


def case(name, n_pad):
    """(qkv [n_pad, 1536], kL [8, 256, 64], U [8, 256, 64], dO [n_pad, 512], pad), float64 holding float32 values; made once
    and shared.  The front pad rows of qkv are zero; dO is NOT zero there: the stage treats all rows alike."""
    key = (name, n_pad)
    if key not in _cases:
        assert name in CASES, name
        g = torch.Generator().manual_seed(9000 + n_pad)
        pad = pad_rows(n_pad)
        qkv = torch.randn((n_pad, 3 * D), generator=g, dtype=torch.float64)
        U = torch.randn((H, M, DH), generator=g, dtype=torch.float64).float().double()
        dO = torch.randn((n_pad, D), generator=g, dtype=torch.float64).float().double()
        qkv[:pad] = 0
        ramp = torch.linspace(0.5, 4.0, n_pad, dtype=torch.float64).reshape(-1, 1)
        if name == "ramp_up":
            qkv[:, :D] *= ramp
        elif name == "ramp_down":
            qkv[:, :D] *= ramp.flip(0)
        qkv = qkv.float().double()
        kL = R.landmarks(qkv, n_pad // M)[1].float().double()
        if name == "hot":
            qkv[:, :D] *= HOT / float(scores(qkv, kL).abs().max())
            qkv = qkv.float().double()
            top = float(scores(qkv, kL).abs().max())
            assert 100.0 <= top <= 120.0, top
        _cases[key] = (qkv, kL, U, dO, pad)
    return _cases[key]


def run(qkv, kL, U, dO, dtype=torch.float64):
    """The stage as it is defined: softmax over the 256 landmarks, gradients through autograd."""
    x, k, u = (t.detach().to(dtype).clone().requires_grad_(True) for t in (qkv, kL, U))
    S = scores(x, k)
    O, lse = merged(S.softmax(-1) @ u), S.logsumexp(-1)
    O.backward(dO.to(dtype))
    return {"O": O.detach(), "lse": lse.detach(), "dq": x.grad[:, :D].clone(), "dU": u.grad, "dkL": k.grad}


def run_formulas(qkv, kL, U, dO, dtype=torch.float64, pad=0, mutate=None, chunked=False):
    """The same through the formulas the kernels implement: P = exp(S - lse), dP = dO_h U^T, delta = rowsum(P o dP),
    dS = P o (dP - delta), dq = QSCALE dS kL, dU = sum over the rows of P^T dO_h, dkL = QSCALE sum over the rows of dS^T Q.
    chunked: the two sums over the rows as one partial per CHUNK rows, added chunk 0, 1, 2 .. - what the kernels do, in
    `dtype`.  mutate: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS, mutate
    qkv, kL, U, dO = qkv.to(dtype), kL.to(dtype), U.to(dtype), dO.to(dtype)
    n = qkv.shape[0]
    Q, dOh = heads(qkv[:, :D]), heads(dO)
    S = QSCALE * (Q @ kL.transpose(-1, -2))
    lse = S.logsumexp(-1)
    O = (S - lse[..., None]).exp() @ U
    lse_b = S[..., :M // 2].logsumexp(-1) if mutate == "lse_half" else lse
    P = (S - lse_b[..., None]).exp()
    dP = dOh @ U.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    if mutate == "delta_zero":
        delta = torch.zeros_like(delta)
    dS = P * (dP - delta)
    dq = (dS @ kL) * (1.0 if mutate == "scale_missing" else QSCALE)
    first = pad if mutate == "pad_skipped" else 0
    cuts = [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)] if (chunked or mutate in ("dU_last", "dkL_last")) else [(0, n)]
    dU, dkL = torch.zeros_like(U), torch.zeros_like(kL)
    for a, b in cuts:
        a = max(a, first)
        pu = P[:, a:b].transpose(-1, -2) @ dOh[:, a:b]
        pk = QSCALE * (dS[:, a:b].transpose(-1, -2) @ Q[:, a:b])
        dU = pu if mutate == "dU_last" else dU + pu
        dkL = pk if mutate == "dkL_last" else dkL + pk
    return {"O": merged(O), "lse": lse, "dq": merged(dq), "dU": dU, "dkL": dkL}


def blocks(n_pad, pad):
    """O and dq: all rows, the pad rows, the first and last 16 rows and every 256-row chunk - a lost or doubled chunk shows in a
    block of its own.  lse, dU, dkL: all heads and each head."""
    rows = C.row_blocks(n_pad, pad, CHUNK)
    return {"O": dict(rows), "lse": C.per_head(), "dq": dict(rows), "dU": C.per_head(), "dkL": C.per_head()}
