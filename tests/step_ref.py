"""Test helpers for the fp32 image-only step (csrc/step.hip, mil_image_only_step_run): a mirror of the host rules that
pick its gate-forward and weight-gradient kernels, the library's own statement of them (mil_gate_step_route) in the
mirror's terms, and a plain float64 restatement of the whole step (gates, scores, softmax pool, head, loss and the
gradients of all eight parameters) that runs on the device."""
import ctypes
import os

import torch

from mil_amd import _lib
from mil_amd.trainer import PARAM_ORDER

WV, BV = "aggregator.attention_V.0.weight", "aggregator.attention_V.0.bias"
WU, BU = "aggregator.attention_U.0.weight", "aggregator.attention_U.0.bias"
WW, WB = "aggregator.attention_weights.weight", "aggregator.attention_weights.bias"
WF, BF = "fc.1.weight", "fc.1.bias"

GF_TM = 128          # rows per k_gate_fwd2 workgroup (gate_fwd.hip GF_TM)
GS_TM = 32           # rows per k_gate_fwd_r32 row tile (GS_TM)
SMALL_ROWS = 64      # MIL_SMALL_ROWS


def num_cu() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def r32_rt(R: int, ncu: int) -> int:
    """Row tiles per k_gate_fwd_r32 workgroup (gate_fwd.hip: gate_r32_rt)."""
    tiles = (R + GS_TM - 1) // GS_TM
    return 1 if tiles <= ncu else 2 if tiles <= 2 * ncu else 3


def split_kg(R: int, L: int, ncu: int) -> int:
    """K groups per weight-gradient workgroup (gate_bwd_dw.hip: gate_dw_plan)."""
    smax = ncu // (3 * (L // 128))
    return 2 if smax >= 1 and R // smax >= 512 else 1


def dw_route(R: int, L: int, ncu: int) -> str:
    """The fp32 weight-gradient kernel (gate_route_plan, launched by gate_bwd_partials_impl)."""
    kg = split_kg(R, L, ncu)
    return "dw2" if kg == 2 and R * L < (1 << 29) else f"dw<{kg}>"


def dw_split(R: int, L: int, ncu: int):
    """(S, kc): row chunks of the weight gradient's split-K and rows per chunk, a multiple of 32 (gate_route_plan)."""
    smax = max((2 * ncu // split_kg(R, L, ncu)) // (3 * (L // 128)), 1)
    kc = max(((R + smax - 1) // smax + 31) // 32 * 32, 32)
    return (R + kc - 1) // kc, kc


def step_route(R: int, L: int, C: int, train: bool, *, aligned32: bool = False, bucketed: bool = False,
               pieces: bool = True, ncu: int = None, given_bits: bool = False) -> dict:
    """Which kernels ImageOnlyTrainer.forward(x, layout, y) + backward() launch for the fp32 step with labels (gates
    saved).  R is the bucket capacity for a bucketed (DeviceBagLayout) batch.

    main:   'r32' (k_gate_fwd_r32), 'fwd2_pw' (k_gate_fwd2<.., PW = true>), 'fwd2' (its fp32-MFMA K loop) or 'legacy'
            (k_gate_fwd, L > 4096)
    rt:     RT of the r32 launch that carries the whole batch
    tail:   None, 'small' (rows beyond whole rounds, <= 64) or 'big' (<= 1024 rows beyond whole rounds)
    tail_rows: rows that leave the main kernel for the tail kernel (0: none)
    tail_kernel / tail_rt: 'linear_small' (mil_linear_small_fwd + k_gate_tail_scores) or 'r32' and its RT
    bits:   train mode only: 'in_kernel' (drawn by k_gate_fwd2<.., GEN = true>) or 'generator' (a launch of its own);
            given_bits (not train: the gate forward alone, with keep bits the caller made): 'given'
    pool:   'fused' (pool partial pass in k_gate_fwd2's epilogue) or 'alone' (k_pool_partial)
    dw:     'dw<1>', 'dw<2>' (k_gate_bwd_dw<.., KG>) or 'dw2' (k_gate_bwd_dw2)
    S, kc:  row chunks of the weight gradient's split-K, rows per chunk
    """
    ncu = ncu or num_cu()
    fused_entry = _fused_entry(C, aligned32, bucketed)
    pw = pieces and L % 32 == 0                       # trainer.py: ImageOnlyTrainer.gate_pieces; step.hip: Wp
    # gate_fwd.hip: gate_route_plan
    r32 = (R + GF_TM - 1) // GF_TM < (3 * ncu) // 4
    tail, big = 0, False
    if not r32:
        t, full = R % GF_TM, R // GF_TM
        if 1 <= t <= SMALL_ROWS and full >= ncu and full % ncu == 0:           # gate_tail_rows
            tail = t
        else:
            over = R % (GF_TM * ncu)
            if R >= GF_TM * ncu and 0 < over <= 1024:
                tail, big = over, True
    fwd2 = L <= 4096
    pool_in = fused_entry and not r32 and tail == 0 and fwd2 and L == 512 and R % 32 == 0
    in_kernel = not r32 and tail == 0 and fwd2 and L <= 1024 and L % 128 == 0
    S, kc = dw_split(R, L, ncu)
    out = dict(main="r32" if r32 else "legacy" if not fwd2 else ("fwd2_pw" if pw else "fwd2"),
               rt=r32_rt(R, ncu) if r32 else None, tail=None, tail_rows=tail, tail_kernel=None, tail_rt=None, bits=None,
               pool="fused" if pool_in else "alone", dw=dw_route(R, L, ncu), S=S, kc=kc)
    if tail:
        out["tail"] = "big" if big else "small"
        if big or train or given_bits:             # keep bits: the 32-row kernel applies them while staging
            out["tail_kernel"], out["tail_rt"] = "r32", r32_rt(tail, ncu)
        else:
            out["tail_kernel"] = "linear_small"
    if train:
        out["bits"] = "in_kernel" if in_kernel else "generator"
    elif given_bits:
        out["bits"] = "given"
    return out


def _fused_entry(C: int, aligned32: bool, bucketed: bool) -> bool:
    """Whether mil_image_only_step_run asks for the pool pass in the forward's epilogue at all (step.hip: the
    gate_fwd_with_pool branch; use_h holds for C <= 4 with labels)."""
    fuse_env = os.environ.get("MIL_FUSE_POOL", "1")[:1] != "0"
    return aligned32 and C == 2 and not bucketed and fuse_env


_MAIN = ("r32", "fwd2", "fwd2_pw", "legacy")                  # MIL_ROUTE_MAIN_*
_TAIL = (None, "small", "big")                                # MIL_ROUTE_TAIL_*
_TAIL_KERNEL = (None, "linear_small", "r32")                  # MIL_ROUTE_TAIL_KERNEL_*
_BITS = (None, "given", "in_kernel", "generator")             # MIL_ROUTE_BITS_*
_DW = ("dw<1>", "dw<2>", "dw2")                               # MIL_ROUTE_DW_*


def lib_route(R: int, L: int, C: int, train: bool, *, aligned32: bool = False, bucketed: bool = False,
              pieces: bool = True, ncu: int = None, given_bits: bool = False) -> dict:
    """The library's own route for the same step (mil_gate_step_route: the plan its launches execute), in step_route's
    terms.  ncu None: the library plans for the device it runs on."""
    p = _lib.GateRoute()
    keep = _BITS.index("generator" if train else "given" if given_bits else None)
    rc = _lib.lib().mil_gate_step_route(R, L, C, 1, keep, int(pieces),
                                        int(_fused_entry(C, aligned32, bucketed)), int(bucketed), ncu or 0, ctypes.byref(p))
    assert rc == 0, rc
    return dict(main=_MAIN[p.main], rt=p.rt or None, tail=_TAIL[p.tail], tail_kernel=_TAIL_KERNEL[p.tail_kernel],
                tail_rt=p.tail_rt or None, bits=_BITS[p.bits], pool="fused" if p.pool_fused else "alone", dw=_DW[p.dw] if p.dw >= 0 else None,
                S=p.S, kc=p.kc, tail_rows=p.tail_rows)


# ------------------------------------------------------------------------------------------ float64 reference
def keep_from_bits(bits: torch.Tensor, L: int) -> torch.Tensor:
    """[n][L/32] keep words (bit j of word k = column 32 k + j) -> float64 0/1 [n, L], on the words' device."""
    b = bits.view(torch.int32).long() & 0xFFFFFFFF
    sh = torch.arange(32, device=bits.device)
    return ((b.unsqueeze(-1) >> sh) & 1).view(b.shape[0], L).to(torch.float64)


def gates_ref(x: torch.Tensor, p: dict, keep_x: torch.Tensor = None):
    """float64 (scores [R], gates [R, 384] = [tanh(V) | sigmoid(U)]) of the (dropped) rows x."""
    xd = x.to(torch.float64)
    if keep_x is not None:
        xd = xd * keep_x * 2.0
    d = {k: p[k].to(x.device, torch.float64) for k in (WV, BV, WU, BU, WW, WB)}
    v = torch.tanh(xd @ d[WV].t() + d[BV])
    u = torch.sigmoid(xd @ d[WU].t() + d[BU])
    s = (v * u) @ d[WW].view(-1) + d[WB]
    return s, torch.cat([v, u], 1)


def step_ref(x: torch.Tensor, lengths, p: dict, y: torch.Tensor, loss: str, keep_x=None, keep_m=None) -> dict:
    """The whole step in float64 on x's device: ABMIL gated attention (ABMIL.py:47-59) over each bag, head with its
    Dropout(.25) (aggregator.py:128-131), BCELoss (<= 2 classes) or CrossEntropyLoss on the sigmoid outputs (> 2), mean
    over the bags, and torch.autograd gradients of every parameter.  keep_x [R, L] / keep_m [B, L]: 0/1 keep masks of a
    train-mode pass (None: eval)."""
    dev = x.device
    leaves = {k: p[k].detach().to(dev, torch.float64).requires_grad_(True) for k in PARAM_ORDER}
    xd = x.to(torch.float64)
    if keep_x is not None:
        xd = xd * keep_x * 2.0
    B, L = len(lengths), x.shape[1]
    v = torch.tanh(xd @ leaves[WV].t() + leaves[BV])
    u = torch.sigmoid(xd @ leaves[WU].t() + leaves[BU])
    s = (v * u) @ leaves[WW].view(-1) + leaves[WB]
    bid = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(list(lengths), device=dev))
    smax = torch.full((B,), float("-inf"), device=dev, dtype=torch.float64).scatter_reduce(0, bid, s.detach(), "amax")
    e = torch.exp(s - smax[bid])
    A = e / torch.zeros(B, device=dev, dtype=torch.float64).index_add(0, bid, e)[bid]
    M = torch.zeros(B, L, device=dev, dtype=torch.float64).index_add(0, bid, A.unsqueeze(1) * xd)
    if keep_m is not None:
        M = M * keep_m * (1.0 / 0.75)
    z = M @ leaves[WF].t() + leaves[BF]
    prob = torch.sigmoid(z)
    yd = y.to(dev, torch.float64)
    if loss == "bce":
        lp = torch.clamp(torch.log(prob), min=-100.0)
        l1p = torch.clamp(torch.log(1.0 - prob), min=-100.0)
        lval = (-(yd * lp + (1.0 - yd) * l1p)).mean()
    else:
        lval = (-(yd * torch.log_softmax(prob, 1)).sum(1)).mean()
    grads = torch.autograd.grad(lval, [leaves[k] for k in PARAM_ORDER])
    return dict(scores=s.detach(), gates=torch.cat([v, u], 1).detach(), logits=z.detach(), prob=prob.detach(),
                loss=float(lval.detach()), grads=dict(zip(PARAM_ORDER, grads)))


def max_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref|, element-wise over the whole tensor."""
    got = got.to(ref.device, torch.float64)
    return float((got - ref).abs().max() / ref.abs().max())
