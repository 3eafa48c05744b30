"""What the two fused passes of the Nystrom core share in their tests (landmark_attn_ref.py / token_attn_ref.py and
test_gpu_landmark_attn.py / test_gpu_token_attn.py): the head layouts, the block builders and the bound check of the float64
restatements, and the sentinel buffers, the core runner and the golden checks of the GPU tests.  A plain module: nothing here
touches the GPU or the package until a helper that needs them is called."""
import argparse
import ctypes

import torch

import transmil_ref as R

H, DH, M, D = R.H, R.DH, R.M, R.H * R.DH


def pad_rows(n_pad):
    return 37 if n_pad > 256 else 3          # as transmil_ref.core_case has them


def heads(cols):
    """[n, 512] merged-head columns -> [8, n, 64]."""
    return cols.reshape(cols.shape[0], H, DH).transpose(0, 1)


def merged(t):
    """[8, n, 64] -> [n, 512]."""
    return t.transpose(0, 1).reshape(t.shape[1], D)


def per_head():
    """All heads and each head of an [8, ..] tensor."""
    blk = {"all": (Ellipsis,)}
    blk.update({f"h{h}": (h,) for h in range(H)})
    return blk


def row_blocks(n_pad, pad, chunk, cols=()):
    """All rows, the pad rows, the first and last 16 rows and every `chunk`-row chunk (a lost or doubled chunk shows in a block
    of its own), each over the columns `cols` (a tuple of further indices; () = all)."""
    rows = {"all": slice(None), "pad": slice(0, pad), "first16": slice(0, 16), "last16": slice(n_pad - 16, n_pad)}
    rows.update({f"chunk{j}": slice(chunk * j, chunk * (j + 1)) for j in range(n_pad // chunk)})
    return {name: (ix, *cols) for name, ix in rows.items()}


def ratios(got, ref, r32, blks):
    """{tensor.block: (error of got, e32, error / max(e32, FLOOR))}."""
    e32, eg = R.flat_err(r32, ref, blks), R.flat_err(got, ref, blks)
    return {b: (e, e32[b], e / max(e32[b], R.FLOOR)) for b, e in eg.items()}


def hold(prefix, k_table, stage, tag, got, ref, r32, blks, k=None):
    """Every block of every tensor of `got` within bound(e32, k) of `ref` (k = k_table[stage] unless given); prints each ratio
    first, as `RATIO | <prefix>_<stage> | ..`."""
    k = k_table[stage] if k is None else k
    bad = []
    for b, (e, e32, ratio) in ratios(got, ref, r32, blks).items():
        print(f"RATIO | {prefix}_{stage} | {tag} | {b} | gpu {e:.2e} | e32 {e32:.2e} | {ratio:.2f}")
        if not e <= R.bound(e32, k):
            bad.append((b, e, e32))
    assert not bad, (stage, tag, bad)


# ---- the GPU tests

DEV = torch.device("cuda:0")
SENT = -12345.678                    # the sentinel; the bit pattern is what is compared
GUARD = 64                           # floats of sentinel on either side of a buffer (a multiple of 4: operands stay 16-byte aligned)
MAP_BYTES = 8 * 256 * 4              # x n_pad: one A1 or A3 map


def _lib():
    from mil_amd import _lib as L
    return L.lib()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(numel, fill=None):
    """A device buffer of GUARD + numel + GUARD floats, all sentinel (or `fill` [numel] inside); returns (whole, inside view)."""
    buf = torch.full((numel + 2 * GUARD,), SENT, device=DEV, dtype=torch.float32)
    if fill is not None:
        buf[GUARD:GUARD + numel].copy_(fill.reshape(-1).to(torch.float32))
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(tag, buf):
    want = torch.full((GUARD,), SENT, dtype=torch.float32).view(torch.int32)
    b = _bits(buf)
    assert torch.equal(b[:GUARD], want) and torch.equal(b[-GUARD:], want), f"{tag}: wrote outside its extent"


def _core(qkv, w, dO, **kw):
    from mil_amd import ops
    qd = qkv.float().to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    o, attn = ops.nystrom_core(qd, wd, **kw)
    o.backward(dO.float().to(DEV))
    torch.cuda.synchronize()
    return {"out": o.detach(), "dqkv": qd.grad, "dw": wd.grad.reshape(R.H, R.CONV)}, attn


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _model(seed):
    from mil_amd import synthetic as syn
    from mil_amd.model.utils_clip import get_model
    args = argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    model = get_model(args)
    sd = {"extractor_pathology." + k: v for k, v in syn.transmil_params(seed, 768, 2).items()}
    sd.update(syn.head_params(seed + 1, 512, 2))
    model.load_state_dict(sd)
    return model.to(DEV).eval()


def _check_grads(model, g, extra=None):
    grads = {"g." + k: v.grad for k, v in model.named_parameters()}
    grads.update(extra or {})
    worst = 0.0
    for k, v in grads.items():
        if k.startswith("g.extractor_pathology._fc2"):
            assert v is None
            continue
        e = max(abs(float(v.norm()) - float(g[k + ".norm"])) / float(g[k + ".norm"]), rel(v.flatten()[::97], g[k + ".sample"]))
        assert e <= 2e-3, (k, e)
        worst = max(worst, e)
    return worst
