"""Generate the TransMIL golden vectors by running the REFERENCE's own model/dim1/TransMIL.py on CPU in float64.

Offline, in a checkout next to the reference (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_transmil.py --reference PATH/TO/REFERENCE

The reference module imports `nystrom_attention`, which is not installable here: a stub module takes its place whose
NystromAttention carries the package's parameters (to_qkv, to_out, res_conv) and computes its attention with the float64
restatement of tests/transmil_ref.py (itself pinned to transformers' Nystromformer by tests/test_transmil_host.py).  Two
more patches let the module run on CPU in float64: `Tensor.cuda` (TransMIL.py:82) and `Tensor.float` (:70) become the
identity.  Everything else (_fc1, square padding and repeats, cls token, PPEG, the two TransLayers, norm of the cls row) is
the reference's own code.  Weights: mil_amd.synthetic.transmil_params + head_params, loaded with load_state_dict; the head
is aggregator_clip's Dropout(0.25) + Linear(512, C) in eval mode, then sigmoid and BCELoss (train_ddp.py).

Writes tests/golden/transmil_N{7,250,1000,2000}.npz and transmil_ragged.npz (seed, lengths, labels, h, logits, prob, loss,
every parameter gradient and the x gradient as norm + stride-97 sample - the format of oracle/gen_golden.py, each file
below 1 MiB) and tests/golden/transmil_state_dict_keys.json."""
import argparse
import glob
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import mil_amd  # noqa: E402,F401
from mil_amd import synthetic as syn  # noqa: E402
import transmil_ref as R  # noqa: E402

SAMPLE_STRIDE = 97
MAX_FILE_BYTES = 960 * 1024
CASES = [("transmil_N7", 7, [7]), ("transmil_N250", 250, [250]), ("transmil_N1000", 1000, [1000]),
         ("transmil_N2000", 2000, [2000]), ("transmil_ragged", 3000, [7, 1000, 2000])]   # (tag, seed, lengths)


class NystromAttention(torch.nn.Module):
    """Stand-in for nystrom_attention.NystromAttention (same parameters; attention by the float64 restatement)."""

    def __init__(self, dim, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6, residual=True, dropout=0., **kw):
        super().__init__()
        assert (dim_head, heads, num_landmarks, pinv_iterations, residual) == (R.DH, R.H, R.M, R.ITERS, True)
        self.to_qkv = torch.nn.Linear(dim, 3 * heads * dim_head, bias=False)
        self.to_out = torch.nn.Sequential(torch.nn.Linear(heads * dim_head, dim), torch.nn.Dropout(dropout))
        self.res_conv = torch.nn.Conv2d(heads, heads, (R.CONV, 1), padding=(R.CONV // 2, 0), groups=heads, bias=False)

    def forward(self, x, return_attn=False):
        outs = [R.nystrom(x[b], self.to_qkv.weight, self.to_out[0].weight, self.to_out[0].bias, self.res_conv.weight,
                          return_attn=return_attn) for b in range(x.shape[0])]
        o = torch.stack([a for a, _ in outs])
        return (o, torch.stack([a for _, a in outs])) if return_attn else o


def load_reference(ref):
    stub = types.ModuleType("nystrom_attention")
    stub.NystromAttention = NystromAttention
    sys.modules["nystrom_attention"] = stub
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.float = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_transmil", os.path.join(ref, "model", "dim1", "TransMIL.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def npz(name, **arrs):
    out = {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()}
    groups, size = [{}], 0
    for k, v in out.items():
        if groups[-1] and size + v.nbytes > MAX_FILE_BYTES:
            groups.append({})
            size = 0
        groups[-1][k] = v
        size += v.nbytes
    for old in glob.glob(os.path.join(OUT, glob.escape(name) + ".part*.npz")):
        os.remove(old)
    for i, g in enumerate(groups):
        path = os.path.join(OUT, name + (".npz" if i == 0 else f".part{i}.npz"))
        np.savez_compressed(path, **g)
        print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB")


def pack(arrs, grads):
    for k, v in grads.items():
        arrs[k + ".norm"] = v.norm()
        arrs[k + ".sample"] = v.flatten()[::SAMPLE_STRIDE]


def bags_of(seed, lengths, L=768):
    return [torch.randn((n, L), generator=torch.Generator().manual_seed(seed + 100 + i), dtype=torch.float64)
            for i, n in enumerate(lengths)]


def gen(mod, tag, seed, lengths, L=768, C=2):
    p = {k: v.double() for k, v in syn.transmil_params(seed, L, C).items()}
    hp = {k: v.double() for k, v in syn.head_params(seed + 1, 512, C).items()}
    net = mod.TransMIL(n_classes=C, L=L).double().eval()
    net.load_state_dict(p)
    fc = torch.nn.Sequential(torch.nn.Dropout(0.25), torch.nn.Linear(512, C)).double().eval()
    fc.load_state_dict({k[len("fc."):]: v for k, v in hp.items()})
    bags = [b.requires_grad_(True) for b in bags_of(seed, lengths, L)]
    y = syn.make_labels(seed + 7, len(lengths), C).double()
    hs = [net(b.unsqueeze(0))[0] for b in bags]                  # [1, 512] each (aggregator_clip.py:109-118)
    h = torch.cat(hs, 0)
    z = fc(h)
    prob = torch.sigmoid(z)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    grads = {"g.extractor_pathology." + k: (v.grad if v.grad is not None else torch.zeros_like(v))
             for k, v in net.named_parameters()}
    grads.update({"g.fc.1." + k: v.grad for k, v in fc[1].named_parameters()})
    arrs = dict(seed=seed, lengths=np.array(lengths), labels=y, h=h, logits=z, prob=prob, loss=loss)
    pack(arrs, grads)
    pack(arrs, {"dx": torch.cat([b.grad for b in bags], 0)})
    npz(tag, **arrs)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds model/dim1/TransMIL.py)")
    a = ap.parse_args()
    torch.set_num_threads(8)
    mod = load_reference(a.reference)
    for tag, seed, lengths in CASES:
        net = gen(mod, tag, seed, lengths)
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(os.path.join(OUT, "transmil_state_dict_keys.json"), "w") as f:
        json.dump({"keys": keys}, f, indent=1)


if __name__ == "__main__":
    main()
