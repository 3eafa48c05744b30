"""Generate tests/golden/fusion_transmil_small.npz: the fusion model with the TransMIL aggregator (fusion_transmil=1), modality
['pathology'], whose aggregator stage is the REFERENCE's own model/dim1/TransMIL.py at L = 512 run on CPU in float64.

Offline, in a checkout next to the reference (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fusion_transmil.py --reference PATH/TO/REFERENCE

Case: the `fused_small_clip` configuration of oracle/gen_golden.py (seed 91, two CLIP layers of width 512, full vocabulary)
with B = 2 ragged bags of 7 and 250 patches and P = 1 note.  Parameters: synthetic.fused_params (its ABMIL aggregator keys
left out of the model) plus synthetic.transmil_params(seed, L=512, prefix="aggregator.").  Per bag, all in float64: the
multi-modal bag x0 = cat([x_Pth2CI, x_CI2Pth]) (aggregator.py:192) from the pieces of oracle.mil_oracle.fused_forward, through
the reference's TransMIL (tools/gen_golden_transmil.py: load_reference, with its nystrom_attention stand-in), element 0 of
its tuple through the head, sigmoid, BCELoss over the batch.  Stored: seed, lengths, labels, h, logits, prob, loss, x_Pth2CI
and every live gradient (parameters and the patches) as norm + stride-97 sample (samples in float32: one file below
960 KiB)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_golden_transmil import MAX_FILE_BYTES, OUT, SAMPLE_STRIDE, load_reference, npz  # noqa: E402
from mil_amd import synthetic as syn  # noqa: E402
from oracle import mil_oracle as orc  # noqa: E402

TAG, SEED, LENGTHS, P = "fusion_transmil_small", 91, [7, 250], 1
CLIP = dict(clip_layers=2, clip_width=512, clip_vocab=49408)
CLIP_HEADS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds model/dim1/TransMIL.py)")
    a = ap.parse_args()
    torch.set_num_threads(8)
    B = len(LENGTHS)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in syn.fused_params(SEED, "TwoWayTransformer_Pth", **CLIP).items()}
    live = [k for k in p if not k.startswith("clinic_extractor.") and not k.startswith("aggregator.")]
    q = dict(p)
    q.update({k: p[k].clone().requires_grad_(True) for k in live})
    tm = {k[len("aggregator."):]: v.double() for k, v in syn.transmil_params(SEED, L=512, prefix="aggregator.").items()}
    x = syn.make_bags(SEED + 3, B, max(LENGTHS), 768).double()
    bags = [x[b, :n].clone().requires_grad_(True) for b, n in enumerate(LENGTHS)]
    ids = syn.make_token_ids(SEED + 4, B, P)
    y = syn.make_labels(SEED + 5, B).double()
    mod = load_reference(a.reference)        # patches Tensor.float / .cuda: after the synthetic inputs are made
    net = mod.TransMIL(n_classes=2, L=512).double().eval()
    net.load_state_dict(tm)
    hs, toks = [], []
    for b in range(B):
        o = orc.fused_forward(bags[b], ids[b], q, CLIP_HEADS)
        x0 = torch.cat([o["x_Pth2CI"], o["x_CI2Pth"]], 0)          # aggregator.py:192: the note's tokens first
        hs.append(net(x0.unsqueeze(0))[0])                          # [1, 512]: element 0 of TransMIL's tuple
        toks.append(o["x_Pth2CI"].detach())
    h = torch.cat(hs, 0)
    z, prob = orc.head_forward(h, q)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    grads = {"g." + k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in live}
    grads.update({"g.aggregator." + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in net.named_parameters()})
    grads["dx"] = torch.cat([b.grad for b in bags], 0)
    arrs = dict(seed=SEED, lengths=np.array(LENGTHS), labels=y, h=h, logits=z, prob=prob, loss=loss, x_Pth2CI=torch.stack(toks, 0))
    for k, v in grads.items():
        arrs[k + ".norm"] = v.norm()
        arrs[k + ".sample"] = v.flatten()[::SAMPLE_STRIDE].to(torch.float32)   # (.float() is patched away)
    npz(TAG, **arrs)
    size = os.path.getsize(os.path.join(OUT, TAG + ".npz"))
    assert size < MAX_FILE_BYTES and not os.path.exists(os.path.join(OUT, TAG + ".part1.npz")), size


if __name__ == "__main__":
    main()
