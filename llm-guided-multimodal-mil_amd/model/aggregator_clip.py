"""Image-only variant (reference: model/aggregator_clip.py:6-118, pathology branch :109-118):
`forward(x_list) -> (bag_embedding [B, F], sigmoid(fc(bag_embedding)) [B, C])` with ABMIL (F = L) or TransMIL (F = 512,
--model_pathology TransMIL) straight on the patch features.  This is BASELINE config 2's model; `trainer.ImageOnlyTrainer` is its fused step."""
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .dim1 import ABMIL, TransMIL


class aggregator(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        which = getattr(args, "model_pathology", "ABMIL")
        if list(args.modality) != ["pathology"] or which not in ("ABMIL", "TransMIL"):
            raise NotImplementedError("aggregator_clip: only modality ['pathology'] with ABMIL or TransMIL is on the built path")
        L = int(getattr(args, "patch_dim", 768))                     # aggregator_clip.py:36
        if which == "TransMIL":
            # aggregator_clip.py:47-52: the extractor gives h [B, 512] (its cls row), the head is Linear(512, C)
            self.extractor_pathology = TransMIL(n_classes=args.num_classes, L=L)
            F_out = self.extractor_pathology.D
        else:
            self.extractor_pathology = ABMIL(args, L=L)
            F_out = L
        self.fc = nn.Sequential(nn.Dropout(0.25), nn.Linear(F_out, args.num_classes))
        self.last_logits: Optional[torch.Tensor] = None
        # --transmil_graph 1 (train_ddp.build_model sets it): an eval-mode, no-grad forward of ONE bag - what test_ddp.py
        # runs per sample - is replayed from the hipGraph of the bag's grid side (transmil_step.RaggedTransMILStepper)
        self.graph_eval = False
        self._eval_stepper = None
        # TransMIL only (ABMIL keeps extractor_pathology.last_scores and ignores this): the forward also asks the extractor for
        # need_attn="cls" and leaves [a0, a1] - per layer a list with one [8, N_b] tensor per bag, the cls token's attention
        # to each patch - in last_patch_attn; the returned tuple does not change
        self.patch_attn = False
        self.last_patch_attn = None
        self._attn_dir, self._attn_names, self._attn_kept, self._attn_done = None, None, [], 0
        # ABMIL only: an eval-mode, no-grad forward also leaves the pool's softmax weights in last_bag_attn, one [N_b] tensor
        # per bag (ops.bag_softmax of extractor_pathology.last_scores); the returned tuple does not change
        self.note_attn = False
        self.last_bag_attn = None

    ATTN_KEEP_BYTES = 1 << 30

    def save_patch_attn_to(self, directory: str, names=None):
        """--save_patch_attn (train_ddp.build_model): every eval-mode, no-grad forward from here on keeps its bags' attention
        as one [2, 8, N] tensor ON THE DEVICE (one small device copy; the results of a replayed forward are the graph's static
        tensors), and flush_patch_attn() - registered to run when the process ends - copies them to the host and writes
        DIR/<names[i] or i>.npy, float32, bags numbered in the order they ran.  So an entry point that times each forward
        (test_ddp.py) has no host copy and no file inside its bracket.  Beyond ATTN_KEEP_BYTES kept, a forward flushes first."""
        import atexit
        import os
        os.makedirs(directory, exist_ok=True)
        self._attn_dir, self._attn_names = directory, (list(names) if names is not None else None)
        self.patch_attn = True
        atexit.register(self.flush_patch_attn)

    def flush_patch_attn(self):
        import os
        import numpy as np
        for a in self._attn_kept:
            i = self._attn_done
            name = str(self._attn_names[i]) if self._attn_names is not None and i < len(self._attn_names) else str(i)
            np.save(os.path.join(self._attn_dir, name + ".npy"), a.float().cpu().numpy())
            self._attn_done += 1
        self._attn_kept = []

    def _keep_patch_attn(self):
        if self._attn_dir is None or self.training or torch.is_grad_enabled():
            return
        if sum(a.numel() for a in self._attn_kept) * 4 > self.ATTN_KEEP_BYTES:
            self.flush_patch_attn()
        a0, a1 = self.last_patch_attn
        self._attn_kept += [torch.stack([x, y]) for x, y in zip(a0, a1)]

    def forward(self, x_list: List[torch.Tensor], lengths=None, geom=None):
        """geom (TransMIL only, model/dim1/TransMIL.py: DeviceGeometry): the capture-safe forward over a slot's static input,
        bag geometry on the device - the body trainer.RaggedTransMILStepper replays from a hipGraph."""
        x0 = x_list[0]
        if (self.graph_eval and geom is None and not self.training and not torch.is_grad_enabled() and x0.is_cuda
                and (x0.dim() == 2 or x0.shape[0] == 1) and (lengths is None or len(lengths) == 1)):
            return self._replayed_eval(x0.reshape(-1, x0.shape[-1]), lengths)
        want = "cls" if self.patch_attn and isinstance(self.extractor_pathology, TransMIL) else False
        if geom is not None:
            M = self.extractor_pathology(x_list[0], None, geom=geom, need_attn=want)
        elif want:
            M = self.extractor_pathology(x_list[0], lengths, need_attn=want)
        else:
            M = self.extractor_pathology(x_list[0], lengths)
        if isinstance(M, tuple):                     # TransMIL: (h, [attn0, attn1])
            if want:
                self.last_patch_attn = M[1]
            M = M[0]
        h = M
        if self.training and M.shape[1] % 32 == 0:
            # Dropout(.25) in front of the head (aggregator_clip.py / aggregator.py:129) from the SAME stream as the fused
            # route: Philox keep words keyed like ABMIL.flat_head_loss's (module seed ^ golden ratio, the pass counter the
            # patch mask of this forward has just advanced), not torch's generator (two training-mode streams)
            ab = self.extractor_pathology
            self.last_mbits = ops.dropout_keep_bits(M.shape[0], M.shape[1], ops.M_DROP_P, ab._drop_seed ^ 0x9E3779B97F4A7C15,
                                                    0, M.device, offset_dev=ab._drop_ctr)
            h = ops.dropout_bits(M, self.last_mbits, ops.M_DROP_SCALE)
        elif self.training:
            h = F.dropout(M, 0.25, True)
        p, z = ops.head_sigmoid(h, self.fc[1].weight, self.fc[1].bias)
        self.last_logits = z
        if self.note_attn and not self.training and not torch.is_grad_enabled():
            if not isinstance(self.extractor_pathology, ABMIL):
                raise NotImplementedError("note_attn gives the gated-attention pool's weights (ABMIL); TransMIL has patch_attn")
            from ..bags import BagLayout
            xs = x0 if x0.dim() == 3 else x0.unsqueeze(0)
            layout = BagLayout.make(lengths, x0.device) if lengths is not None else BagLayout.uniform(xs.shape[0], xs.shape[1], x0.device)
            scores = self.extractor_pathology.last_scores
            self.last_bag_attn = list(torch.split(ops.bag_softmax(scores, layout), list(layout.lengths)))
        if want and geom is None:
            self._keep_patch_attn()
        return M, p

    def _replayed_eval(self, x: torch.Tensor, lengths=None):
        """One bag [n, L] (rows [0, lengths[0]) of it) through the evaluation stepper: copied into the side's static input,
        forward replayed.  The results are the graph's static tensors, valid until that side's next forward."""
        if self._eval_stepper is None:
            from ..transmil_step import RaggedTransMILStepper
            self._eval_stepper = RaggedTransMILStepper(self, None, B=1, backward=False)
        st = self._eval_stepper
        n = int(lengths[0]) if lengths is not None else x.shape[0]
        slot = st.slot([n])
        slot.x[:n].copy_(x[:n], non_blocking=True)
        _, prob = st.step(slot, [n])
        self.last_logits = slot.last["logits"]
        if slot.last["patch_attn"] is not None:     # the side's static [8, s^2] tensors, cut to the bag
            self.last_patch_attn = [[a[:, :n] for a in layer] for layer in slot.last["patch_attn"]]
            self._keep_patch_attn()
        return slot.last["h"], prob
