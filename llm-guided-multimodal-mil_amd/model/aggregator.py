"""`aggregator(args)`: the drop-in boundary of the path (reference: model/aggregator.py:9-209).

Same constructor (`args.modality`, `args.model_pathology`, `args.model_CI`, `args.aggregator`,
`args.num_classes`), same `forward(x_list, x_CI)` and return tuples, same state_dict keys - but every
tensor op on the path runs through the HIP library:

    fc_pathology (GEMM + tanh) -> clinic_extractor (frozen CLIP text tower, cached per note)
    -> fc_CI2Pth (GEMM + tanh) -> TwoWayTransformer (text <-> patches) -> multi-modal bag [text | patches]
    -> aggregator (gated-attention MIL pool) -> fc + sigmoid.

Differences, all deliberate: a batch is B independent bags (the reference's B>1 ABMIL
degenerates to a sum); CT encoders / TransMIL / tabular-CI MLPs are out of scope and raise; the positional
table lives on the device (the reference re-uploads `pe[:, :N]` every forward, aggregator.py:160-190);
`last_logits` exposes the pre-sigmoid scores for the parity checks.

`args.fusion_transmil` (opt-in, default off; without it `aggregator="TransMIL"` and `model_pathology="TransMIL"` raise as
they always did): the multi-modal bag is aggregated by TransMIL (dim1/TransMIL.py, csrc/transmil.hip) - upstream's default
`--aggregator` and the authors' own run.  TransMIL depends on the order of a bag's rows, so each branch hands `_pool_head`
the bag's pieces in upstream's sequence order (aggregator.py:173,184,192,195) while the rows stay where they lie in memory;
the sequence is assembled through an index written on the device (ops.tm_seq_index_segs).  Upstream feeds TransMIL's
returned TUPLE `(h, attn)` into `self.fc` (aggregator.py:199-200), which cannot run; the dataflow built here is element 0,
`h [B, 512]`, into `fc`.  Bags run one after another, on the eager autograd path; `bucket=` is taken only from
fusion_step.RaggedFusionTransMILStepper, whose bucket carries the TransMIL geometry of the step's key (`bucket.tm_geom`: sides
from the key, gather index written on the device, TransMIL.flat_bucket) - any other bucket raises as before.
`model_pathology="TransMIL"` builds `extractor_pathology` for the state_dict alone (aggregator.py:54-56): never called."""
import math
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import lifetime, ops
from ..bags import BagLayout
from .sam.transformer import TwoWayTransformer

EMBED = 512
HEAD_DROP_KEY = 0x48656164467573      # the head's Dropout(0.25) on the replayed TransMIL-aggregator step: seed ^ this


def _arg(args, name, default):
    return getattr(args, name, default)


def _offsets(lengths):
    """First row of each bag when the bags lie back to back."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return off


class aggregator(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        modality = list(args.modality)
        # 'CT' in modality: the CT ENCODERS (torchvision / MONAI 3-D backbones, model/dim3/*) stay outside the hot path, but
        # their output - the feature map [B, 512, 160, h, w] of aggregator.py:139-140 - is accepted as x_list[0], precomputed
        # (extractor_CT is the identity here), and everything downstream of it is built: map -> tokens, fc_CI2CT,
        # TwoWayTransformer_CT / _Both, the 4-segment multi-modal bag (:155-184).
        mk_twoway = lambda: TwoWayTransformer(args=args, depth=2, embedding_dim=EMBED, num_heads=8, mlp_dim=2048)  # noqa: E731
        self.fc_CI2CT = nn.Sequential(nn.Linear(EMBED, EMBED), nn.Tanh())                 # aggregator.py:44
        if "pathology" in modality:
            self.fc_pathology = nn.Sequential(nn.Linear(768, EMBED), nn.Tanh())           # :47
            if _arg(args, "model_pathology", "ABMIL") == "ABMIL":
                from .dim1 import ABMIL
                self.extractor_pathology = ABMIL(args, L=EMBED)                           # :50 (built, never called)
            elif args.model_pathology == "TransMIL" and _arg(args, "fusion_transmil", 0):
                from .dim1 import TransMIL
                self.extractor_pathology = TransMIL(n_classes=args.num_classes, L=EMBED)  # :54-56 (built, never called)
            elif args.model_pathology not in ("-", None):
                raise NotImplementedError(f"model_pathology={args.model_pathology}: only ABMIL is on the built path by default; "
                                          "TransMIL is built with fusion_transmil=1 (--fusion_transmil 1)")
            self.TwoWayTransformer_Pth = mk_twoway()                                      # :58
        if "CT" in modality:
            self.TwoWayTransformer_CT = mk_twoway()                                       # :36
        self.fc_CI2Pth = nn.Sequential(nn.Linear(EMBED, EMBED), nn.Tanh())                # :66
        self.fc_CI = nn.Sequential(nn.Linear(EMBED, EMBED), nn.Tanh())                    # :68
        self.TwoWayTransformer_Both = mk_twoway()                                         # :70
        agg = _arg(args, "aggregator", "ABMIL")
        if agg == "ABMIL":
            from .dim1 import ABMIL
            self.aggregator = ABMIL(args, L=EMBED)                                        # :81
        elif agg == "TransMIL" and _arg(args, "fusion_transmil", 0):
            from .dim1 import TransMIL
            self.aggregator = TransMIL(n_classes=args.num_classes, L=EMBED)               # :85-87
        elif agg != "-":
            raise NotImplementedError(f"aggregator={agg}: TransMIL over the multi-modal bag is opt-in, set fusion_transmil=1 "
                                      "(--fusion_transmil 1; eager autograd path only); ABMIL_v2 is not on the built path")
        if _arg(args, "model_CI", "CLIP") == "CLIP":
            from .dim1 import CLIP
            self.clinic_extractor = CLIP(args)                                            # :122
        else:
            raise NotImplementedError(f"model_CI={args.model_CI}: only the CLIP text extractor is on the built path")
        self.prompt_embedding = nn.Parameter(torch.randn(1, EMBED))                       # :124 (unused upstream too)
        self.fc = nn.Sequential(nn.Dropout(0.25), nn.Linear(EMBED, args.num_classes))     # :128-131
        self._pe: Optional[torch.Tensor] = None
        self.last_logits: Optional[torch.Tensor] = None
        self.last_loss: Optional[torch.Tensor] = None
        self.last_pooled: Optional[torch.Tensor] = None    # op-by-op tail only (the fused pool + head + loss node keeps no M)
        self._labels: Optional[torch.Tensor] = None
        self._loss_scale: Optional[float] = None
        # note_attn: an eval-mode, no-grad forward of the pathology (+ text) model also leaves, per bag,
        #   last_note_attn[site][bag]  [8, N_b] (P = 1 text token per bag; [P, 8, N_b] for P = 2 .. 12): the softmax weights of
        #       the note's token(s) over the bag's patches at the three token->image attention sites - block 0, block 1, the
        #       final attention of TwoWayTransformer_Pth - every head summing to 1 over the patches;
        #   last_bag_attn[bag]  [N_b + P]: the final gated-attention aggregator's weights over the multi-modal bag, PATCHES
        #       FIRST, then the note's tokens - the order of the rows in memory (upstream concatenates the tokens first,
        #       aggregator.py:192; pooling does not depend on the order).  With a TransMIL aggregator [2, 8, N_b + P] = layers
        #       x heads x rows: the cls token's attention to each row of the bag (a repeated row's two keys summed, not
        #       renormalised; ops.tm_cls_attention), in the same patches-first order.
        # Off: the forward issues exactly the launches it always did and both stay None.  The returned tuple never changes.
        # note_attn = "all" (True keeps the scope above, and its refusals): the same export wherever the three token->image
        # sites run on the absorbed one-token / multi-token pools - CT in the modality, the capacity-bucket forwards, the
        # replayed evaluation.  It adds
        #   last_note_attn_ct[site][bag]  [8, D] ([P, 8, D]): the note's weights over the D CT tokens at the three sites of the
        #       transformer that ran the CT side (TwoWayTransformer_CT; the first pass through TwoWayTransformer_Both with
        #       pathology beside it - last_note_attn then comes from the second pass; None for ['CT'] alone);
        #   last_bag_attn[bag] over the bag's rows in memory order: [D + P] for ['CT'] (CT tokens, text tokens),
        #       [N_b + P + D + P] for CT + pathology (patches, CT-side text tokens, CT tokens, pathology-side text tokens).
        # The work is split in two: the launches run inside the forward, read nothing from the host and leave their results in
        # capacity shape (_note_device: capture-safe, a graph's static outputs); note_attn_finish(lengths) slices them per bag
        # by the step's host lengths afterwards.  A forward without bucket= calls both; with bucket= the caller calls the second
        # (fusion_step.RaggedFusionInference / RaggedFusionTransMILStepper do, after the replay).
        self.note_attn = False
        self.last_note_attn = None
        self.last_note_attn_ct = None
        self.last_bag_attn = None
        self._tm_bag_attn = None
        self._note_ctx, self._note_meta, self._note_tensors = None, None, None
        self._tm_geom, self._tm_len_dev = None, None       # set per forward from bucket.tm_geom (the replayed TransMIL step)
        self.last_head_bits = None
        # graph_eval (train_ddp.build_model sets it for --fusion_transmil_graph 1): an eval-mode, no-grad forward of ONE bag
        # given as the reference gives it - model([ct,] x [1, N, F], ids) - is replayed from the graph of its key
        # (fusion_step.RaggedFusionTransMILStepper without backward, the text tower inside the replay); test_ddp.py's loop
        self.graph_eval = False
        self._eval_stepper = None
        self._note_dir, self._note_names, self._note_kept, self._note_done = None, None, [], 0

    NOTE_KEEP_BYTES = 1 << 30

    def save_note_attn_to(self, directory: str, names=None):
        """--save_note_attn (train_ddp.build_model): every eval-mode, no-grad forward from here on keeps its bags' weights ON
        THE DEVICE (note [3, P, 8, N] and bag [N + P] - [2, 8, N + P] with a TransMIL aggregator - per bag), and flush_note_attn() - registered to run when the process
        ends - copies them to the host and writes DIR/<names[i] or i>.npz, float32, bags numbered in the order they ran: an
        entry point that times each forward has no host copy and no file inside its bracket.  Beyond NOTE_KEEP_BYTES kept, a
        forward flushes first.  Under note_attn = "all" with CT in the modality the file gains note_ct [3, P, 8, D], note is
        there only with pathology, and bag covers the whole multi-modal bag in memory order."""
        import atexit
        import os
        os.makedirs(directory, exist_ok=True)
        self._note_dir, self._note_names = directory, (list(names) if names is not None else None)
        self.note_attn = True
        atexit.register(self.flush_note_attn)

    def flush_note_attn(self):
        import os
        import numpy as np
        for kept in self._note_kept:
            i = self._note_done
            name = str(self._note_names[i]) if self._note_names is not None and i < len(self._note_names) else str(i)
            np.savez(os.path.join(self._note_dir, name + ".npz"),
                     **{k: v.float().cpu().numpy() for k, v in zip(("note", "bag", "note_ct"), kept) if v is not None})
            self._note_done += 1
        self._note_kept = []

    def _keep_note_attn(self):
        if self._note_dir is None or self.last_bag_attn is None or (self.last_note_attn is None
                                                                    and self.last_note_attn_ct is None):
            return
        if sum(t.numel() for kept in self._note_kept for t in kept if t is not None) * 4 > self.NOTE_KEEP_BYTES:
            self.flush_note_attn()
        stack = lambda sites, b: torch.stack([site[b].reshape(-1, 8, site[b].shape[-1]) for site in sites])   # noqa: E731
        for b, bag in enumerate(self.last_bag_attn):
            note = stack(self.last_note_attn, b) if self.last_note_attn is not None else None
            if self.last_note_attn_ct is None:
                self._note_kept.append((note, bag.clone()))
            else:                                          # note_ct [3, P, 8, D]; stack() copies, like note
                self._note_kept.append((note, bag.clone(), stack(self.last_note_attn_ct, b)))

    def _wants_note_attn(self) -> bool:
        return bool(self.note_attn) and not self.training and not torch.is_grad_enabled()

    def _note_all(self) -> bool:
        return isinstance(self.note_attn, str) and self.note_attn == "all"

    def _note_device(self, sites):
        """note_attn = "all", inside the forward: the weights of the token->image sites from what their kernels held (three
        records per branch, in the order the branches ran) - one mil_absorbed_pool_attn launch per one-token site, the
        softmaxed score matrix the multi-token pool holds anyway - and the aggregator's weights (ABMIL: ops.bag_softmax of its
        scores; TransMIL: the cls attention _pool_head asked for).  Nothing here reads the host; every tensor keeps the shape
        of its buffer (a capacity bucket: zeros behind the bags).  Leaves (_note_meta, _note_tensors) for note_attn_finish."""
        ctx = self._note_ctx
        if len(sites) != 3 * len(ctx["branches"]):
            raise NotImplementedError(f"note_attn: {len(sites)} of the {3 * len(ctx['branches'])} token->image attention sites "
                                      "(three per branch) ran on the absorbed one-token / multi-token pool; the general "
                                      "attention_pool route keeps no weights")
        tensors, TH = [], []
        for rec in sites:
            if "A" in rec:          # P = 2 .. 12: the softmaxed score matrix [rows, P 8 (+ padding)], column t 8 + h
                tensors.append(rec["A"])
                TH.append(int(rec["TH"]))
            else:
                tensors.append(ops.absorbed_pool_attention(rec["keys"], rec["pe"], rec["Qp"], rec["lse"], rec["segs"], rec["C"]))
                TH.append(8)
        meta = dict(ctx, TH=TH, bag=None)
        agg = getattr(self, "aggregator", None)
        if self._is_transmil():
            if ctx["cap"] is None:                         # host lengths: _pool_head has sliced and reordered already
                meta["bag"] = "final"
                tensors += list(self._tm_bag_attn)
            else:                                          # [attn0, attn1], each one static [8, s_b^2] per bag
                meta["bag"] = "transmil"
                tensors += list(self._tm_bag_attn[0]) + list(self._tm_bag_attn[1])
        elif agg is not None and getattr(agg, "last_scores", None) is not None:
            meta["bag"] = "rows" if ctx["cap"] is not None else "bags"
            tensors.append(ops.bag_softmax(agg.last_scores, ctx["layout"]))
        meta["count"] = len(tensors)
        self._note_meta, self._note_tensors = meta, tensors

    def note_attn_finish(self, lengths=None, tensors=None):
        """note_attn = "all", after the forward: slice what _note_device left per bag.  lengths: the step's patch counts on the
        host (the capacity-bucket forwards; a forward without bucket= has called this itself).  tensors: the static outputs
        of a replayed graph standing in for the tensors of the pass that was captured.  Views only - _keep_note_attn clones."""
        meta = self._note_meta
        if meta is None:
            return
        ts = list(tensors) if tensors is not None else self._note_tensors
        B, P, D, cap, tail = meta["B"], meta["P"], meta["D"], meta["cap"], meta["tail"]
        n_len = [int(n) for n in (lengths if lengths is not None else meta["n_len"] or [])]
        if "pth" in meta["branches"] and len(n_len) != B:
            raise ValueError(f"note_attn_finish: {B} bags, lengths {n_len}")
        offs = dict(ct=_offsets([D] * B), pth=_offsets(n_len))
        out = {}
        for i, br in enumerate(meta["branches"]):
            off, sites = offs[br], []
            for X, TH in zip(ts[3 * i:3 * i + 3], meta["TH"][3 * i:3 * i + 3]):
                per = [X[off[b]:off[b + 1], :TH].t() for b in range(B)]
                sites.append([a.reshape(P, TH // P, -1) for a in per] if P > 1 else per)
            out[br] = sites
        self.last_note_attn, self.last_note_attn_ct = out.get("pth"), out.get("ct")
        bag = ts[3 * len(meta["branches"]):]
        T = sum(tail)                                      # the static rows behind a bag's patches
        off = offs["pth"] if n_len else [0] * (B + 1)
        if meta["bag"] == "final":
            self.last_bag_attn = bag
        elif meta["bag"] == "bags":
            self.last_bag_attn = list(torch.split(bag[0], list(meta["layout"].lengths)))
        elif meta["bag"] == "rows":
            # the bucket's rows: [cap patch rows | segment 0 of every bag | segment 1 of every bag | ..]
            w, base = bag[0], cap
            pieces = [[w[off[b]:off[b + 1]]] for b in range(B)]
            for rows in tail:
                for b in range(B):
                    pieces[b].append(w[base + b * rows:base + (b + 1) * rows])
                base += B * rows
            self.last_bag_attn = [torch.cat(p) for p in pieces]
        elif meta["bag"] == "transmil":
            # sequence order of the bucket form: [tail segments | patches]; exported: patches first
            self.last_bag_attn = []
            for b in range(B):
                a = torch.stack([bag[b], bag[B + b]])      # [2, 8, s_b^2]: layers x heads x sequence rows
                n = off[b + 1] - off[b]
                self.last_bag_attn.append(torch.cat([a[..., T:T + n], a[..., :T]], -1))
        self._keep_note_attn()

    def _note_attention(self, sites, n_len, P, layout):
        """After the forward: the weights of the three token->image sites from what their kernels held (`sites`,
        ops.note_sites), one launch per site, and the aggregator's weights from its scores."""
        if len(sites) != 3:
            raise NotImplementedError(f"note_attn: {len(sites)} of the 3 token->image attention sites ran on the absorbed "
                                      "one-token / multi-token pool; the general attention_pool route keeps no weights")
        off = [0]
        for n in n_len:
            off.append(off[-1] + int(n))
        out = []
        for rec in sites:
            if "A" in rec:      # P = 2 .. 12: views of the softmaxed score matrix [rows, P 8 (+ padding)], column t 8 + h
                A, TH = rec["A"], rec["TH"]
                out.append([A[off[b]:off[b + 1], :TH].t().reshape(P, TH // P, -1) for b in range(len(n_len))])
            else:
                a = ops.absorbed_pool_attention(rec["keys"], rec["pe"], rec["Qp"], rec["lse"], rec["segs"], rec["C"])
                out.append([a[off[b]:off[b + 1]].t() for b in range(len(n_len))])
        self.last_note_attn = out
        self._bag_attention(layout)
        self._keep_note_attn()

    def _bag_attention(self, layout):
        agg = getattr(self, "aggregator", None)
        if self._is_transmil():
            self.last_bag_attn = self._tm_bag_attn
        elif agg is not None and getattr(agg, "last_scores", None) is not None:
            self.last_bag_attn = list(torch.split(ops.bag_softmax(agg.last_scores, layout), list(layout.lengths)))

    # ------------------------------------------------------------------ positional table (aggregator.py:99-106)
    def pe_rows(self, n: int, device) -> torch.Tensor:
        """First n rows of the sinusoidal table, device-resident, grown on demand.  Computed on the host with
        the reference's own expressions (bit-identical to `self.pe[:, :n]`) and uploaded once."""
        if self._pe is None or self._pe.shape[0] < n or self._pe.device != device:
            rows = max(n, 2048, 0 if self._pe is None else 2 * self._pe.shape[0])
            pe = torch.zeros((rows, EMBED))
            position = torch.arange(0, rows).unsqueeze(1)
            div_term = torch.exp(torch.arange(0, EMBED, 2, dtype=torch.float) * -(math.log(10000.0) / EMBED))
            pe[:, 0::2] = torch.sin(position.float() * div_term)
            pe[:, 1::2] = torch.cos(position.float() * div_term)
            self._pe = pe.to(device)
        return lifetime.note(self._pe)            # a captured graph keeps the table it saw when a larger one replaces it

    def _lin_tanh(self, seq: nn.Sequential, x, rows_dev=None):
        return ops.linear_act(x, seq[0].weight, seq[0].bias, "tanh", rows_dev=rows_dev)

    def _head(self, M, geom=None):
        if self.training and geom is not None:
            # the replayed step: torch's generator cannot be rewound after the warm-up passes of a capture, so Dropout(0.25)
            # draws Philox keep bits at the aggregator's device pass counter (which _run_bags has just advanced); the bits are
            # an output of the step (last_head_bits)
            tm = self.aggregator
            self.last_head_bits = ops.dropout_keep_bits(M.shape[0], EMBED, 0.25, tm._drop_seed ^ HEAD_DROP_KEY, 0, M.device,
                                                        offset_dev=tm._drop_ctr)
            M = ops.dropout_bits(M, self.last_head_bits, 1.0 / 0.75)
        elif self.training:
            M = F.dropout(M, 0.25, True)
        p, z = ops.head_sigmoid(M, self.fc[1].weight, self.fc[1].bias)
        self.last_logits = z
        return p

    def _is_transmil(self) -> bool:
        return hasattr(getattr(self, "aggregator", None), "flat_segments")

    def _pool_head(self, x0, layout, segs):
        """Multi-modal bag rows -> prob.  segs[b]: the pieces (first row, length) of bag b in x0 in UPSTREAM'S SEQUENCE ORDER
        (aggregator.py:173,184,192,195), which a TransMIL aggregator needs (square padding repeats the first rows, PPEG is
        positional) and the attention pool does not (None then).  With labels handed to forward() (the training loop's `criterion(prob, y)` of
        train_ddp.py:323-324 moved inside) and an ABMIL aggregator, pool + Dropout(.25) + fc + sigmoid + BCE / CE run as one
        fused node (ops.gated_pool_head_loss) and the loss is left in `self.last_loss`; otherwise op by op."""
        y = self._labels
        C = self.args.num_classes
        if y is not None and hasattr(getattr(self, "aggregator", None), "flat_head_loss") and \
                self.aggregator.can_fuse_head(x0, C) and not self._wants_note_attn():      # note_attn reads last_scores
            ce = C > 2                                     # train_ddp.py:95-98: CrossEntropyLoss on the sigmoid outputs
            scale = self._loss_scale if self._loss_scale is not None else 1.0 / (layout.B * (1 if ce else C))
            loss, p, z = self.aggregator.flat_head_loss(x0, layout, self.fc[1].weight, self.fc[1].bias, y, scale,
                                                        1 if ce else 0, head_train=self.training)
            self.last_logits, self.last_loss = z, loss
            return p
        geom = self._tm_geom
        if self._is_transmil() and geom is not None:
            # the capacity-bucket form (fusion_step.RaggedFusionTransMILStepper): lengths on the device, sides from the key
            want = self._wants_note_attn()                 # scope "all": any other has raised in _forward
            M, attn = self.aggregator.flat_bucket(x0, geom, self._tm_len_dev, need_attn="cls" if want else False)
            self._tm_bag_attn = attn if want else None
        elif self._is_transmil():
            # TransMIL returns (h, attn); element 0 feeds fc.  need_attn="cls" only under note_attn (eval, no grad)
            want = self._wants_note_attn()
            M, attn = self.aggregator.flat_segments(x0, segs, need_attn="cls" if want else False)
            self._tm_bag_attn = None
            if want:
                # [2, 8, L_b] = layers x heads x rows in sequence order -> the rows' order in memory (patches first)
                self._tm_bag_attn = []
                for b, bag in enumerate(segs):
                    a = torch.stack([attn[0][b], attn[1][b]])
                    start, cuts = 0, []
                    for first, n in bag:
                        cuts.append((first, start, n))
                        start += n
                    self._tm_bag_attn.append(torch.cat([a[..., st:st + n] for _, st, n in sorted(cuts)], -1))
        else:
            M = self.aggregator.flat(x0, layout) if hasattr(self, "aggregator") else x0
        self.last_pooled = M                               # [B, 512]: what the head saw (parity checks, like last_logits)
        p = self._head(M, geom)
        if y is not None:
            crit = torch.nn.CrossEntropyLoss() if C > 2 else torch.nn.BCELoss()
            self.last_loss = crit(p, y) * (1.0 if self._loss_scale is None else
                                           self._loss_scale * layout.B * (1 if C > 2 else C))
        return p

    # ------------------------------------------------------------------ CT branches (aggregator.py:155-184)
    def _forward_ct(self, x_list, t, lengths):
        """x_list[0] = the CT encoder's feature map [B, 512, 160, h, w] (precomputed; or tokens [B, D, 512]);
        with 'pathology' also x_list[1] = [B, N, 768].  Returns (prob, x_CT2CI[, x_Pth2CI]) as :202-205."""
        B, P, _ = t.shape
        dev = t.device
        ct = x_list[0]
        if ct.dim() == 5:
            ct_rows, D = ops.ct_map_tokens(ct, _arg(self.args, "model_CT", "resnetMC3_18"))     # sam/transformer.py:86-98
        else:
            D = ct.shape[1]
            ct_rows = ct.reshape(B * D, EMBED).contiguous()
        tflat = t.reshape(B * P, EMBED)
        point_ct = self._lin_tanh(self.fc_CI2CT, tflat)                                       # :160 / :179
        if "pathology" not in self.args.modality:
            q, k = self.TwoWayTransformer_CT.flat(ct_rows, point_ct, self.pe_rows(D, dev), [D] * B, [P] * B,
                                                  keys_tail_rows=B * P)                       # :179
            x0 = ops.append_rows(k, q, tail_reserved=True)                                    # :184
            layout = BagLayout.two_segment([D] * B, [P] * B, dev)
            self._note_ctx = dict(branches=["ct"], B=B, P=P, D=D, cap=None, tail=[], n_len=None, layout=layout)
            segs = [[(B * D + b * P, P), (b * D, D)] for b in range(B)] if self._is_transmil() else None   # :184
            return self._pool_head(x0, layout, segs), q.view(B, P, EMBED)                     # :204-205
        x = x_list[1]
        if x.dim() == 2:
            x = x.unsqueeze(0)
        N = x.shape[1]
        if lengths is None:
            n_len = [N] * B
            flat = x.reshape(B * N, x.shape[2])
        else:
            n_len = [int(v) for v in lengths]
            flat = torch.cat([x[b, :n] for b, n in enumerate(n_len)], 0)
        tw = self.TwoWayTransformer_Both                                                      # :160,168: one module, twice
        q_ct, k_ct = tw.flat(ct_rows, point_ct, self.pe_rows(D, dev), [D] * B, [P] * B)
        xi = self._lin_tanh(self.fc_pathology, flat)                                          # :141
        point_p = self._lin_tanh(self.fc_CI2Pth, tflat)
        extra = B * (2 * P + D)
        q_p, k_p = tw.flat(xi, point_p, self.pe_rows(max(n_len), dev), n_len, [P] * B, keys_tail_rows=extra)
        # multi-modal bag (:173) = [x_CT2CI | x_CI2CT | x_Pth2CI | x_CI2Pth] per patient.  Rows are kept as
        # [all patch tokens | CT-side text tokens | CT tokens | pathology-side text tokens]: the big patch block stays where
        # the last LayerNorm wrote it, the small blocks are appended, the tile map says which rows form a bag.
        x0 = ops.append_rows(k_p, torch.cat([q_ct, k_ct, q_p], 0), tail_reserved=True)
        layout = BagLayout.multi_segment([n_len, [P] * B, [D] * B, [P] * B], dev)
        self._note_ctx = dict(branches=["ct", "pth"], B=B, P=P, D=D, cap=None, tail=[P, D, P], n_len=n_len, layout=layout)
        segs = None
        if self._is_transmil():
            R, off = sum(n_len), _offsets(n_len)
            segs = [[(R + b * P, P), (R + B * P + b * D, D), (R + B * (P + D) + b * P, P), (off[b], n_len[b])]
                    for b in range(B)]                                                    # :173
        return self._pool_head(x0, layout, segs), q_ct.view(B, P, EMBED), q_p.view(B, P, EMBED)   # :198-200,202-203

    # ------------------------------------------------------------------ capacity-bucket form of the pathology branch
    def _forward_bucket(self, x, t, bucket):
        """The pathology + text branch (aggregator.py:186-192,207) on a segments.FusionBucket: x [cap, 768] holds the
        patches of the B bags packed from row 0 (zero rows behind), the true lengths are on the device (bucket.len_dev),
        and every launch below depends on (cap, B) only - so ONE captured graph per bucket serves every bag length the
        authors' loader produces (dataset.py:366-393; fusion_step.RaggedFusionStepper).  One text token per bag."""
        B, P, _ = t.shape
        if x.dim() != 2 or x.shape[0] != bucket.cap or B != bucket.B or P != bucket.P:
            raise ValueError(f"bucket of {bucket.B} bags x {bucket.cap} rows x {bucket.P} token(s): got x {tuple(x.shape)}, "
                             f"text {tuple(t.shape)}")
        bucket.refresh()                                                                   # maps from len_dev, on the device
        xi = self._lin_tanh(self.fc_pathology, x, rows_dev=bucket.rows_dev)                # :149 (tiles behind the true rows: zeros)
        point = self._lin_tanh(self.fc_CI2Pth, t.reshape(B * P, EMBED))                    # :190
        q, k = self.TwoWayTransformer_Pth.flat(xi, point, self.pe_rows(bucket.cap, xi.device), None, None,
                                               keys_tail_rows=B * P, segs=(bucket.s_tt, bucket.s_ti, bucket.s_it))
        x0 = ops.append_rows(k, q, tail_reserved=True)                                     # :192 (no concat copy)
        self._note_ctx = dict(branches=["pth"], B=B, P=P, D=0, cap=bucket.cap, tail=list(bucket.tail), n_len=None,
                              layout=bucket.layout)
        return self._pool_head(x0, bucket.layout, None), q.view(B, P, EMBED)               # :198-200,207

    def _forward_ct_bucket(self, x_list, t, bucket):
        """The CT + pathology branch (aggregator.py:155-173,202-203) on a segments.FusionBucket whose tail is [P, D, P]:
        x_list = [CT feature map [B, 512, 160, h, w] (or tokens [B, D, 512]), patches [cap, 768] packed from row 0].  The CT
        side is static (D tokens per bag) and runs on host-built maps; the pathology side and the 4-segment multi-modal bag
        follow the device-side bag lengths.  This is the authors' own run (run_train.sh:81: `--modality ['CT','pathology']
        --CI_prompt_version single --learnablePrompt 0 --loss_point CT-Pth-Last`, one bag per GPU)."""
        B, P, _ = t.shape
        dev = t.device
        ct, x = x_list[0], x_list[1]
        if ct.dim() == 5:
            ct_rows, D = ops.ct_map_tokens(ct, _arg(self.args, "model_CT", "resnetMC3_18"))     # sam/transformer.py:86-98
        else:
            D = ct.shape[1]
            ct_rows = ct.reshape(B * D, EMBED).contiguous()
        if x.dim() != 2 or x.shape[0] != bucket.cap or B != bucket.B or list(bucket.tail) != [P, D, P]:
            raise ValueError(f"bucket of {bucket.B} bags x {bucket.cap} rows with tail {bucket.tail}: got x {tuple(x.shape)}, "
                             f"text {tuple(t.shape)}, {D} CT tokens per bag")
        bucket.refresh()
        tflat = t.reshape(B * P, EMBED)
        tw = self.TwoWayTransformer_Both                                                      # :160,168: one module, twice
        q_ct, k_ct = tw.flat(ct_rows, self._lin_tanh(self.fc_CI2CT, tflat), self.pe_rows(D, dev), [D] * B, [P] * B)
        xi = self._lin_tanh(self.fc_pathology, x, rows_dev=bucket.rows_dev)                   # :141
        q_p, k_p = tw.flat(xi, self._lin_tanh(self.fc_CI2Pth, tflat), self.pe_rows(bucket.cap, dev), None, None,
                           keys_tail_rows=bucket.tail_rows, segs=(bucket.s_tt, bucket.s_ti, bucket.s_it))
        x0 = ops.append_rows(k_p, torch.cat([q_ct, k_ct, q_p], 0), tail_reserved=True)        # :173 (no concat of the patches)
        self._note_ctx = dict(branches=["ct", "pth"], B=B, P=P, D=D, cap=bucket.cap, tail=list(bucket.tail), n_len=None,
                              layout=bucket.layout)
        return self._pool_head(x0, bucket.layout, None), q_ct.view(B, P, EMBED), q_p.view(B, P, EMBED)

    def _graph_eval_forward(self, x_list, x_CI):
        """One bag through the replayed forward, or None when the call is not one the stepper takes (then the eager forward
        runs as always).  Returns the shipped module's tuple; the tensors are the graph's static outputs, valid until the next
        forward of that key."""
        modality = list(self.args.modality)
        with_ct = modality == ["CT", "pathology"]
        if not self._is_transmil() or (modality != ["pathology"] and not with_ct) or len(x_list) != (2 if with_ct else 1):
            return None
        x = x_list[-1]
        if x.dim() == 2:
            x = x.unsqueeze(0)
        ct = x_list[0] if with_ct else None
        if (x.dim() != 3 or x.shape[0] != 1 or not x.is_cuda or x_CI is None or x_CI.dim() != 3 or x_CI.shape[0] != 1
                or x_CI.shape[1] > 12 or (ct is not None and ct.shape[0] != 1)):
            return None
        st = self._eval_stepper
        if st is None:
            # tower_in_graph=True switches the text tower to its fixed-shape form (clinic_extractor.model.static_rows) for
            # good, as RaggedFusionStepper / RaggedFusionInference do: a later call that falls back to the eager forward
            # below (a bag the bucket cannot take) runs the tower in that form too - the same values, padded launches
            from ..fusion_step import RaggedFusionTransMILStepper
            st = self._eval_stepper = RaggedFusionTransMILStepper(
                self, None, B=1, P=int(x_CI.shape[1]), in_dim=int(x.shape[2]), ctx_len=int(x_CI.shape[2]), backward=False,
                ct_shape=tuple(ct.shape[1:]) if ct is not None else None, tower_in_graph=True)
        n = int(x.shape[1])
        slot = st.slot(n)
        if (not slot.bucket.fits([n]) or x.shape[2] != st.in_dim or tuple(x_CI.shape[1:]) != tuple(slot.ids.shape[1:])
                or (ct is not None and tuple(ct.shape) != tuple(slot.ct.shape))):
            return None
        slot.x[:n].copy_(x[0], non_blocking=True)
        if ct is not None:
            slot.ct.copy_(ct, non_blocking=True)
        slot.ids.copy_(x_CI, non_blocking=True)             # the text tower is part of the replayed forward
        _, prob = st.step(slot, [n])
        self.last_pooled, self.last_logits = st.last["h"], st.last["logits"]
        return (prob, *st.last["tokens"])

    # ------------------------------------------------------------------ forward (aggregator.py:134-209)
    def forward(self, x_list: List[torch.Tensor], x_CI: torch.Tensor, lengths: Optional[List[int]] = None,
                text_features: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                loss_scale: Optional[float] = None, bucket=None):
        """The shipped module's return tuples (aggregator.py:202-209), which test_ddp.py:220 consumes.  With
        `args.train_contract` set, the tuple the reference's TRAINING loop unpacks instead (train_ddp.py:300,305-316; no
        shipped module provides it): CT + pathology -> ([out, out, out], [x_CT2CI, x_Pth2CI], None) - one head, so the three
        outputs of loss_point 'CT-Pth-Last' are the same tensor -, a single modality -> (out, token, None), text only ->
        (out, None)."""
        out = self._forward(x_list, x_CI, lengths, text_features, labels, loss_scale, bucket)
        if not _arg(self.args, "train_contract", 0):
            return out
        if not isinstance(out, tuple):
            return out, None
        if len(out) == 3:
            return [out[0], out[0], out[0]], [out[1], out[2]], None
        return out[0], out[1], None

    def _forward_branch(self, x_list, t, lengths, bucket):
        """The CT branches and the capacity-bucket forms."""
        modality = self.args.modality
        if "CT" in modality and "pathology" in modality and bucket is not None:
            return self._forward_ct_bucket(x_list, t, bucket)
        if "CT" in modality:
            return self._forward_ct(x_list, t, lengths)
        return self._forward_bucket(x_list[0], t, bucket)

    def _forward(self, x_list: List[torch.Tensor], x_CI: torch.Tensor, lengths: Optional[List[int]] = None,
                 text_features: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
                 loss_scale: Optional[float] = None, bucket=None):
        """x_list = [x_pathology [B, N, 768]] (or [] for CI only); x_CI int64 [B, P, ctx] token ids.
        `lengths` (optional) gives the true patch count of each zero-padded bag (dataset.py:386-391 pads to a
        fixed length when batch > 1); padded rows are then dropped instead of being attended to."""
        # labels [B, C] float one-hot (optional, an extension of the reference signature): the criterion of
        # train_ddp.py:323-324 evaluated inside, result in `self.last_loss` (mean loss unless loss_scale is given);
        # the return tuple is unchanged
        if (self.graph_eval and bucket is None and not self.training and not torch.is_grad_enabled() and lengths is None
                and text_features is None and labels is None and (not self._wants_note_attn() or self._note_all())):
            out = self._graph_eval_forward(x_list, x_CI)
            if out is not None:
                return out
        self._labels, self._loss_scale, self.last_loss, self.last_pooled = labels, loss_scale, None, None
        self.last_head_bits = None
        modality = self.args.modality
        self._tm_geom = getattr(bucket, "tm_geom", None) if self._is_transmil() else None
        self._tm_len_dev = bucket.len_dev if self._tm_geom is not None else None
        if bucket is not None and self._is_transmil() and self._tm_geom is None:
            raise NotImplementedError("bucket=: the capacity-bucket forward is built for the ABMIL aggregator; TransMIL's "
                                      "shapes follow the grid side ceil(sqrt(rows)) of each bag (eager path, or a bucket that "
                                      "carries the TransMIL geometry: fusion_step.RaggedFusionTransMILStepper)")
        if self._tm_geom is not None and (self._tm_geom.cap != bucket.cap or self._tm_geom.B != bucket.B
                                          or list(self._tm_geom.tail) != list(bucket.tail)):
            raise ValueError(f"bucket of {bucket.B} bags x {bucket.cap} rows, tail {bucket.tail}: its TransMIL geometry is for "
                             f"{self._tm_geom.B} bags x {self._tm_geom.cap} rows, tail {list(self._tm_geom.tail)}")
        want = self._wants_note_attn()
        if want:
            self.last_note_attn = self.last_note_attn_ct = self.last_bag_attn = None
            self._note_meta = self._note_tensors = None
            if self.note_attn is not True and not self._note_all():
                raise ValueError(f"note_attn must be False, True or 'all', got {self.note_attn!r}")
            if self._note_all() and _arg(self.args, "alignment_base", "CI") == "CT":
                raise NotImplementedError("note_attn: with alignment_base='CT' the token->image sites run on the general "
                                          "attention_pool route, which keeps no weights")
            if not self._note_all() and ("CT" in modality or bucket is not None):
                raise NotImplementedError("note_attn is built for modality ['pathology'] (or ['CI']) on host-side bag lengths: "
                                          "the CT branches and the capacity-bucket forward keep no attention weights")
        # text_features [B, P, 512] (optional): embeddings of the frozen text tower computed earlier by
        # `self.clinic_extractor(x_CI)`; lets a captured hipGraph replay the trainable part only
        t = text_features if text_features is not None else self.clinic_extractor(x_CI)   # :151  [B, P, 512]
        B, P, _ = t.shape
        if want and ("CT" in modality or ("pathology" in modality and bucket is not None)):
            # scope "all": the branch under the site tap, then the device part; the slicing by host lengths follows at once
            # on host-side lengths and is the caller's with a bucket (note_attn_finish)
            with ops.note_sites() as sites:
                out = self._forward_branch(x_list, t, lengths, bucket)
            self._note_device(sites)
            if bucket is None:
                self.note_attn_finish()
            return out
        if "CT" in modality or ("pathology" in modality and bucket is not None):
            return self._forward_branch(x_list, t, lengths, bucket)
        if "pathology" in modality:
            x = x_list[0]
            if x.dim() == 2:
                x = x.unsqueeze(0)
            N = x.shape[1]
            if lengths is None:
                n_len = [N] * B
                flat = x.reshape(B * N, x.shape[2])
            else:
                n_len = [int(v) for v in lengths]
                flat = torch.cat([x[b, :n] for b, n in enumerate(n_len)], 0)
            xi = self._lin_tanh(self.fc_pathology, flat)                                  # :149
            point = self._lin_tanh(self.fc_CI2Pth, t.reshape(B * P, EMBED))               # :190
            if want:
                with ops.note_sites() as sites:
                    q, k = self.TwoWayTransformer_Pth.flat(xi, point, self.pe_rows(max(n_len), xi.device), n_len, [P] * B,
                                                           keys_tail_rows=B * P)
            else:
                q, k = self.TwoWayTransformer_Pth.flat(xi, point, self.pe_rows(max(n_len), xi.device), n_len, [P] * B,
                                                       keys_tail_rows=B * P)
            # multi-modal bag per patient = its text tokens + its patch tokens (:192).  Rows are kept as
            # [all patches | all tokens] (the patch tokens stay where the last LayerNorm wrote them, only the few
            # token rows are appended) and the tile map tells the pool kernels which rows belong to which bag;
            # attention pooling does not depend on the order of a bag's rows.
            x0 = ops.append_rows(k, q, tail_reserved=True)     # k comes from the last block's norm4 with keys_tail_rows
            layout = BagLayout.two_segment(n_len, [P] * B, x0.device)
            segs = None
            if self._is_transmil():
                R, off = sum(n_len), _offsets(n_len)
                segs = [[(R + b * P, P), (off[b], n_len[b])] for b in range(B)]           # :192 [x_Pth2CI | x_CI2Pth]
            prob = self._pool_head(x0, layout, segs)
            if want:
                self._note_attention(sites, n_len, P, layout)
            return prob, q.view(B, P, EMBED)                                              # :198-200,207
        if "CI" in modality:
            x0 = self._lin_tanh(self.fc_CI, t.reshape(B * P, EMBED))                      # :195
            layout = BagLayout.uniform(B, P, x0.device)
            prob = self._pool_head(x0, layout, [[(b * P, P)] for b in range(B)] if self._is_transmil() else None)   # :198-200,209
            if want:
                self._bag_attention(layout)
            return prob
        raise NotImplementedError(f"modality {modality}")
