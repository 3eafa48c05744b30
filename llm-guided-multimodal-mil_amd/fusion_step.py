"""The authors' training regime for the FUSION model: one ragged bag per GPU, its length changing every step
(reference run_train.sh:81 `--batch_size` = number of GPUs; dataset.py:366-393 drops a random 10-20 % of a bag's
patches every epoch and bags hold 2 000 .. 15 592 patches).

`graph_step.GraphedStep` keys a captured step by the exact bag lengths, so on such a cohort nothing ever replays and the
paper's model runs eagerly - host-bound at ~190 launches per step.  `RaggedFusionStepper` does for `aggregator(args)` what
`trainer.RaggedImageOnlyStepper` does for the image-only step: every batch goes into a CAPACITY bucket (bags.bucket_rows:
2 048, 3 072, 4 096, ... patch rows), the bag lengths go to the device (segments.FusionBucket), every segment map the
step reads is rebuilt there by its first launch, and the bucket's step - forward, loss, backward AND the Adam update, whose
step number and learning rate live on the device too - is ONE hipGraph captured the second time the bucket is seen.  Padding
rows carry zero softmax weight in all four pooling sites and receive exactly zero gradient.

    stepper = RaggedFusionStepper(model, opt)          # opt = optim.FlatAdam(..., counted=True)
    slot = stepper.slot(n)                             # static inputs of the bucket: slot.x[:n], slot.text, slot.y
    loss, prob = stepper.step(slot, [n])

P text tokens per bag: 1 (`CI_prompt_version='single'`, dataset.py:479-502: the absorbed one-token kernels), or up to 12
(`'devided'`, or upstream's default learnable-prompt branch with its len(clinical_features) + 1 prompts: the multi-token
grouped products, whose outputs are cleared for the padding rows).  A frozen text tower runs outside the graph (its launch
geometry follows the notes' lengths) and hands `slot.text` its embeddings; learnable prompts run the tower inside the step
on `slot.ids` in its fixed-shape form."""
from typing import Dict, Sequence

import torch

from .bags import bucket_rows
from .graph_step import GraphedStep
from .segments import FusionBucket


class RaggedFusionStepper:
    class Slot:
        def __init__(self, cap: int, B: int, C: int, in_dim: int, device, P: int = 1, ctx_len: int = 77, ct_shape=None,
                     ct_tokens: int = 0):
            self.cap, self.B = cap, B
            # CT + pathology (aggregator.py:155-173): the CT encoder's feature map is an input of the step as well
            self.ct = torch.zeros((B,) + tuple(ct_shape), device=device, dtype=torch.float32) if ct_shape else None
            self.x = torch.zeros((cap, in_dim), device=device, dtype=torch.float32)    # rows beyond the bags: padding
            self.text = torch.zeros((B, P, 512), device=device, dtype=torch.float32)   # frozen-tower embedding per prompt
            self.ids = torch.zeros((B, P, ctx_len), device=device, dtype=torch.int64)  # learnable prompts: the token ids
            self.y = torch.zeros((B, C), device=device, dtype=torch.float32)
            self.bucket = FusionBucket(cap, B, device, P, tail=[P, ct_tokens, P] if ct_shape else None)

    def __init__(self, model, opt, B: int = 1, use_graph: bool = True, max_graphs: int = 16, in_dim: int = 768,
                 opt_in_graph: bool = True, P: int = 1, learnable: bool = False, ctx_len: int = 77, ct_shape=None,
                 loss_mult: float = 1.0, cossim: bool = False, tower_in_graph: bool = False):
        """opt_in_graph=False keeps the optimizer (and, at world size > 1, its gradient all-reduce) outside the captured
        graph, as graph_step.GraphedStep does.  P: text tokens per bag (1 = one note; 10 = `CI_prompt_version='devided'` or
        the learnable-prompt branch, whose P = len(clinical_features) + 1).  learnable=True: upstream's default
        `--learnablePrompt 1` - the text tower runs INSIDE the step on `slot.ids` in its fixed-shape form
        (`clinic_extractor.model.static_rows = True`, set here) and its context vectors are trained through it."""
        if use_graph and opt_in_graph and not getattr(opt, "counted", False):
            raise ValueError("RaggedFusionStepper: an optimizer inside the graph needs optim.FlatAdam(counted=True) "
                             "(step number and learning rate on the device)")
        self.model, self.opt, self.B, self.use_graph, self.in_dim = model, opt, int(B), bool(use_graph), int(in_dim)
        self.opt_in_graph = bool(opt_in_graph)
        self.P, self.learnable, self.ctx_len = int(P), bool(learnable), int(ctx_len)
        # ct_shape (E, D, h, w): modality ['CT', 'pathology'] - slot.ct holds the CT feature map, the multi-modal bag has
        # four segments.  loss_mult: 3 for `--loss_point CT-Pth-Last` (train_ddp.py:319-322: the criterion on three outputs,
        # one head here).  cossim: add CosineEmbeddingLoss(x_CT2CI, x_Pth2CI, 1) ('textCosSim', train_ddp.py:325-329).
        self.ct_shape = tuple(ct_shape) if ct_shape else None
        self.ct_tokens = 0
        if self.ct_shape:
            E_, D_, h_, w_ = self.ct_shape
            self.ct_tokens = D_ * h_ * w_ if getattr(model.args, "model_CT", "resnetMC3_18") == "medicalNet" else D_
        self.loss_mult, self.cossim = float(loss_mult), bool(cossim)
        # tower_in_graph (frozen prompts): the reference runs encode_text on every step's notes (model/dim1/CLIP.py:71-75).
        # Outside the graph that is ~100 eager launches per note (3-4 ms of host time against a 1 ms step); inside, in the
        # tower's fixed-shape form, it is part of the replay: fill slot.ids instead of calling encode_notes().
        self.tower_inside = self.learnable or bool(tower_in_graph)
        if self.tower_inside and use_graph:
            model.clinic_extractor.model.static_rows = True      # the tower is inside the graph: no token-dependent host work
        self.device = next(model.parameters()).device
        self.C = int(model.args.num_classes)
        self.slots: Dict[int, "RaggedFusionStepper.Slot"] = {}
        self.gs = GraphedStep(list(opt.params), max_graphs=max_graphs)
        self.eager_only = 0

    @property
    def replays(self):
        return self.gs.replays

    @property
    def eager_steps(self):
        return self.gs.eager_steps + self.eager_only

    def slot(self, total_rows: int) -> "RaggedFusionStepper.Slot":
        cap = bucket_rows(total_rows)
        s = self.slots.get(cap)
        if s is None:
            s = self.slots[cap] = self.Slot(cap, self.B, self.C, self.in_dim, self.device, self.P, self.ctx_len,
                                           self.ct_shape, self.ct_tokens)
        return s

    def encode_notes(self, slot, ids):
        """Frozen text tower on this step's notes (token ids [B, 1, ctx]) -> slot.text; outside the graph."""
        with torch.no_grad():
            slot.text.copy_(self.model.clinic_extractor(ids))
        return slot.text

    def _body(self, slot):
        m = self.model
        xs = [slot.x] if slot.ct is None else [slot.ct, slot.x]
        scale = self.loss_mult / (self.B * (1 if self.C > 2 else self.C)) if self.loss_mult != 1.0 else None
        kw = dict(labels=slot.y, bucket=slot.bucket, loss_scale=scale)
        out = m(xs, slot.ids, **kw) if self.tower_inside else m(xs, None, text_features=slot.text, **kw)
        if isinstance(out[0], list):                   # args.train_contract: ([x, x, x], [CT2CI, Pth2CI], None)
            prob, toks = out[0][0], out[1]
        else:
            prob, toks = out[0], list(out[1:])
        toks = [t_ for t_ in toks if t_ is not None]
        loss = m.last_loss
        if self.cossim and len(toks) == 2:
            from . import ops
            loss = loss + ops.cosine_embedding_loss(toks[0].squeeze(1), toks[1].squeeze(1))
        return loss, prob, m.last_logits

    def step(self, slot, lengths: Sequence[int], on_device: bool = False):
        """One training step on the bags packed in slot.x (bag b at rows [sum(lengths[:b]), +lengths[b])).  Returns
        (loss, prob, logits) - static tensors of the bucket's graph once it replays.  on_device: the lengths already sit in
        slot.bucket.len_dev (the cohort's feed launch wrote them)."""
        slot.bucket.set_lengths(lengths, on_device=on_device)
        body = lambda: self._body(slot)      # noqa: E731
        if not self.use_graph:
            self.eager_only += 1
            self.gs._drop_grads()
            out = body()
            from . import ops
            ops.backward(out[0])
            self.opt.step()
            return tuple(o.detach() for o in out)
        key = ("fusion-bucket", slot.cap, self.model.training)
        if not self.opt_in_graph:
            out = self.gs.run(key, (), body)
            self.opt.step()
            return out
        self.opt.sync_lr()                   # a changed learning rate reaches its device word before the replay reads it
        return self.gs.run(key, (), body, after_backward=self.opt.step)


def _exports_note_attn(model, backward: bool) -> bool:
    """The evaluation forward of a model whose note_attn scope is "all": the stepper's body also runs the export's launches
    (aggregator._note_device) and returns their capacity-shaped results, so they are static outputs of the key's graph; step()
    slices them by the call's host lengths afterwards (aggregator.note_attn_finish).  Never with backward."""
    return (not backward) and (not model.training) and getattr(model, "note_attn", False) == "all"


class RaggedFusionTransMILStepper:
    """The same regime for the fusion model with the TransMIL aggregator (`--aggregator TransMIL --fusion_transmil 1`, the
    authors' own run), training step or evaluation forward.  The branch in front of the aggregator follows the capacity bucket
    as above; TransMIL's shapes follow the grid side of each multi-modal bag, s_b = ceil(sqrt(N_b + tail)), tail = the static
    rows behind the patches (P text tokens; P + D + P with CT).  So a step is keyed by (cap, sides): the slot of a capacity
    holds the static inputs and the FusionBucket, a model.dim1.TransMIL.BucketGeometry per key holds the gather index that the
    step's launch mil_tm_seq_index_bucket writes from the lengths on the device.  One bag of 2 000 .. 15 592 patches touches 86
    keys with tail 162 and 87 with tail 1; all graphs share one memory pool.

        stepper = RaggedFusionTransMILStepper(model, opt, ct_shape=...)   # opt = optim.FlatAdam(counted=True) at world size 1
        slot = stepper.slot(n)                             # static inputs: slot.x[:n], slot.ct, slot.text / slot.ids, slot.y
        loss, prob = stepper.step(slot, [n])               # or cohort.feed(..., slot.bucket.len_dev, ...) + on_device=True
        value = stepper.read_loss(loss)                    # the host sync; raises if a length on the device left its key

    The first visit of a key runs eagerly through the same device-geometry body, the second captures, later ones replay.
    Everything random is Philox on the aggregator's fixed seed and device pass counter - TransMIL's two Dropout(0.1) and, on
    this path, the head's Dropout(0.25) -, and the keep bits of a pass are outputs of the step (stepper.last["bits"]).
    backward=False / opt=None: the evaluation forward (test_ddp.py).

    The TRAINING step of this stepper runs on TransMIL's fixed-order sums (`aggregator.deterministic = True`, set here when
    backward is on; +0 - 0.8 % of the TransMIL stage).  On the atomic sums two runs of this step from one seed - with
    or without graphs - were measured to part by up to 8.3e-3 in the parameter update after 8 steps (docs/lab_notes.md), outside
    the module's 2e-3 bar, and the cause was not found; on the fixed-order sums every run gives the same bits.  The forward
    holds no atomic sum, so the evaluation stepper leaves the switch alone."""

    def __init__(self, model, opt=None, B: int = 1, use_graph: bool = True, max_graphs=None, in_dim: int = 768,
                 opt_in_graph=None, P: int = 1, ctx_len: int = 77, ct_shape=None, loss_mult: float = 1.0, cossim: bool = False,
                 tower_in_graph: bool = False, drop_seed=None, backward=None):
        from .model.dim1.TransMIL import bucket_side
        from .transmil_step import DEFAULT_MAX_GRAPHS
        agg = getattr(model, "aggregator", None)
        if type(agg).__name__ != "TransMIL":
            raise ValueError("RaggedFusionTransMILStepper: the model's aggregator is not TransMIL (--fusion_transmil 1)")
        if list(model.args.modality) not in (["pathology"], ["CT", "pathology"]):
            raise NotImplementedError("RaggedFusionTransMILStepper: built for modality ['pathology'] and ['CT', 'pathology']")
        if ("CT" in model.args.modality) != bool(ct_shape):
            raise ValueError("RaggedFusionTransMILStepper: ct_shape goes with modality ['CT', 'pathology']")
        if getattr(model.args, "learnablePrompt", 0):
            raise NotImplementedError("RaggedFusionTransMILStepper: learnable prompts (their SGD inside the graph) are not built")
        self.model, self.opt, self.B, self.use_graph, self.in_dim = model, opt, int(B), bool(use_graph), int(in_dim)
        self.backward = (opt is not None) if backward is None else bool(backward)
        if opt is not None and not self.backward:
            raise ValueError("RaggedFusionTransMILStepper: an optimizer needs the backward")
        world = getattr(opt, "world", 1) if opt is not None else 1
        self.opt_in_graph = (world == 1) if opt_in_graph is None else bool(opt_in_graph)
        if opt is not None and use_graph and self.opt_in_graph and not getattr(opt, "counted", False):
            raise ValueError("RaggedFusionTransMILStepper: an optimizer inside the graph needs optim.FlatAdam(counted=True) "
                             "(step number and learning rate on the device)")
        self.P, self.ctx_len = int(P), int(ctx_len)
        self.ct_shape = tuple(ct_shape) if ct_shape else None
        self.ct_tokens = 0
        if self.ct_shape:
            if len(self.ct_shape) == 2:                     # the CT side given as tokens [B, D, 512]
                self.ct_tokens = self.ct_shape[0]
            else:
                E_, D_, h_, w_ = self.ct_shape
                self.ct_tokens = D_ * h_ * w_ if getattr(model.args, "model_CT", "resnetMC3_18") == "medicalNet" else D_
        self.tail = [self.P, self.ct_tokens, self.P] if self.ct_shape else [self.P]
        self.ntok = 2 if self.ct_shape else 1               # x_CT2CI, x_Pth2CI / x_Pth2CI: returned beside prob
        self.loss_mult, self.cossim = float(loss_mult), bool(cossim)
        self.tower_inside = bool(tower_in_graph)
        if self.tower_inside and use_graph:
            model.clinic_extractor.model.static_rows = True      # the tower is inside the graph: no token-dependent host work
        self.device = next(model.parameters()).device
        self.C = int(model.args.num_classes)
        if drop_seed is not None:
            agg._drop_seed = int(drop_seed)
        agg._drop_state(self.device)                        # seed and pass counter exist before any capture
        if self.backward:
            agg.deterministic = True                        # see the class docstring: no atomic sums in this training step
        self.flag = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._pad_cache: dict = {}
        self._side = bucket_side
        self.slots: Dict[int, RaggedFusionStepper.Slot] = {}
        self.geoms: Dict[tuple, object] = {}
        params = list(opt.params) if opt is not None else [p for p in model.parameters() if p.requires_grad]
        cap = DEFAULT_MAX_GRAPHS if max_graphs is None else int(max_graphs)
        self.gs = GraphedStep(params, max_graphs=cap if self.use_graph else 0, share_pool=True, backward=self.backward)
        self.last = None
        self._note_metas: dict = {}                         # per key: how the export's tensors of that graph are laid out

    @property
    def replays(self):
        return self.gs.replays

    @property
    def eager_steps(self):
        return self.gs.eager_steps

    @property
    def n_graphs(self):
        return len(self.gs._graphs)

    def slot(self, total_rows: int) -> "RaggedFusionStepper.Slot":
        cap = bucket_rows(total_rows)
        s = self.slots.get(cap)
        if s is None:
            s = self.slots[cap] = RaggedFusionStepper.Slot(cap, self.B, self.C, self.in_dim, self.device, self.P, self.ctx_len,
                                                           self.ct_shape, self.ct_tokens)
        return s

    def sides(self, lengths: Sequence[int]) -> tuple:
        """The grid sides of the multi-modal bags: patches + the static rows behind them."""
        tail = sum(self.tail)
        return tuple(self._side(int(n) + tail) for n in lengths)

    def key(self, cap: int, lengths: Sequence[int]) -> tuple:
        agg = self.model.aggregator
        from . import ops
        note = _exports_note_attn(self.model, self.backward)
        # the route the aggregator's flat_bucket resolves for this step; a forward that exports the attention (scope "all")
        # runs the cls route and more launches behind it: it never shares a key with one that does not
        route = ops.tm_route(agg, len(lengths), "cls" if note else False)
        # this key has carried "cls" wherever it carries "packed" and packed_cls is on, although the graph step never asks for
        # attention; that is not what the route says, so it is added here and existing keys stay what they were
        cls = ("cls",) if route.bags == "packed" and ops.tm_packed_cls(agg.packed_cls) else ()
        return (("fusion-transmil", int(cap), self.sides(lengths), bool(self.model.training), bool(agg.training), self.backward)
                + route.key() + cls + (("note_attn", "all") if note else ()))

    def _note_scope(self) -> bool:
        return _exports_note_attn(self.model, self.backward)

    def encode_notes(self, slot, ids):
        """Frozen text tower on this step's notes (token ids [B, P, ctx]) -> slot.text; outside the graph."""
        with torch.no_grad():
            slot.text.copy_(self.model.clinic_extractor(ids))
        return slot.text

    def _body(self, slot, geom):
        m = self.model
        slot.bucket.tm_geom = geom
        xs = [slot.x] if slot.ct is None else [slot.ct, slot.x]
        scale = self.loss_mult / (self.B * (1 if self.C > 2 else self.C)) if self.loss_mult != 1.0 else None
        kw = dict(labels=slot.y, bucket=slot.bucket, loss_scale=scale)
        out = m(xs, slot.ids, **kw) if self.tower_inside else m(xs, None, text_features=slot.text, **kw)
        if isinstance(out[0], list):                       # args.train_contract: ([x, x, x], [CT2CI, Pth2CI], None)
            prob, toks = out[0][0], out[1]
        else:
            prob, toks = out[0], list(out[1:])
        toks = [t_ for t_ in toks if t_ is not None]
        loss = m.last_loss
        if self.cossim and len(toks) == 2:
            from . import ops
            loss = loss + ops.cosine_embedding_loss(toks[0].squeeze(1), toks[1].squeeze(1))
        res = [loss, prob, m.last_pooled, m.last_logits] + toks      # one token tensor per branch: self.ntok
        if m.aggregator.training:                          # the keep bits of this pass: static tensors once the graph replays
            for pair in m.aggregator.last_bits:
                res += list(pair)
        if m.last_head_bits is not None:
            res.append(m.last_head_bits)
        if m._note_meta is not None:                       # scope "all": the export's tensors, last
            res += list(m._note_tensors)
        return tuple(res)

    def step(self, slot, lengths: Sequence[int], on_device: bool = False):
        """One step (or, with backward=False, one forward) on the bags packed in slot.x (bag b at rows [sum(lengths[:b]),
        +lengths[b])).  on_device: the lengths already sit in slot.bucket.len_dev.  Returns (loss, prob); self.last holds h,
        logits, tokens (the text-aligned tokens the module returns beside prob) and, in train mode, bits = TransMIL's keep bits per bag and layer, then the head's - static tensors of the
        key's graph once it replays."""
        lengths = [int(n) for n in lengths]
        slot.bucket.set_lengths(lengths, on_device=on_device)
        key = self.key(slot.cap, lengths)
        geom = self.geoms.get(key[1:3])
        if geom is None:
            from .model.dim1.TransMIL import BucketGeometry
            geom = self.geoms[key[1:3]] = BucketGeometry(slot.cap, self.tail, key[2], self.device, self._pad_cache, self.flag)
        m = self.model
        body = lambda: self._body(slot, geom)      # noqa: E731
        m._note_meta = None                        # set by a pass of the body that exports; a replay runs none
        ctr = m.aggregator._drop_ctr
        from . import ops
        # the warm-up passes in front of a capture draw masks too: the pass counter goes back, so the stream of a replayed
        # run stays the stream of an eager one
        # (forced masks, aggregator.force_bits, do not move the counter: nothing to rewind then)
        moves = m.aggregator.training and m.aggregator.force_bits is None
        rewind = (lambda: ops.counter_add(ctr, -self.gs.warmup)) if moves else None      # noqa: E731
        in_graph = self.opt is not None and self.opt_in_graph
        if in_graph:
            self.opt.sync_lr()                     # a changed learning rate reaches its device word before the replay reads it
        out = self.gs.run(key, (), body, after_backward=self.opt.step if in_graph else None, before_capture=rewind)
        if self.opt is not None and not in_graph:
            self.opt.step()
        nt = self.ntok
        self.last = dict(h=out[2], logits=out[3], tokens=list(out[4:4 + nt]),
                         bits=list(out[4 + nt:]) if m.aggregator.training else None)
        if self._note_scope():
            if m._note_meta is not None:
                self._note_metas[key] = m._note_meta
            meta = m._note_meta = self._note_metas[key]
            m.note_attn_finish(lengths, out[len(out) - meta["count"]:])
        return out[0], out[1]

    def pool_bytes(self) -> int:
        """Device memory the shared pool of this stepper's graphs holds (the allocator's segments of that pool).  Walks the
        allocator's snapshot: for tools, never called by step()."""
        pid = tuple(self.gs.pool)
        return sum(int(seg["total_size"]) for seg in torch.cuda.memory_snapshot() if tuple(seg["segment_pool_id"]) == pid)

    def read_loss(self, loss: torch.Tensor) -> float:
        """The step's loss on the host (a sync), after checking the device flag mil_tm_seq_index_bucket raises for a bag whose
        rows on the device do not fit the grid side of its key, or lengths beyond the capacity - such a step ran on a
        clamped index."""
        v = float(loss.detach())
        if int(self.flag.item()):
            self.flag.zero_()
            raise RuntimeError("RaggedFusionTransMILStepper: a bag length on the device lay outside its key's grid side "
                               "(or the lengths exceeded the bucket's capacity)")
        return v


class RaggedFusionInference:
    """Evaluation of the fusion model (reference test_ddp.py:187-253: eval mode, one bag per forward, per-sample inference
    time) on capacity buckets: the forward of a bucket is captured into a hipGraph the second time the bucket is seen and
    replayed afterwards - a forward is ~70 short launches, eagerly the host sets the pace.  Same slots and device-side
    segments as RaggedFusionStepper; no gradients, no optimizer.

        inf = RaggedFusionInference(model, P=1)              # model.eval()
        slot = inf.slot(n); slot.x[:n].copy_(bag); inf.encode_notes(slot, ids)
        prob = inf.forward(slot, [n])                        # [B, C], valid until the next replay of that bucket"""

    def __init__(self, model, B: int = 1, P: int = 1, in_dim: int = 768, ctx_len: int = 77, ct_shape=None, use_graph: bool = True,
                 tower_in_graph: bool = True):
        self.model, self.B, self.P, self.in_dim, self.ctx_len = model, int(B), int(P), int(in_dim), int(ctx_len)
        # the text tower inside the replayed forward (fixed-shape form, fill slot.ids) or outside (encode_notes -> slot.text)
        self.tower_inside = bool(tower_in_graph) and bool(use_graph)
        if self.tower_inside:
            model.clinic_extractor.model.static_rows = True
        self.device = next(model.parameters()).device
        self.C = int(model.args.num_classes)
        self.ct_shape = tuple(ct_shape) if ct_shape else None
        self.ct_tokens = 0
        if self.ct_shape:
            E_, D_, h_, w_ = self.ct_shape
            self.ct_tokens = D_ * h_ * w_ if getattr(model.args, "model_CT", "resnetMC3_18") == "medicalNet" else D_
        self.use_graph = bool(use_graph)
        self.slots: Dict[int, RaggedFusionStepper.Slot] = {}
        self._graphs: Dict[int, tuple] = {}
        self._seen: Dict[int, int] = {}
        self.replays = self.eager = 0
        self.stream = torch.cuda.Stream()

    def slot(self, total_rows: int):
        cap = bucket_rows(total_rows)
        s = self.slots.get(cap)
        if s is None:
            s = self.slots[cap] = RaggedFusionStepper.Slot(cap, self.B, self.C, self.in_dim, self.device, self.P, self.ctx_len,
                                                           self.ct_shape, self.ct_tokens)
        return s

    def encode_notes(self, slot, ids):
        with torch.no_grad():
            slot.text.copy_(self.model.clinic_extractor(ids))
        return slot.text

    def _body(self, slot):
        xs = [slot.x] if slot.ct is None else [slot.ct, slot.x]
        if self.tower_inside:
            out = self.model(xs, slot.ids, bucket=slot.bucket)
        else:
            out = self.model(xs, None, text_features=slot.text, bucket=slot.bucket)
        prob = out[0][0] if isinstance(out[0], list) else out[0]
        m = self.model
        if m._note_meta is None:
            return prob
        return (prob, m._note_meta, *m._note_tensors)      # scope "all": the export's tensors are outputs of the forward

    def _finish(self, out, lengths):
        """prob of a pass of the body; with the export (model.note_attn = "all") the per-bag slicing by this call's lengths."""
        if not isinstance(out, tuple):
            return out
        self.model._note_meta = out[1]
        self.model.note_attn_finish(lengths, out[2:])
        return out[0]

    @torch.no_grad()
    def forward(self, slot, lengths: Sequence[int], on_device: bool = False):
        slot.bucket.set_lengths(lengths, on_device=on_device)
        m = self.model
        m._note_meta = None
        # a forward that exports the attention runs more launches: it has graphs of its own
        key = (slot.cap, "note_attn", "all") if (m.note_attn == "all" and not m.training) else slot.cap
        ent = self._graphs.get(key)
        if ent is None:
            n = self._seen[key] = self._seen.get(key, 0) + 1
            if not self.use_graph or n < 2:
                self.eager += 1
                return self._finish(self._body(slot), lengths)
            from . import lifetime
            cur = torch.cuda.current_stream()
            with lifetime.recording() as keep:
                self.stream.wait_stream(cur)
                with torch.cuda.stream(self.stream):
                    self._body(slot)                                   # caches (positional rows, segment maps) fill here
                cur.wait_stream(self.stream)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.stream):
                    prob = self._body(slot)
            ent = self._graphs[key] = (g, prob, keep)
        ent[0].replay()
        self.replays += 1
        return self._finish(ent[1], lengths)
