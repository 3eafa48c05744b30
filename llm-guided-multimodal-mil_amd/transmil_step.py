"""The authors' training regime for the image-only TransMIL model (`--model_pathology TransMIL`): one ragged bag per GPU, its
length changing every step, replayed from hipGraphs.

Everything that shapes TransMIL's launches - the s x s grid of PPEG, seq = s^2 + 1, n_pad, the landmark group, the front pad -
depends on the grid side s = ceil(sqrt(N)) only (model/dim1/TransMIL.py: side_geometry).  Within one side, (s - 1)^2 < N <=
s^2, a bag's length moves three things: N itself, add = s^2 - N, and the gather index of the sequence assembly.  All three are
read from the bag length ON THE DEVICE (csrc/transmil.hip: mil_tm_seq_index writes the index and the true row count that
`_fc1` runs under), so ONE captured graph per tuple of sides serves every bag of those sides: bags of 2 000 .. 15 592 patches
touch sides 45 .. 125, at most 81 graphs for one bag per step.  All graphs of a stepper share one memory pool.

    stepper = RaggedTransMILStepper(model, opt)        # model = aggregator_clip(TransMIL), opt = optim.FlatAdam(counted=True)
    slot = stepper.slot([n])                           # static inputs of the side: slot.x[:n], slot.len_dev, slot.y
    loss, prob = stepper.step(slot, [n])               # or cohort.feed(take, slot.x, slot.len_dev, slot.y) + on_device=True
    value = stepper.read_loss(loss)                    # the host sync; raises if a length left its side's bucket

The first visit of a key runs eagerly (through the same device-geometry body), the second captures; beyond `max_graphs`
graphs a new key keeps running eagerly.  Replayed body, in order: mil_tm_seq_index, the model's forward, the criterion, the
backward and - at world size 1 - the counted FlatAdam step; at world size > 1 the all-reduce and the update stay outside."""
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import ops
from .graph_step import GraphedStep
from .model.dim1.TransMIL import DeviceGeometry, bucket_side

# Measured on the MI355X (tools/bench_transmil.py): one graph alone keeps 306 MiB (s = 45), 868 MiB (s = 88),
# 1604 MiB (s = 125); in the shared pool 78 graphs of U[2000, 15 592] keep 3.0 GiB together (the largest graph plus ~18 MiB of
# outputs and gradients per further graph) next to 1.8 GiB of slot inputs.  96 covers all 81 sides of that regime with one bag
# per step and stays near 3.4 GiB, far inside the 24 GiB DeviceCohort.fits keeps free; the cap is for cohorts with many
# bags per step, whose keys are tuples of sides.
DEFAULT_MAX_GRAPHS = 96


class RaggedTransMILStepper:
    class Slot:
        def __init__(self, sides: Tuple[int, ...], L: int, C: int, device, pad_cache: dict, flag: torch.Tensor):
            self.sides = sides
            self.geom = DeviceGeometry(sides, device, pad_cache, flag)
            self.cap = self.geom.cap
            self.x = torch.zeros((self.cap, L), device=device, dtype=torch.float32)     # bags packed at the front
            self.y = torch.zeros((len(sides), C), device=device, dtype=torch.float32)
            self.len_dev, self.idx, self.rows_dev = self.geom.len_dev, self.geom.idx, self.geom.rows_dev
            self.last: Optional[dict] = None

    def __init__(self, model, opt=None, B: int = 1, use_graph: bool = True, max_graphs: Optional[int] = None,
                 backward: Optional[bool] = None, opt_in_graph: Optional[bool] = None, drop_seed: Optional[int] = None):
        """opt: optim.FlatAdam; inside the graph (opt_in_graph, default: world size 1) it must be counted.  opt=None with
        backward=True leaves the gradients in `.grad` (tests); backward=False is the evaluation stepper (model/aggregator_clip.py:
        graph_eval, the per-bag forward of test_ddp.py).
        drop_seed: the Philox seed of the model's dropout stream, fixed here - a captured step cannot draw it."""
        ext = model.extractor_pathology
        if type(ext).__name__ != "TransMIL":
            raise ValueError("RaggedTransMILStepper: the model's extractor is not TransMIL")
        self.model, self.opt, self.B, self.use_graph = model, opt, int(B), bool(use_graph)
        self.backward = (opt is not None) if backward is None else bool(backward)
        if opt is not None and not self.backward:
            raise ValueError("RaggedTransMILStepper: an optimizer needs the backward")
        world = getattr(opt, "world", 1) if opt is not None else 1
        self.opt_in_graph = (world == 1) if opt_in_graph is None else bool(opt_in_graph)
        if opt is not None and use_graph and self.opt_in_graph and not getattr(opt, "counted", False):
            raise ValueError("RaggedTransMILStepper: an optimizer inside the graph needs optim.FlatAdam(counted=True) "
                             "(step number and learning rate on the device)")
        self.device = next(model.parameters()).device
        self.L, self.C = int(ext.L), int(model.args.num_classes)
        # train_ddp.py:95-98: CrossEntropyLoss above two classes (on the sigmoid outputs, float one-hot targets)
        self.criterion = torch.nn.CrossEntropyLoss() if self.C > 2 else torch.nn.BCELoss()
        if drop_seed is not None:
            ext._drop_seed = int(drop_seed)
        ext._drop_state(self.device)                      # seed and pass counter exist before any capture
        self.flag = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._pad_cache: dict = {}
        self.slots: Dict[Tuple[int, ...], "RaggedTransMILStepper.Slot"] = {}
        params = list(opt.params) if opt is not None else [p for p in model.parameters() if p.requires_grad]
        cap = DEFAULT_MAX_GRAPHS if max_graphs is None else int(max_graphs)
        self.gs = GraphedStep(params, max_graphs=cap if self.use_graph else 0, share_pool=True, backward=self.backward)
        self.graph_bytes: Dict[tuple, int] = {}           # bytes each capture added to the graphs' shared memory pool
        self._pool_seen = 0

    @property
    def replays(self):
        return self.gs.replays

    @property
    def eager_steps(self):
        return self.gs.eager_steps

    @property
    def n_graphs(self):
        return len(self.gs._graphs)

    def slot(self, lengths: Sequence[int]) -> "RaggedTransMILStepper.Slot":
        if len(lengths) != self.B:
            raise ValueError(f"RaggedTransMILStepper: built for {self.B} bags per step, got {len(lengths)}")
        sides = tuple(bucket_side(int(n)) for n in lengths)
        s = self.slots.get(sides)
        if s is None:
            s = self.slots[sides] = self.Slot(sides, self.L, self.C, self.device, self._pad_cache, self.flag)
        return s

    def _body(self, slot):
        m = self.model
        slot.geom.update(slot.x)                          # index, true row count, zeroed tail: from slot.len_dev
        h, prob = m([slot.x], geom=slot.geom)
        loss = self.criterion(prob, slot.y)
        out = [loss, prob, h, m.last_logits]
        if m.training:                                    # the keep bits of this pass: static tensors once the graph replays
            for pair in m.extractor_pathology.last_bits:
                out += list(pair)
            out.append(m.last_mbits)
        if getattr(m, "patch_attn", False):               # [8, s_b^2] per layer and bag, zeros behind the length on the device
            out += list(m.last_patch_attn[0]) + list(m.last_patch_attn[1])
        return tuple(out)

    def key(self, sides: Sequence[int]) -> tuple:
        """The graph key of a slot of these sides under the model's switches as they stand now."""
        m = self.model
        attn = bool(getattr(m, "patch_attn", False))
        # a graph captured without the attention outputs is never replayed for a request with them, and the other way round;
        # nor one captured on one route for a model whose switches now name another: the route the extractor's forward will
        # resolve for this step (ops.tm_route) is part of the key
        route = ops.tm_route(m.extractor_pathology, len(sides), "cls" if attn else False)
        return (("transmil-sides", tuple(sides), bool(m.training), self.backward) + (("patch_attn",) if attn else ())
                + route.key())

    def step(self, slot, lengths: Sequence[int], on_device: bool = False):
        """One step on the bags packed at the front of slot.x.  on_device: the lengths already sit in slot.len_dev (the
        cohort's feed launch wrote them); otherwise they are copied there.  Returns (loss, prob); slot.last holds h, logits,
        in train mode the keep bits and, when model.patch_attn is set, patch_attn = [a0, a1] (per layer one [8, s_b^2] tensor per
        bag, zeros from the bag's length on) - static tensors of the key's graph once it replays."""
        lengths = [int(n) for n in lengths]
        if tuple(bucket_side(n) for n in lengths) != slot.sides:
            raise ValueError(f"RaggedTransMILStepper: lengths {lengths} do not belong to the slot of sides {slot.sides}")
        if not on_device:
            slot.len_dev.copy_(torch.tensor(lengths, dtype=torch.int32), non_blocking=True)
        m = self.model
        training = bool(m.training)
        attn = bool(getattr(m, "patch_attn", False))
        key = self.key(slot.sides)
        body = lambda: self._body(slot)      # noqa: E731
        ctr = m.extractor_pathology._drop_ctr
        # the warm-up passes in front of a capture draw masks too: the pass counter goes back, so the stream of a replayed
        # run stays the stream of an eager one
        rewind = (lambda: ops.counter_add(ctr, -self.gs.warmup)) if training else None      # noqa: E731
        in_graph = self.opt is not None and self.opt_in_graph
        if in_graph:
            self.opt.sync_lr()               # a changed learning rate reaches its device word before the replay reads it
        n0 = self.n_graphs
        out = self.gs.run(key, (), body, after_backward=self.opt.step if in_graph else None, before_capture=rewind)
        if self.n_graphs > n0:               # a capture happened: what it added to the shared pool (host bookkeeping only)
            now = self.pool_bytes()
            self.graph_bytes[key], self._pool_seen = now - self._pool_seen, now
        if self.opt is not None and not in_graph:
            self.opt.step()
        na = 2 * self.B if attn else 0
        slot.last = dict(h=out[2], logits=out[3], bits=list(out[4:len(out) - na]) if training else None,
                         patch_attn=[list(out[len(out) - na:len(out) - self.B]), list(out[len(out) - self.B:])] if attn else None)
        return out[0], out[1]

    def pool_bytes(self) -> int:
        """Device memory the shared pool of this stepper's graphs holds (the allocator's segments of that pool)."""
        pid = tuple(self.gs.pool)
        return sum(int(seg["total_size"]) for seg in torch.cuda.memory_snapshot() if tuple(seg["segment_pool_id"]) == pid)

    def read_loss(self, loss: torch.Tensor) -> float:
        """The step's loss on the host (a sync), after checking the device flag mil_tm_seq_index raises for a bag length
        outside its side's bucket - such a step ran on a clamped length."""
        v = float(loss.detach())
        if int(self.flag.item()):
            self.flag.zero_()
            raise RuntimeError("RaggedTransMILStepper: a bag length on the device lay outside its slot's grid side")
        return v
