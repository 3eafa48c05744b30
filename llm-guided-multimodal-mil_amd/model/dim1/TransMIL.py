"""TransMIL (reference: model/dim1/TransMIL.py:8-107 with nystrom_attention's NystromAttention in its TransLayer), MI355X path.

Same constructor, parameter names and output `(h [B, 512], [attn0, attn1])` (need_attn: the whole maps, or "cls" for the cls
token's per-patch attention at any bag size).  Input: flat rows [R, L] plus per-bag lengths, or
[B, N, L] / [N, L].  Each bag runs alone (its own square padding, front pad and landmarks): a batch is B independent bags.
The one deliberate difference from upstream is there for B > 1 only: the pseudo-inverse's starting scale (max row sum x max
column sum of softmax(qL kL^T)) is taken per bag over its 8 heads, where upstream takes it over the whole batch.

Hot path: _fc1 / to_qkv / to_out on mil_gemm (ops.linear_act), LayerNorm on mil_layernorm_*, the Nystrom core, PPEG and the
sequence assembly on csrc/transmil.hip (ops.nystrom_core, ops.tm_ppeg, ops.tm_row_gather).  Train mode: to_out's Dropout(0.1)
draws Philox keep bits from the module's seed and a device pass counter, as ABMIL's masks do.  `TransMIL.deterministic` (None =
MIL_TM_DETERMINISTIC) puts every sum that crosses workgroups on its fixed-order entry: two runs then give the same bits.
`TransMIL.gemm_pieces` (None = MIL_TM_PIECES; 0 or 3) runs the Nystrom core's K >= 256 products on three-piece split-bf16 MFMA."""
import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ... import ops

TM_DROP_P = 0.1


def geometry(N: int) -> dict:
    """Per-bag shapes: grid side s, repeated rows add, sequence rows seq = s^2 + 1 (cls first), n_pad = 256 ceil(seq / 256),
    landmark group l = n_pad / 256, front zero pad rows."""
    s = int(math.ceil(math.sqrt(N)))
    add = s * s - N
    seq = s * s + 1
    n_pad = ops.TM_M * -(-seq // ops.TM_M)
    return dict(N=N, s=s, add=add, seq=seq, n_pad=n_pad, l=n_pad // ops.TM_M, pad=n_pad - seq)


def bucket_side(N: int) -> int:
    """Grid side s of a bag of N rows, (s - 1)^2 < N <= s^2, in integer arithmetic: the key of a captured step."""
    if N < 1:
        raise ValueError("TransMIL: a bag needs at least one row")
    return math.isqrt(N - 1) + 1


def side_geometry(s: int) -> dict:
    """What geometry(N) gives for every N of side s: all shapes but N and add."""
    seq = s * s + 1
    n_pad = ops.TM_M * -(-seq // ops.TM_M)
    return dict(s=s, seq=seq, n_pad=n_pad, l=n_pad // ops.TM_M, pad=n_pad - seq)


def seq_index_entry(j: int, N: int, off: int) -> int:
    """Entry j (0 <= j <= s^2) of a bag's part of the sequence index: -2 = the cls row, then the bag's N rows (the first of
    them row `off` of the flat input), then its first s^2 - N rows again.  csrc/transmil.hip: k_tm_seq_index evaluates this
    per entry from the lengths on the device."""
    return -2 if j == 0 else (off + j - 1 if j <= N else off + j - 1 - N)


def seq_index(lengths: Sequence[int]) -> List[int]:
    """The index of the sequence assembly for bags packed back to back: per bag [cls | tokens | first `add` tokens again]."""
    idx, off = [], 0
    for n in lengths:
        add = bucket_side(n) ** 2 - n
        idx += [-2] + list(range(off, off + n)) + list(range(off, off + add))
        off += n
    return idx


def seg_index_entry(j: int, s: int, bag_segs: Sequence[Tuple[int, int]], x_rows: Optional[int] = None) -> int:
    """Entry j (0 <= j <= s^2) of one bag whose rows lie in the pieces bag_segs = [(first row, length), ..] of the source, in
    sequence order: -2 = the cls row, the pieces' rows one after another (L of them), then the first s^2 - L again.  The
    position is clamped into [0, L - 1]; no rows at all, or a row outside [0, x_rows), give -1 (a zero row).
    csrc/transmil.hip: k_tm_seq_index_segs evaluates exactly this per entry from the table on the device."""
    if j == 0:
        return -2
    lens = [max(int(n), 0) for _, n in bag_segs]
    L = sum(lens)
    if L == 0:
        return -1
    pos = j - 1
    if pos >= L:
        pos -= L
    pos = min(max(pos, 0), L - 1)
    for (first, _), n in zip(bag_segs, lens):
        if pos < n:
            row = int(first) + pos
            return row if row >= 0 and (x_rows is None or row < x_rows) else -1
        pos -= n
    return -1


def seq_index_segments(segs: Sequence[Sequence[Tuple[int, int]]], sides: Optional[Sequence[int]] = None,
                       x_rows: Optional[int] = None) -> List[int]:
    """The index of the sequence assembly for bags whose rows are NOT packed back to back (the fusion model's multi-modal
    bag): segs[b] = the bag's (first row, length) pieces in sequence order, sides[b] its grid side (default: the side of its
    row count).  The host mirror of ops.tm_seq_index_segs, entry by entry."""
    idx: List[int] = []
    for b, bag in enumerate(segs):
        s = int(sides[b]) if sides is not None else bucket_side(sum(max(int(n), 0) for _, n in bag))
        idx += [seg_index_entry(j, s, bag, x_rows) for j in range(1 + s * s)]
    return idx


def bucket_segments(lengths: Sequence[int], cap: int, tail: Sequence[int]) -> Tuple[List[List[Tuple[int, int]]], int]:
    """(the pieces of every bag of a capacity bucket in sequence order, the rows of the source): the source is [cap patch rows
    | B x tail[0] | B x tail[1] | ..], bag b's sequence is its tail segments in row order, then its patches (upstream
    aggregator.py:173,192).  A length is read as min(max(len, 0), rows of the source), as the kernel reads it."""
    B, cap, tail = len(lengths), int(cap), [int(t) for t in tail]
    x_rows = cap + B * sum(tail)
    lens = [min(max(int(n), 0), x_rows) for n in lengths]
    segs, off = [], 0
    for b in range(B):
        bag, base = [], cap
        for t in tail:
            bag.append((base + b * t, t))
            base += B * t
        bag.append((off, lens[b]))
        off += lens[b]
        segs.append(bag)
    return segs, x_rows


def seq_index_bucket(lengths: Sequence[int], cap: int, tail: Sequence[int], sides: Optional[Sequence[int]] = None) -> List[int]:
    """The host mirror of ops.tm_seq_index_bucket (csrc/transmil.hip: k_tm_seq_index_bucket), entry by entry: the pieces from
    the lengths, then seq_index_segments on them.  sides default to the side of each bag's len + sum(tail) rows."""
    segs, x_rows = bucket_segments(lengths, cap, tail)
    return seq_index_segments(segs, sides, x_rows)


def segment_table(segs: Sequence[Sequence[Tuple[int, int]]], sides: Optional[Sequence[int]] = None) -> Tuple[List[List[int]], int]:
    """(rows of the int32 table ops.tm_seq_index_segs reads - per bag [s, first0, len0, .. first3, len3] -, the number of
    index entries sum(1 + s^2))."""
    rows, total = [], 0
    for b, bag in enumerate(segs):
        if len(bag) > ops.TM_SEG_MAX:
            raise ValueError(f"TransMIL: a bag of {len(bag)} segments (at most {ops.TM_SEG_MAX})")
        s = int(sides[b]) if sides is not None else bucket_side(sum(max(int(n), 0) for _, n in bag))
        row = [s]
        for first, n in bag:
            row += [int(first), int(n)]
        rows.append(row + [0] * (ops.TM_SEG_STRIDE - len(row)))
        total += 1 + s * s
    return rows, total


def pad_index(g: dict) -> List[int]:
    """Front zero pad of one bag's rows to n_pad: -1 = a zero row.  Depends on the side only."""
    return [-1] * g["pad"] + list(range(g["seq"]))


def packed_index(sides: Sequence[int]) -> Tuple[List[int], List[int], List[int]]:
    """The static indices of the packed route for bags of these grid sides, one bag after another:
    (pad [sum n_pad]: every bag's pad_index with its rows shifted by the sequence rows in front of the bag - -1 stays a zero row;
     unpad [sum seq]: where sequence row j of bag b lies among the padded rows, pad_b + j behind the padded rows in front;
     blocks [B]: n_pad_b / 256, what ops.tm_packed_table takes)."""
    pad, unpad, blocks, row, prow = [], [], [], 0, 0
    for s in sides:
        g = side_geometry(int(s))
        pad += [i if i < 0 else row + i for i in pad_index(g)]
        unpad += range(prow + g["pad"], prow + g["n_pad"])
        blocks.append(g["l"])
        row += g["seq"]
        prow += g["n_pad"]
    return pad, unpad, blocks


def _check_need_attn(need_attn):
    if not (isinstance(need_attn, bool) or (isinstance(need_attn, str) and need_attn == "cls")):
        raise ValueError(f"TransMIL: need_attn must be False, True or 'cls', got {need_attn!r}")


class PackedGeometry:
    """packed_index on the device plus the block table, the PPEG table (ops.tm_ppeg_table: the unpadded sequence rows, per-bag
    row offsets and sides) and the cls attention's table (ops.tm_cls_table: per-bag sides and output offsets): what
    TransMIL._run_bags reads on the packed route.  It depends on the tuple of sides alone; a replayed step builds
    it once, with its geometry, outside the capture."""

    def __init__(self, sides: Sequence[int], device):
        pad, unpad, blocks = packed_index(sides)
        self.sides = tuple(int(s) for s in sides)
        self.pad_idx = torch.tensor(pad, dtype=torch.int32).to(device, non_blocking=True)
        self.unpad_idx = torch.tensor(unpad, dtype=torch.int32).to(device, non_blocking=True)
        self.table = ops.tm_packed_table(blocks, device)
        self.ppeg_table = ops.tm_ppeg_table(self.sides, device)
        self.cls_table = ops.tm_cls_table(self.sides, device)


def _static_geometry(sides: Sequence[int], device, pad_cache: Optional[dict]):
    """What a captured step's geometry holds that depends on the sides alone: (the pad index per side - filled into pad_cache,
    which a stepper shares among its slots -, the packed route's static tables, None for a single bag)."""
    pad_idx = pad_cache if pad_cache is not None else {}
    for s in sides:
        if s not in pad_idx:
            pad_idx[s] = torch.tensor(pad_index(side_geometry(s)), dtype=torch.int32).to(device)
    return pad_idx, PackedGeometry(sides, device) if len(sides) > 1 else None


class DeviceGeometry:
    """The part of a forward's geometry that a replayed step cannot build on the host: the grid side of every bag (host
    ints, fixed per captured graph), the gather index and the true row count on the device (ops.tm_seq_index writes both
    from the lengths in `len_dev`), the per-side pad index (static) and the out-of-bucket flag."""

    def __init__(self, sides: Sequence[int], device, pad_cache: Optional[dict] = None, flag: Optional[torch.Tensor] = None):
        self.sides = tuple(int(s) for s in sides)
        self.cap = sum(s * s for s in self.sides)                         # rows of the flat input buffer
        i32 = dict(device=device, dtype=torch.int32)
        self.len_dev = torch.zeros(len(self.sides), **i32)
        self.idx = torch.zeros(sum(1 + s * s for s in self.sides), **i32)
        self.rows_dev = torch.zeros(1, **i32)
        self.flag = flag if flag is not None else torch.zeros(1, **i32)
        self.pad_idx, self.packed = _static_geometry(self.sides, device, pad_cache)

    def update(self, x_tail: Optional[torch.Tensor] = None):
        """Index and row count from the lengths now in len_dev; x_tail: the slot's input buffer, its rows behind the bags zeroed."""
        ops.tm_seq_index(self.len_dev, self.sides, self.idx, self.rows_dev, self.flag, x_tail)
        return self


class BucketGeometry:
    """DeviceGeometry's counterpart for the fusion model's capacity bucket (segments.FusionBucket): the bags' rows lie in
    pieces of [cap patch rows | B x tail_j ..], the patch counts sit in the bucket's `len_dev`, and a captured step is keyed by
    (cap, sides).  Holds the gather index ops.tm_seq_index_bucket writes from those lengths, the sequence lengths `L_dev`, the
    STATIC index that puts the cls row in front of every bag (cls_idx: -2 at a bag's first entry, the entry's own row elsewhere),
    the per-side pad index and the out-of-bucket flag."""

    def __init__(self, cap: int, tail: Sequence[int], sides: Sequence[int], device, pad_cache: Optional[dict] = None,
                 flag: Optional[torch.Tensor] = None):
        self.cap, self.tail = int(cap), tuple(int(t) for t in tail)
        self.sides = tuple(int(s) for s in sides)
        self.B = len(self.sides)
        self.x_rows = self.cap + self.B * sum(self.tail)                  # rows of the multi-modal bag buffer
        i32 = dict(device=device, dtype=torch.int32)
        self.total = sum(1 + s * s for s in self.sides)
        self.idx = torch.zeros(self.total, **i32)
        self.len_dev = self.L_dev = torch.zeros(self.B, **i32)            # the SEQUENCE rows per bag (patches + tail)
        self.flag = flag if flag is not None else torch.zeros(1, **i32)
        cls_idx, row = [], 0
        for s in self.sides:
            cls_idx += [-2] + list(range(row + 1, row + 1 + s * s))
            row += 1 + s * s
        self.cls_idx = torch.tensor(cls_idx, dtype=torch.int32).to(device)
        self.pad_idx, self.packed = _static_geometry(self.sides, device, pad_cache)

    def update(self, patch_len_dev: torch.Tensor):
        """Index and sequence lengths from the patch counts now on the device (the bucket's len_dev)."""
        ops.tm_seq_index_bucket(patch_len_dev, self.cap, self.tail, self.sides, self.idx, self.L_dev, self.flag)
        return self


class NystromAttention(nn.Module):
    """Parameters of nystrom_attention.NystromAttention(dim=512, dim_head=64, heads=8, num_landmarks=256, pinv_iterations=6,
    residual=True, dropout=0.1): to_qkv (no bias), to_out = Linear + Dropout, res_conv = depthwise (33, 1) over the heads."""

    def __init__(self, dim: int = 512, heads: int = 8, dim_head: int = 64, dropout: float = TM_DROP_P):
        super().__init__()
        self.heads = heads
        self.to_qkv = nn.Linear(dim, 3 * heads * dim_head, bias=False)
        self.to_out = nn.Sequential(nn.Linear(heads * dim_head, dim), nn.Dropout(dropout))
        self.res_conv = nn.Conv2d(heads, heads, (ops.TM_CONV, 1), padding=(ops.TM_CONV // 2, 0), groups=heads, bias=False)


class TransLayer(nn.Module):
    """x + to_out(Nystrom(LN(x))).  One front and one back around the core; `route` (ops.TmRoute) names the core's entries."""

    def __init__(self, norm_layer=nn.LayerNorm, dim: int = 512):
        super().__init__()
        self.norm = norm_layer(dim)
        self.attn = NystromAttention(dim=dim)

    def front(self, x: torch.Tensor, pad_idx: torch.Tensor, route) -> torch.Tensor:
        """LayerNorm, the zero rows in front (one gather through pad_idx) and to_qkv: x [rows, 512] -> [padded rows, 1536]."""
        ln = ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return ops.linear_act(ops.tm_row_gather(ln, None, pad_idx, route.det), self.attn.to_qkv.weight, None)

    def back(self, x: torch.Tensor, o: torch.Tensor, bits: Optional[torch.Tensor]) -> torch.Tensor:
        """to_out on the core's rows o (those of x) and the residual: fused into the product, or behind the dropout of `bits`."""
        lin = self.attn.to_out[0]
        if bits is None:
            return ops.linear_act(o, lin.weight, lin.bias, residual=x)
        return x + ops.dropout_bits(ops.linear_act(o, lin.weight, lin.bias), bits, 1.0 / (1.0 - TM_DROP_P))

    def run(self, x: torch.Tensor, g: dict, pad_idx: torch.Tensor, bits: Optional[torch.Tensor], need_attn, route,
            cls: Optional[dict] = None):
        """x [seq, 512] of one bag -> (the layer's rows, attn map / cls attention [8, s^2] / None).
        cls: the bag length for need_attn="cls", dict(n=N) or dict(len_dev=.., bag=b)."""
        geo = dict(pad=g["pad"], s=g["s"], **cls) if cls is not None else {}
        o, attn = ops.nystrom_core(self.front(x, pad_idx, route), self.attn.res_conv.weight, need_attn, fused_a3=route.fused_a3,
                                   fused_a1=route.fused_a1, fused_cls=route.cls == "fused", deterministic=route.det,
                                   pieces=route.pieces, **geo)
        return self.back(x, o[g["pad"]:], bits), attn

    def run_bags(self, xs: Sequence[torch.Tensor], geo: Sequence[dict], pad_idxs: Sequence[torch.Tensor],
                 bits: Sequence[Optional[torch.Tensor]], route) -> List[torch.Tensor]:
        """run() (need_attn False) over all bags of a step, stage by stage: the front per bag; the Nystrom cores of all bags as
        one ops.nystrom_core_bags, whose landmark-side chain is one set of launches at batch 8 x bags; the back per bag.  Bag
        b's values are those of run() on bag b."""
        qkvs = [self.front(x, pad_idx, route) for x, pad_idx in zip(xs, pad_idxs)]
        outs = ops.nystrom_core_bags(qkvs, self.attn.res_conv.weight, fused_a3=route.fused_a3, fused_a1=route.fused_a1,
                                     deterministic=route.det, pieces=route.pieces)
        return [self.back(x, o[g["pad"]:], keep) for x, g, o, keep in zip(xs, geo, outs, bits)]

    def run_packed(self, x: torch.Tensor, pk: PackedGeometry, bits: Optional[torch.Tensor], route, cls: Optional[dict] = None):
        """run() over all bags of a step as ONE packed sequence: x [sum seq, 512], the bags' sequences one after another ->
        (the same rows, None).  One front into [sum n_pad, 1536], ops.nystrom_core_packed, one gather back, one back (bits
        [sum seq, 16], each bag's words in its row slice).  cls (need_attn="cls"): the bag lengths, dict(n=[..]) or
        dict(len_dev=..) -> (the rows, [one [8, s_b^2] cls attention per bag]), formed by the core in one launch set."""
        attn = None
        kw = dict(deterministic=route.det, pieces=route.pieces)
        if cls is None:
            o = ops.nystrom_core_packed(self.front(x, pk.pad_idx, route), pk.table, self.attn.res_conv.weight, **kw)
        else:
            o, attn = ops.nystrom_core_packed(self.front(x, pk.pad_idx, route), pk.table, self.attn.res_conv.weight,
                                              need_attn="cls", cls=dict(sides=pk.cls_table, **cls), **kw)
        return self.back(x, ops.tm_row_gather(o, None, pk.unpad_idx, route.det), bits), attn


class PPEG(nn.Module):
    def __init__(self, dim: int = 512):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, 7, 1, 7 // 2, groups=dim)
        self.proj1 = nn.Conv2d(dim, dim, 5, 1, 5 // 2, groups=dim)
        self.proj2 = nn.Conv2d(dim, dim, 3, 1, 3 // 2, groups=dim)

    def run(self, x: torch.Tensor, s: int, deterministic: bool) -> torch.Tensor:
        return ops.tm_ppeg(x, s, self.proj.weight, self.proj.bias, self.proj1.weight, self.proj1.bias, self.proj2.weight,
                           self.proj2.bias, deterministic)

    def run_packed(self, x: torch.Tensor, table, deterministic: bool) -> torch.Tensor:
        """run() over all bags of a step in one launch set: x [sum (1 + s_b^2), 512], the bags' sequences one after another,
        table = PackedGeometry.ppeg_table -> the same rows (ops.tm_ppeg_packed)."""
        return ops.tm_ppeg_packed(x, table, self.proj.weight, self.proj.bias, self.proj1.weight, self.proj1.bias, self.proj2.weight,
                                  self.proj2.bias, deterministic)


class TransMIL(nn.Module):
    """The reference's TransMIL extractor on the HIP kernels of csrc/transmil.hip: _fc1, the cls token, two Nystrom layers with
    PPEG between them, LayerNorm of the cls rows; one bag or a ragged batch of bags per call.
    Switches, each an attribute that overrides its environment variable when not None (all default off): fused_cls
    (MIL_TM_FUSED_CLS), deterministic (MIL_TM_DETERMINISTIC), gemm_pieces (MIL_TM_PIECES), batch_bags (MIL_TM_BATCH_BAGS), packed
    (MIL_TM_PACKED), packed_ppeg (MIL_TM_PACKED_PPEG), packed_cls (MIL_TM_PACKED_CLS).  Which of them take effect in a step, and
    which wins, is decided once per step by ops.tm_route and stated there, nowhere else.  The routes:
    each - bag by bag;
    batched - stage by stage across the bags, the landmark-side chain of each layer (A2, the pseudo-inverse, U and their
    gradients) as one set of launches for all bags (ops.nystrom_core_bags); every bag keeps its own pseudo-inverse scale and the
    values of the bag-by-bag route (bit-equal under deterministic); the token-side passes, the dense layers and PPEG stay per bag;
    packed - every layer over ONE packed sequence of all bags' rows (ops.nystrom_core_packed), every stage but PPEG one launch
    set whatever the bag count; with packed_ppeg PPEG too (ops.tm_ppeg_packed), with no per-bag slice or concatenation between
    the layers; with packed_cls the bags' per-patch cls attention of each layer as well (ops.tm_cls_attention_packed)."""

    def __init__(self, n_classes: int, L: int = 768, D: int = 512, K: int = 1):
        super().__init__()
        if D != ops.TM_D or K != 1:
            raise NotImplementedError("the HIP TransMIL kernels are built for D=512 (8 heads x 64), K=1 (the reference's values)")
        self.L, self.D, self.K = L, D, K
        self.pos_layer = PPEG(dim=D)
        self._fc1 = nn.Sequential(nn.Linear(L, D), nn.ReLU())
        self.cls_token = nn.Parameter(torch.randn(1, 1, D))
        self.n_classes = n_classes
        self.layer1 = TransLayer(dim=D)
        self.layer2 = TransLayer(dim=D)
        self.norm = nn.LayerNorm(D)
        self._fc2 = nn.Linear(D, n_classes)          # upstream keeps it but never calls it (TransMIL.py:99-104)
        self._drop_seed: Optional[int] = None
        self._drop_ctr: Optional[torch.Tensor] = None
        self.last_bits: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = None
        self.force_bits: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = None   # tests: masks supplied from outside
        self.fused_cls: Optional[bool] = None        # need_attn="cls" on the fused passes (ops.nystrom_core); None = MIL_TM_FUSED_CLS
        self.deterministic: Optional[bool] = None    # every cross-workgroup sum in a fixed order (ops.tm_deterministic); None = MIL_TM_DETERMINISTIC
        self.gemm_pieces: Optional[int] = None       # 3: the Nystrom core's products on split-bf16 MFMA (ops.tm_pieces); None = MIL_TM_PIECES
        self.batch_bags: Optional[bool] = None       # a step's bags through one landmark-side chain (ops.tm_batch_bags); None = MIL_TM_BATCH_BAGS
        self.packed: Optional[bool] = None           # a step's bags as one packed sequence (ops.tm_packed); None = MIL_TM_PACKED
        self.packed_ppeg: Optional[bool] = None      # on the packed route, PPEG as one launch set too (ops.tm_packed_ppeg); None = MIL_TM_PACKED_PPEG
        self.packed_cls: Optional[bool] = None       # need_attn="cls" on the packed route too (ops.tm_packed_cls); None = MIL_TM_PACKED_CLS

    def _drop_state(self, device):
        if self._drop_seed is None:
            self._drop_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if self._drop_ctr is None or self._drop_ctr.device != device:
            self._drop_ctr = torch.zeros(1, device=device, dtype=torch.int32)

    def _bits(self, b: int, seq: int, device, out=(None, None)):
        """Keep bits of the two Dropout(0.1) of bag b: key seed ^ layer, stream offset 2 b (+1) + the device pass counter.
        out: per layer where the words go (the packed route: the bag's rows of the step's buffer); default fresh tensors."""
        if self.force_bits is not None:
            return self.force_bits[b]
        return tuple(ops.dropout_keep_bits(seq, self.D, TM_DROP_P, self._drop_seed ^ (0x5472616E734D494C + j), 2 * b + j, device,
                                           out=out[j], offset_dev=self._drop_ctr) for j in range(2))

    def forward(self, x: torch.Tensor, lengths: Optional[Sequence[int]] = None, need_attn=False,
                geom: Optional[DeviceGeometry] = None):
        """geom: the capture-safe form (RaggedTransMILStepper).  x is then the slot's whole [sum s^2, L] buffer, the bags packed
        at its front, and nothing below touches the host: sides from geom, index / row count / pad index on the device.
        need_attn: False -> (h, [None, None]); True -> the layers' whole [8, n_pad, n_pad] maps (n_pad^2 memory: small bags
        only); "cls" -> (h, [a0, a1]), a_l a list with one [8, N_b] tensor per bag: what the cls token gives each patch in
        layer l, a repeated patch's two keys summed (ops.tm_cls_attention; any bag size, train or eval).  With geom each entry is
        the static [8, s_b^2] tensor, zeros behind the bag's length on the device."""
        _check_need_attn(need_attn)
        dev = x.device
        if geom is not None:
            if x.dim() != 2 or x.shape[0] != geom.cap:
                raise ValueError(f"TransMIL: geom of sides {geom.sides} wants a [{geom.cap}, L] input, got {tuple(x.shape)}")
            if self.training and (self._drop_seed is None or self._drop_ctr is None or self._drop_ctr.device != dev):
                raise ValueError("TransMIL: fix the dropout stream (_drop_state) before a forward with geom")
            # _fc1 runs over the slot's capacity.  The rows behind the true count hold an earlier step's data: they are never
            # gathered, so their gradient rows are zero, but 0 x NaN in _fc1's weight gradient would still poison it.
            # ops.tm_seq_index (geom.update) has ZEROED that tail of x, which holds for every kernel _fc1 dispatches to;
            # rows_dev on top lets the tall kernels skip the tiles behind the count (the few-rows kernels ignore it).
            h = ops.linear_act(x, self._fc1[0].weight, self._fc1[0].bias, "relu", rows_dev=geom.rows_dev)
            geo = [side_geometry(s) for s in geom.sides]
            idx_dev = geom.idx
        else:
            if x.dim() == 2 and lengths is None:
                x = x.unsqueeze(0)
            if x.dim() == 3:
                B, N, L = x.shape
                lengths = [N] * B
                x = x.reshape(B * N, L)
            lengths = [int(n) for n in lengths]
            if min(lengths) < 1 or sum(lengths) != x.shape[0]:
                raise ValueError(f"TransMIL: lengths {lengths} do not cover the {x.shape[0]} rows")
            h = ops.linear_act(x, self._fc1[0].weight, self._fc1[0].bias, "relu")        # [R, 512]
            geo = [geometry(n) for n in lengths]
            # [cls | tokens | first `add` tokens again] per bag, one gather for all bags; index -2 = the cls row
            idx_dev = torch.tensor(seq_index(lengths), dtype=torch.int32).to(dev, non_blocking=True)
        return self._run_bags(h, idx_dev, geo, need_attn, geom)

    def flat_segments(self, x0: torch.Tensor, segs: Sequence[Sequence[Tuple[int, int]]], need_attn=False):
        """forward() over rows that are not contiguous per bag: x0 [R, L], segs[b] = the bag's (first row, length) pieces in
        SEQUENCE order (at most ops.TM_SEG_MAX).  _fc1 + ReLU runs over all R rows in whatever order they lie, the sequences
        [cls | the bag's rows | its first s^2 - L_b rows again] are assembled through an index written on the device from the
        [B, 9] table of the pieces (ops.tm_seq_index_segs: no list of 1 + s^2 ints per bag is built or uploaded), then the
        bags run as in forward().  Same returns; with need_attn="cls" bag b's entries are [8, L_b] in sequence order.  Rows of
        x0 that no bag names get a zero gradient."""
        _check_need_attn(need_attn)
        if x0.dim() != 2 or x0.shape[1] != self.L:
            raise ValueError(f"TransMIL: flat_segments wants rows [R, {self.L}], got {tuple(x0.shape)}")
        R = x0.shape[0]
        segs = [[(int(f), int(n)) for f, n in bag] for bag in segs]
        for b, bag in enumerate(segs):                                      # the kernel clamps and flags; eager mode refuses
            if sum(n for _, n in bag) < 1 or any(n < 0 or f < 0 or f + n > R for f, n in bag):
                raise ValueError(f"TransMIL: segments {bag} of bag {b} do not lie in the {R} rows (or hold none)")
        rows, total = segment_table(segs)
        table = torch.tensor(rows, dtype=torch.int32).to(x0.device, non_blocking=True)
        h = ops.linear_act(x0, self._fc1[0].weight, self._fc1[0].bias, "relu")        # [R, 512]
        idx_dev = ops.tm_seq_index_segs(table, total, R)
        return self._run_bags(h, idx_dev, [geometry(sum(n for _, n in bag)) for bag in segs], need_attn, None)

    def flat_bucket(self, x0: torch.Tensor, geom: BucketGeometry, patch_len_dev: torch.Tensor, need_attn=False):
        """flat_segments() in its capture-safe form, for a step replayed from a hipGraph: x0 [cap + B sum(tail), L] is the
        bucket's multi-modal bag buffer, the patch counts are on the device, the sides come from geom - nothing below touches
        the host.  Rows [sum of the lengths, cap) of x0 hold whatever an earlier step left there; x0 is an autograd intermediate
        and cannot be cleared, and although those rows are never gathered (zero gradient rows), _fc1's weight gradient over all
        of x0 would still multiply what they hold.  So the order is turned round: the bags' rows are gathered FIRST (the cls
        entries read as zero rows), _fc1 + ReLU runs over the gathered [sum(1 + s_b^2), L] rows - it is row-wise, so the values
        are those of flat_segments, and a repeated row adds twice in dW as it does through the gather's backward there -, and a
        second gather through the static cls_idx puts the cls token in front of every bag.  No product ever reads a row of x0
        that no bag names.  Returns (h [B, D], [None, None]); with need_attn="cls" (no other form is offered here) the second is
        [attn0, attn1], per layer one static [8, s_b^2] tensor per bag in SEQUENCE order - the tail segments, then the patches -
        with zeros from the bag's length on the device on.  The route is the one ops.tm_route gives for that need_attn."""
        if not (need_attn is False or (isinstance(need_attn, str) and need_attn == "cls")):
            raise ValueError(f"TransMIL: flat_bucket offers need_attn False or 'cls', got {need_attn!r}")
        if x0.dim() != 2 or x0.shape[1] != self.L or x0.shape[0] != geom.x_rows:
            raise ValueError(f"TransMIL: flat_bucket wants rows [{geom.x_rows}, {self.L}], got {tuple(x0.shape)}")
        if self.training and (self._drop_seed is None or self._drop_ctr is None or self._drop_ctr.device != x0.device):
            raise ValueError("TransMIL: fix the dropout stream (_drop_state) before a forward with geom")
        geom.update(patch_len_dev)
        route = ops.tm_route(self, len(geom.sides), need_attn)
        rows = ops.tm_row_gather(x0, None, geom.idx, route.det)                         # [sum(1 + s^2), L]
        h = ops.linear_act(rows, self._fc1[0].weight, self._fc1[0].bias, "relu")
        return self._run_bags(h, geom.cls_idx, [side_geometry(s) for s in geom.sides], need_attn, geom, route)

    def _keep_bits(self, rows: List[int], dev, packed: bool):
        """All bags' keep bits in front of the layers, for the batched and the packed route -> (bits: per bag those of (layer1,
        layer2), the bag-by-bag route's; keep: per layer the words of all bags as one [sum seq, 16] tensor for the packed
        route, else (None, None)).  The packed route draws each bag's words into its row slice of the step's buffer, so `bits`
        are views of `keep`."""
        bags = range(len(rows) - 1)
        if not packed:
            return [self._bits(b, rows[b + 1] - rows[b], dev) for b in bags], (None, None)
        if self.force_bits is not None:
            bits = [self._bits(b, 0, dev) for b in bags]
            return bits, tuple(torch.cat([k[j] for k in bits], 0) for j in range(2))
        keep = tuple(torch.empty((rows[-1], self.D // 32), device=dev, dtype=torch.int32) for _ in range(2))
        return [self._bits(b, rows[b + 1] - rows[b], dev, tuple(k[rows[b]:rows[b + 1]] for k in keep)) for b in bags], keep

    def _run_bags(self, h: torch.Tensor, idx: torch.Tensor, geo: List[dict], need_attn, geom, route=None):
        """h [rows, 512] behind _fc1 and the index that assembles the sequences [sum(1 + s_b^2), 512], one bag after another:
        layer1 -> PPEG -> layer2 -> norm of the cls rows, on the route ops.tm_route resolves here, once, from the module's
        switches, the number of bags and need_attn (flat_bucket hands in the one it resolved).  The routes share the prologue (the
        dropout stream, the keep bits of every (bag, layer) - the bag-by-bag route draws a bag's, and uploads its pad index, just
        in front of that bag's layers, so that this host work runs under the launches of the bag before) and the epilogue (the pass counter advances once, last_bits is the per-bag list, the norm of the cls rows,
        the attention in its three forms); only the layers between differ.  On the batched and the packed route all bags' layer
        tensors are alive at once: in eval mode, where the bag-by-bag route frees a bag's before the next, the peak grows with
        the number of bags.  need_attn="cls" returns [attn0, attn1], each a list with one tensor per bag: [8, N_b] with host
        lengths, the static [8, s_b^2] with zeros from the device length on with geom."""
        route = route or ops.tm_route(self, len(geo), need_attn)
        seqs = ops.tm_row_gather(h, self.cls_token, idx, route.det)
        dev, train, packed = seqs.device, self.training, route.bags == "packed"
        rows = [0]
        for g in geo:
            rows.append(rows[-1] + g["seq"])
        bits, keep = [(None, None)] * len(geo), (None, None)
        if train:
            self._drop_state(dev)
            if route.bags != "each":
                bits, keep = self._keep_bits(rows, dev, packed)
        if packed:
            pk = geom.packed if geom is not None else PackedGeometry([g["s"] for g in geo], dev)   # host lengths: built per call
            cls = None
            if route.cls:               # host lengths are uploaded once here, outside any capture
                cls = dict(len_dev=geom.len_dev if geom is not None else
                           torch.tensor([g["N"] for g in geo], dtype=torch.int32).to(dev, non_blocking=True))
            x, attn0 = self.layer1.run_packed(seqs, pk, keep[0], route, cls)
            if route.ppeg_packed:       # one launch set on the rows as they stand; else per bag on row slices: its grid follows the side
                x = self.pos_layer.run_packed(x, pk.ppeg_table, route.det)
            else:
                x = torch.cat([self.pos_layer.run(x[rows[b]:rows[b + 1]], g["s"], route.det) for b, g in enumerate(geo)], 0)
            x, attn1 = self.layer2.run_packed(x, pk, keep[1], route, cls)
            cls_rows = [x[r:r + 1] for r in rows[:-1]]
        else:
            xs = [seqs[rows[b]:rows[b + 1]] for b in range(len(geo))]
            attn0, attn1 = [], []

            def pad_of(g):
                if geom is not None:
                    return geom.pad_idx[g["s"]]
                return torch.tensor(pad_index(g), dtype=torch.int32).to(dev, non_blocking=True)
            if route.bags == "batched":
                pads = [pad_of(g) for g in geo]
                xs = self.layer1.run_bags(xs, geo, pads, [k[0] for k in bits], route)
                xs = [self.pos_layer.run(x, g["s"], route.det) for x, g in zip(xs, geo)]
                xs = self.layer2.run_bags(xs, geo, pads, [k[1] for k in bits], route)
            else:
                for b, g in enumerate(geo):
                    pad = pad_of(g)
                    if train:
                        bits[b] = self._bits(b, g["seq"], dev)
                    cls = None
                    if route.cls:
                        cls = dict(len_dev=geom.len_dev, bag=b) if geom is not None else dict(n=g["N"])
                    x, a0 = self.layer1.run(xs[b], g, pad, bits[b][0], need_attn, route, cls)
                    x = self.pos_layer.run(x, g["s"], route.det)
                    xs[b], a1 = self.layer2.run(x, g, pad, bits[b][1], need_attn, route, cls)
                    attn0.append(a0)
                    attn1.append(a1)
            cls_rows = [x[:1] for x in xs]
        if train and self.force_bits is None:
            ops.counter_add(self._drop_ctr, 1)
        self.last_bits = bits if train else None
        hc = cls_rows[0] if len(cls_rows) == 1 else torch.cat(cls_rows, 0)
        out = ops.layer_norm(hc, self.norm.weight, self.norm.bias, self.norm.eps)     # norm of the cls rows only
        if need_attn is False:
            return out, [None, None]
        if route.cls and geom is None:
            attn0, attn1 = ([a[:, :g["N"]] for a, g in zip(attn, geo)] for attn in (attn0, attn1))
        if need_attn is True and len(geo) == 1:
            return out, [attn0[0].unsqueeze(0), attn1[0].unsqueeze(0)]
        return out, [attn0, attn1]      # several bags: one [8, n_pad, n_pad] map, or one cls attention, per bag
