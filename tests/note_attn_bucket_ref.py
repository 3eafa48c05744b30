"""Restatement, for any float dtype, of mil_bag_softmax_rows (csrc/attn_pool.hip): the gated-attention pool's weights over
a capacity bucket, whose rows are [cap patch rows | segment 0 of every bag | segment 1 of every bag | ..] and whose bags are
named by a row -> bag map (-1 on the padding rows).  float64 is the reference, the same code in float32 gives `e32`; mutate=
plants one error.  Also the host mirror of that row layout.  Test-side helper: nothing here reads the code under test."""
import torch

MUTATIONS = ("padding", "boundary")
# the kernel cases of tests/test_gpu_bag_softmax_rows.py: (cap, tail, lengths)
CASES = [(256, [1], [256]),                  # no padding row at all
         (256, [1], [70]),                   # a partial 32-row tile, padding tiles behind it
         (512, [1, 4, 1], [130, 70, 200]),   # three bags, three tail segments
         (256, [10], [100])]                 # a tail segment that fills a third of a tile


def row_bag(cap, tail, lengths):
    """int64 [cap + B sum(tail)]: the bag of every row of the bucket's multi-modal bag buffer, -1 on the padding rows.  The
    patches are packed from row 0; segment j of bag b lies at cap + B sum(tail[:j]) + b tail[j]."""
    B = len(lengths)
    assert sum(lengths) <= cap
    rb = torch.full((cap + B * sum(tail),), -1, dtype=torch.int64)
    r = 0
    for b, n in enumerate(lengths):
        rb[r:r + n] = b
        r += n
    base = cap
    for rows in tail:
        for b in range(B):
            rb[base + b * rows:base + (b + 1) * rows] = b
        base += B * rows
    return rb


def bag_order(rb, B):
    """(perm, off): the index that gathers the bucket's rows bag by bag, each bag's rows in memory order, and the bags' offsets
    in the gathered vector."""
    idx = [torch.nonzero(rb == b).reshape(-1) for b in range(B)]
    off = [0]
    for i in idx:
        off.append(off[-1] + int(i.numel()))
    return torch.cat(idx), off


def bag_softmax_rows(scores, rb, B, mutate=None):
    """w [R]: w[r] = exp(s_r - lse[bag(r)]) over the rows of bag(r), 0 where rb[r] < 0.  The scores of the padding rows are never
    read.  mutate: "padding" - the padding rows (read as score 0) are counted into the sum of the last bag; "boundary" - the
    first row of every bag but the first is taken for the bag in front of it (a bag index off by one where two bags meet in a
    tile)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    rb = rb.clone()
    if mutate == "boundary":
        for b in range(1, B):
            rb[int(torch.nonzero(rb == b)[0])] = b - 1
    w = torch.zeros_like(scores)
    for b in range(B):
        rows = rb == b
        s = scores[rows]
        m = s.max()
        l = (s - m).exp().sum()
        if mutate == "padding" and b == B - 1:
            l = l + int((rb < 0).sum()) * (0 - m).exp()
        w[rows] = (s - m).exp() / l
    return w


def scores_for(kind, rb, B, seed):
    """float32-exact float64 scores [R]: "normal" N(0, 1); "peak" one row per bag (its row 13 mod n) 30 above the rest; "equal"
    one value everywhere.  NaN on the padding rows: they must not be read."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rb.numel(), generator=g, dtype=torch.float64)
    if kind == "equal":
        s = torch.full_like(s, 0.375)
    elif kind == "peak":
        for b in range(B):
            rows = torch.nonzero(rb == b).reshape(-1)
            s[rows[13 % rows.numel()]] += 30.0
    else:
        assert kind == "normal", kind
    s = s.float().double()
    s[rb < 0] = float("nan")
    return s
