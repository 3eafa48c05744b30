"""CPU: the sequence index of the fusion model's multi-modal bag under a TransMIL aggregator (model/dim1/TransMIL.py:
seq_index_segments, the host mirror of csrc/transmil.hip: k_tm_seq_index_segs) as a definition - against a literal
concatenation of aranges -, and the entry point's refusal of --fusion_transmil 1 together with --hip_graph 1."""
import random

import pytest
import torch


def bag_segments(desc):
    """Bag descriptions (P, n) / (P, D, P, n) / (P,) per bag -> segs[b] = [(first row, length), ..] in upstream's sequence order,
    against rows laid out as model/aggregator.py lays them out: [patches | tokens], [patches | q_ct | k_ct | q_p], [tokens]."""
    B = len(desc)
    kind = len(desc[0])
    assert all(len(d) == kind for d in desc)
    if kind == 1:
        segs, off = [], 0
        for (P,) in desc:
            segs.append([(off, P)])
            off += P
        return segs, off
    if kind == 2:
        R = sum(n for _, n in desc)
        segs, off, tok = [], 0, R
        for P, n in desc:
            segs.append([(tok, P), (off, n)])
            off += n
            tok += P
        return segs, tok
    assert kind == 4
    R = sum(d[3] for d in desc)
    qct = R
    kct = qct + sum(d[0] for d in desc)
    qp = kct + sum(d[1] for d in desc)
    segs, off = [], 0
    for P, D, P2, n in desc:
        segs.append([(qct, P), (kct, D), (qp, P2), (off, n)])
        qct, kct, qp, off = qct + P, kct + D, qp + P2, off + n
    return segs, qp


INDEX_CASES = [[(1, 7)], [(1, 250)], [(10, 27)], [(1, 2, 1, 1)], [(1,)], [(10,)], [(1, 7), (1, 250)], [(1, 3)] * 40]
SIX = INDEX_CASES[:6]


def literal_index(segs):
    """[-2 | the bag's rows in sequence order | its first s^2 - L rows again] per bag, spelled with torch.cat."""
    out = []
    for bag in segs:
        rows = torch.cat([torch.arange(f, f + n) for f, n in bag])
        L = rows.numel()
        s = 1
        while s * s < L:
            s += 1
        out.append(torch.cat([torch.tensor([-2]), rows, rows[:s * s - L]]))
    return torch.cat(out).tolist()


def random_descriptions(count=200, seed=0):
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        bags = []
        for _ in range(rnd.randint(1, 3)):
            k = rnd.randint(1, 4)
            lens = [rnd.randint(0, 40) for _ in range(k)]
            if sum(lens) == 0:
                lens[rnd.randrange(k)] = rnd.randint(1, 40)
            bags.append(lens)
        # non-overlapping pieces anywhere in the source, in a shuffled memory order
        pieces = [(b, i) for b, lens in enumerate(bags) for i in range(len(lens))]
        rnd.shuffle(pieces)
        first, pos = {}, rnd.randint(0, 5)
        for b, i in pieces:
            first[(b, i)] = pos
            pos += bags[b][i] + rnd.randint(0, 3)
        out.append(([[(first[(b, i)], n) for i, n in enumerate(lens)] for b, lens in enumerate(bags)], pos + 1))
    return out


@pytest.mark.parametrize("desc", SIX, ids=str)
def test_host_index_equals_the_literal_concatenation(desc):
    from mil_amd.model.dim1.TransMIL import seq_index_segments
    segs, rows = bag_segments(desc)
    idx = seq_index_segments(segs, x_rows=rows)
    assert idx == literal_index(segs)
    assert all(-2 <= i < rows for i in idx)
    used = {i for i in idx if i >= 0}
    assert used == set(range(rows))                      # every row of x0 belongs to a bag


def test_host_index_known_values():
    from mil_amd.model.dim1.TransMIL import seq_index_segments
    # (1, 7): rows [7 patches | token 7]; s = 3, the one repeated row is the token
    assert seq_index_segments(bag_segments([(1, 7)])[0]) == [-2, 7, 0, 1, 2, 3, 4, 5, 6, 7]
    # (1, 2, 1, 1): rows [patch 0 | q_ct 1 | k_ct 2 3 | q_p 4]; s = 3, add = 4 crosses three borders
    assert seq_index_segments(bag_segments([(1, 2, 1, 1)])[0]) == [-2, 1, 2, 3, 4, 0, 1, 2, 3, 4]


def test_host_index_random_descriptions():
    from mil_amd.model.dim1.TransMIL import bucket_side, segment_table, seq_index_segments
    for segs, rows in random_descriptions():
        idx = seq_index_segments(segs, x_rows=rows)
        assert idx == literal_index(segs), segs
        assert all(i == -2 or 0 <= i < rows for i in idx), segs
        table, total = segment_table(segs)
        assert total == len(idx) and all(len(r) == 9 for r in table)
        assert [r[0] for r in table] == [bucket_side(sum(n for _, n in bag)) for bag in segs]


def test_host_index_never_leaves_the_source():
    """What the kernel does with a table that is not consistent: positions clamped into the bag, rows outside dropped."""
    from mil_amd.model.dim1.TransMIL import seq_index_segments
    assert seq_index_segments([[(0, 3)]], sides=[3], x_rows=3) == [-2, 0, 1, 2, 0, 1, 2, 2, 2, 2]     # L = 3 below (4, 9]
    assert seq_index_segments([[(0, 0)]], sides=[1], x_rows=3) == [-2, -1]
    assert seq_index_segments([[(2, 4)]], sides=[2], x_rows=4) == [-2, 2, 3, -1, -1]


def test_fusion_transmil_with_hip_graph_is_refused_before_any_gpu_work(monkeypatch):
    from mil_amd.config import create_arg_parser
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the flags must be refused before any GPU work"))
    argv = ["--variant", "fusion", "--aggregator", "TransMIL", "--synthetic", "[300, 768, 4]"]
    with pytest.raises(ValueError, match="fusion_transmil"):
        create_arg_parser([*argv, "--fusion_transmil", "1", "--hip_graph", "1"])
    assert create_arg_parser(argv).fusion_transmil == 0
    args = create_arg_parser([*argv, "--fusion_transmil", "1"])
    assert args.fusion_transmil == 1 and args.hip_graph == 0
