"""CPU: what the replayed TransMIL-aggregator step of the fusion model is keyed by and what its index kernel must write -
seq_index_bucket (model/dim1/TransMIL.py, the host mirror of csrc/transmil.hip: k_tm_seq_index_bucket) against
seq_index_segments on the pieces written out literally, the key count of the authors' bag lengths, the new switch with its
refusals, and the C-ABI entry."""
import ctypes
import os

import pytest

# (tail per bag in row order, cap, patch counts): L = N + sum(tail) sits at both ends of side 15 / 16, the repeats end inside
# a tail piece (add 3 < 8) or run through the tail into the patches (add 28 > 8)
BUCKET_CASES = [([1], 256, [200]), ([1], 256, [224]), ([1], 256, [196]), ([1], 256, [225]),
                ([1, 6, 1], 256, [214]), ([1, 6, 1], 256, [189]), ([1, 6, 1], 256, [217]), ([1, 6, 1], 256, [218]),
                ([1], 512, [200, 224]), ([1, 6, 1], 512, [189, 218])]
ADD = {200: 24, 224: 0, 196: 28, 225: 30, 214: 3, 189: 28, 217: 0, 218: 30}


def literal_pieces(lengths, cap, tail):
    """The issue's sentence, written out: per bag (cap + B sum_{k<j} tail_k + b tail_j, tail_j) for each j, then
    (sum_{a<b} len[a], len[b])."""
    B = len(lengths)
    segs = []
    for b in range(B):
        bag = [(cap + B * sum(tail[:j]) + b * tail[j], tail[j]) for j in range(len(tail))]
        bag.append((sum(lengths[:b]), lengths[b]))
        segs.append(bag)
    return segs, cap + B * sum(tail)


@pytest.mark.parametrize("tail,cap,lengths", BUCKET_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_mirror_equals_seq_index_segments_on_the_pieces(tail, cap, lengths):
    from mil_amd.model.dim1.TransMIL import bucket_segments, bucket_side, seq_index_bucket, seq_index_segments
    segs, rows = literal_pieces(lengths, cap, tail)
    assert bucket_segments(lengths, cap, tail) == (segs, rows)
    got = seq_index_bucket(lengths, cap, tail)
    assert got == seq_index_segments(segs, x_rows=rows)
    sides = [bucket_side(n + sum(tail)) for n in lengths]
    assert len(got) == sum(1 + s * s for s in sides)
    assert min(got) == -2 and got.count(-2) == len(lengths) and -1 not in got and max(got) < rows
    if len(lengths) == 1:
        n, t = lengths[0], sum(tail)
        s = sides[0]
        assert s * s - (n + t) == ADD[n]
        # upstream's order: the tail segments in row order, then the patches, then the first `add` rows of that again
        seq = list(range(cap, cap + t)) + list(range(n))
        assert got == [-2] + seq + seq[:ADD[n]]
    # explicit sides: a length that does not fit them is clamped, nothing leaves the source
    wrong = [s + 1 for s in sides]
    bad = seq_index_bucket(lengths, cap, tail, wrong)
    assert bad == seq_index_segments(segs, wrong, rows) and max(bad) < rows and min(bad) >= -2


def test_mirror_reads_a_length_as_the_kernel_does():
    from mil_amd.model.dim1.TransMIL import bucket_segments
    segs, rows = bucket_segments([-5, 10 ** 9], 256, [1])
    assert rows == 258 and segs[0][-1] == (0, 0) and segs[1][-1] == (0, 258)


def test_key_count_of_the_authors_bag_lengths_fits_the_default_cap():
    """One bag of N in [2000, 15 592] patches: (cap, side) pairs with tail 162 (P + D + P = 1 + 160 + 1) and tail 1."""
    from mil_amd.bags import bucket_rows
    from mil_amd.model.dim1.TransMIL import bucket_side
    from mil_amd.transmil_step import DEFAULT_MAX_GRAPHS
    counts = {}
    for tail in (162, 1):
        counts[tail] = len({(bucket_rows(n), bucket_side(n + tail)) for n in range(2000, 15593)})
    assert counts == {162: 86, 1: 87}
    assert max(counts.values()) <= DEFAULT_MAX_GRAPHS


BASE = ["--variant", "fusion", "--aggregator", "TransMIL", "--fusion_transmil", "1", "--synthetic", "[300, 768, 6]"]


def test_switch_exists_and_defaults_off():
    from mil_amd.config import create_arg_parser
    assert create_arg_parser(BASE).fusion_transmil_graph == 0
    assert create_arg_parser(BASE + ["--fusion_transmil_graph", "1"]).fusion_transmil_graph == 1
    a = create_arg_parser(BASE + ["--fusion_transmil_graph", "1", "--modality", "['CT','pathology']"])
    assert a.fusion_transmil_graph == 1 and a.modality == ["CT", "pathology"]


@pytest.mark.parametrize("argv,match", [
    (["--variant", "fusion", "--aggregator", "TransMIL", "--fusion_transmil_graph", "1"], "fusion_transmil 1"),
    (["--variant", "fusion", "--aggregator", "ABMIL", "--fusion_transmil", "1", "--fusion_transmil_graph", "1"], "aggregator TransMIL"),
    (["--variant", "image_only", "--model_pathology", "TransMIL", "--fusion_transmil_graph", "1"], "variant fusion"),
    (BASE + ["--fusion_transmil_graph", "1", "--flat_adam", "0"], "flat_adam 1"),
    (BASE + ["--fusion_transmil_graph", "1", "--hip_graph", "1"], "hip_graph"),
    (BASE + ["--fusion_transmil_graph", "1", "--learnablePrompt", "1"], "learnablePrompt"),
    (BASE + ["--fusion_transmil_graph", "1", "--modality", "['CI']"], "modality"),
    (BASE + ["--fusion_transmil_graph", "1", "--save_note_attn", "somewhere"], "save_note_attn"),
])
def test_switch_is_refused_outside_its_model(argv, match):
    from mil_amd.config import create_arg_parser
    with pytest.raises(ValueError, match=match):
        create_arg_parser(argv)


def test_the_old_refusal_still_stands():
    from mil_amd.config import create_arg_parser
    with pytest.raises(ValueError, match="hip_graph"):
        create_arg_parser(BASE + ["--hip_graph", "1"])


def test_abi_declares_and_exports_the_bucket_index_entry():
    from mil_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    name = "mil_tm_seq_index_bucket"
    assert name in _lib.header_symbols() and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == 11
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, name)
    handle.mil_abi_version.restype = ctypes.c_int
    assert _lib.ABI_VERSION >= 18 and handle.mil_abi_version() == _lib.ABI_VERSION


def test_stepper_imports_without_a_gpu():
    from mil_amd import ops
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1.TransMIL import BucketGeometry
    assert callable(RaggedFusionTransMILStepper) and callable(BucketGeometry) and callable(ops.tm_seq_index_bucket)
