"""CPU: what the bounds of tests/test_gpu_landmark_attn.py see.  Each planted error of landmark_attn_ref breaks bound(e32, 16)
of at least one block by more than 10 x; the formulas the kernels implement are the stage's autograd gradients; and the
float32 restatement evaluated chunk by chunk - 256-key chunks, a running maximum and sum, rescaled at every chunk - stays
within 2 x max(e32, 1e-7) of float64, so the chunking itself costs nothing a bound has to absorb."""
import pytest
import torch

import landmark_attn_ref as LR
import transmil_ref as R

_runs = {}


def _ref(name, n_pad):
    """(float64 reference, float32 restatement, blocks) of a case, computed once."""
    key = (name, n_pad)
    if key not in _runs:
        qkv, qL, dW, pad = LR.case(name, n_pad)
        _runs[key] = (LR.run(qkv, qL, dW), LR.run(qkv, qL, dW, torch.float32), LR.blocks(n_pad, pad))
    return _runs[key]


@pytest.mark.parametrize("n_pad", [512, 1280])
@pytest.mark.parametrize("name", ["randn", "ramp_up"])
def test_formulas_are_the_autograd_gradients(name, n_pad):
    qkv, qL, dW, pad = LR.case(name, n_pad)
    ref, _, blks = _ref(name, n_pad)
    for chunked in (False, True):
        got = LR.run_formulas(qkv, qL, dW, pad=pad, chunked=chunked)
        worst = max(R.flat_err(got, ref, blks).values())
        assert worst < 1e-12, (chunked, worst)


@pytest.mark.parametrize("n_pad", [512, 1280])
@pytest.mark.parametrize("name", ["randn", "ramp_up"])
@pytest.mark.parametrize("mutate", LR.MUTATIONS)
def test_each_planted_error_breaks_a_bound_by_ten(mutate, name, n_pad):
    qkv, qL, dW, pad = LR.case(name, n_pad)
    ref, r32, blks = _ref(name, n_pad)
    bad = LR.run_formulas(qkv, qL, dW, pad=pad, mutate=mutate)
    e32, eb = R.flat_err(r32, ref, blks), R.flat_err(bad, ref, blks)
    excess = {b: e / R.bound(e32[b], R.K_CAP) for b, e in eb.items()}
    top = max(excess, key=excess.get)
    print(f"EXCESS | {mutate} | {name} | n_pad {n_pad} | {top} | {excess[top]:.1f}")
    assert excess[top] > 10.0, (mutate, name, n_pad, top, excess[top])


def test_most_ramp_up_rows_peak_in_the_last_chunk():
    """What makes ramp_up a test of the rescaling: the running maximum moves in the last chunk for most rows."""
    qkv, qL, _, _ = LR.case("ramp_up", 512)
    arg = LR.scores(qkv, qL).argmax(-1)
    assert int((arg >= 256).sum()) > 0.75 * arg.numel()


@pytest.mark.parametrize("n_pad", [512, 1280])
@pytest.mark.parametrize("name", LR.CASES)
def test_chunked_float32_costs_no_more_than_float32(name, n_pad):
    """The float32 restatement with its forward evaluated in 256-key chunks (landmark_attn_ref.online) against float64, per
    block.  Printed beside it, not asserted: the same figure with the backward through the kernels' formulas as well (saved
    lse, delta from W), whose float64 form the test above pins to autograd - in float32 P = exp(S - lse) carries the rounding
    of an lse of size 10 on top of that of S; single blocks read up to 1.9 x e32 here and 2.3 x at n_pad = 768
    (docs/lab_notes.md)."""
    qkv, qL, dW, pad = LR.case(name, n_pad)
    ref, r32, blks = _ref(name, n_pad)
    rat = LR.ratios(LR.run(qkv, qL, dW, torch.float32, chunked=True), ref, r32, blks)
    top = max(rat, key=lambda b: rat[b][2])
    rf = LR.ratios(LR.run_formulas(qkv, qL, dW, torch.float32, pad=pad, chunked=True), ref, r32, blks)
    tf = max(rf, key=lambda b: rf[b][2])
    print(f"CHUNKED | {name} | n_pad {n_pad} | {top} | {rat[top][2]:.2f} | formulas | {tf} | {rf[tf][2]:.2f}")
    bad = [(b, e, e32) for b, (e, e32, _) in rat.items() if not e <= R.bound(e32, 2)]
    assert not bad, (name, n_pad, bad)
