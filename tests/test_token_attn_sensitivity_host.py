"""CPU: what the bounds of tests/test_gpu_token_attn.py see.  The formulas the kernels implement (plain, and with the two sums
over the rows formed as one partial per 256-row chunk) are the stage's autograd gradients in float64; and each planted error of
token_attn_ref breaks bound(e32, 16) of at least one block by more than 10 x, on every case at two and at five row chunks."""
import pytest
import torch

import token_attn_ref as TR
import transmil_ref as R

_runs = {}


def _ref(name, n_pad):
    """(float64 reference, float32 restatement, blocks) of a case, computed once."""
    key = (name, n_pad)
    if key not in _runs:
        qkv, kL, U, dO, pad = TR.case(name, n_pad)
        _runs[key] = (TR.run(qkv, kL, U, dO), TR.run(qkv, kL, U, dO, torch.float32), TR.blocks(n_pad, pad))
    return _runs[key]


@pytest.mark.parametrize("n_pad", [512, 1280])
@pytest.mark.parametrize("name", TR.CASES)
def test_formulas_are_the_autograd_gradients(name, n_pad):
    qkv, kL, U, dO, pad = TR.case(name, n_pad)
    ref, _, blks = _ref(name, n_pad)
    for chunked in (False, True):
        got = TR.run_formulas(qkv, kL, U, dO, pad=pad, chunked=chunked)
        worst = max(R.flat_err(got, ref, blks).values())
        assert worst <= 1e-10, (chunked, worst)


@pytest.mark.parametrize("n_pad", [512, 1280])
@pytest.mark.parametrize("name", TR.CASES)
@pytest.mark.parametrize("mutate", TR.MUTATIONS)
def test_each_planted_error_breaks_a_bound_by_ten(mutate, name, n_pad):
    qkv, kL, U, dO, pad = TR.case(name, n_pad)
    ref, r32, blks = _ref(name, n_pad)
    bad = TR.run_formulas(qkv, kL, U, dO, pad=pad, mutate=mutate)
    e32, eb = R.flat_err(r32, ref, blks), R.flat_err(bad, ref, blks)
    excess = {b: e / R.bound(e32[b], R.K_CAP) for b, e in eb.items()}
    top = max(excess, key=excess.get)
    print(f"EXCESS | {mutate} | {name} | n_pad {n_pad} | {top} | {excess[top]:.1f}")
    assert excess[top] > 10.0, (mutate, name, n_pad, top, excess[top])


def test_the_ramps_make_the_chunks_partials_differ():
    """What makes ramp_up / ramp_down a test of the reduce: the chunks' dkL partials differ in size by more than 2 x end to end,
    so a lost or doubled chunk cannot hide."""
    for name in ("ramp_up", "ramp_down"):
        qkv, kL, U, dO, pad = TR.case(name, 1280)
        full = TR.run_formulas(qkv, kL, U, dO, pad=pad)["dkL"]
        last = TR.run_formulas(qkv, kL, U, dO, pad=pad, mutate="dkL_last")["dkL"]
        share = float(last.norm() / full.norm())
        assert (share > 0.5) if name == "ramp_up" else (share < 0.2), (name, share)


def test_hot_overflows_without_the_maximum():
    """The hot case is one: exp(S) without the row maximum is not finite in float32."""
    qkv, kL, _, _, _ = TR.case("hot", 512)
    S = TR.scores(qkv, kL).float()
    assert not bool(torch.isfinite(S.exp().sum(-1)).all())
    assert bool(torch.isfinite((S - S.amax(-1, keepdim=True)).exp().sum(-1)).all())
