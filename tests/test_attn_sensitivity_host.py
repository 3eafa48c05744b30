"""CPU: what the per-block bounds of tests/test_gpu_attn_stages.py can see.

The GPU bound of a block is k x max(e32, 1e-7), k <= 16, with e32 the error of the float32 restatement of the same stage
on the CPU against float64 (tests/attn_ref.py).  For every case of the GPU file, with its own inputs and blocks:
  a. every block has a non-zero reference, except those that are zero by construction (attn_ref.expected_zero);
  b. every planted error that applies to the case (mutate= of the restatement), measured in float64 against the clean
     float64 result, exceeds the bound at the cap k = 16 by a factor of 10 on at least one block;
  c. the float32 restatement is finite on every block.
pytest -s lists the achieved margins.  Nothing here reads the code under test."""
import math

import pytest
import torch

import attn_ref as A

MARGIN = 10.0


def margin(mut, ref, r32, blocks):
    blocks = {t: blocks[t] for t in mut}
    e32, em = A.flat_err(r32, ref, blocks), A.flat_err(mut, ref, blocks)
    best = max(em, key=lambda b: em[b] / A.bound(e32[b], A.K_CAP))
    return em[best] / A.bound(e32[best], A.K_CAP), best, em[best], e32[best]


def caught(case, planted, ref, r32, blocks):
    for name, mut in planted.items():
        m, blk, em, e32 = margin(mut, ref, r32, blocks)
        print(f"planted {name:<12} case {case:<28} margin {m:9.1f}x on {blk:<18} (error {em:.1e}, e32 {e32:.1e})")
        assert m >= MARGIN, (case, name, m, blk)


def teeth(case, c, ref, r32, blocks):
    """(a) and (c) for the attention forms."""
    for t in blocks:
        for name, ix in blocks[t].items():
            r = ref[t][ix]
            if r.numel() == 0:
                continue
            top = float(r.abs().max())
            if t != "lse" and A.expected_zero(c, t, name):
                assert top == 0.0, (case, t, name, top)
            else:
                assert top > 0.0 and math.isfinite(top), (case, t, name, top)
    e32 = A.flat_err(r32, ref, blocks)
    assert all(math.isfinite(e) and e <= A.bound(e, 1) for e in e32.values()), case
    print(f"case {case:<28} {len(e32)} blocks, worst e32 {max(e32.values()):.1e}")
    return e32


def attn_planted(c, causal, fwd_muts, bwd_muts, tag, exact=False):
    ref_f, r32_f = A.fwd_run(c, causal=causal), A.fwd_run(c, torch.float32, causal=causal)
    fb, bb = A.fwd_blocks(c), A.bwd_blocks(c, causal, exact)
    teeth(tag + " fwd", c, ref_f, r32_f, fb)
    caught(tag + " fwd", {m: A.fwd_run(c, causal=causal, mutate=m) for m in fwd_muts}, ref_f, r32_f, fb)
    if bwd_muts is None:
        return
    ref_b = A.bwd_run(c, causal=causal)
    r32_b = A.bwd_run(c, torch.float32, causal=causal, fwd=ref_f)
    teeth(tag + " bwd", c, ref_b, r32_b, bb)
    caught(tag + " bwd", {m: A.bwd_run(c, causal=causal, mutate=m, fwd=ref_f) for m in bwd_muts}, ref_b, r32_b, bb)
    if not exact:
        # the blocks that are zero by cancellation: the float32 restatement leaves noise below the bound; a lost D term in
        # the first row of a causal sequence is far above it (for a one-key bag the restatement states the zero outright)
        for name, rel in A.cancel_noise(c, r32_b, causal).items():
            print(f"case {tag:<28} {name}: noise / cancelling terms {rel:.1e} in float32 (bound {A.noise_bound(c['C']):.1e})")
            assert rel <= A.noise_bound(c["C"]), (tag, name, rel)
        lost = A.cancel_noise(c, A.bwd_run(c, causal=causal, mutate="nodelta", fwd=ref_f), causal)
        one = [f"bag{b}" for b in A.one_key_bags(c)]
        assert all(rel >= MARGIN * A.noise_bound(c["C"]) for n, rel in lost.items() if n.split(".")[1] not in one), (tag, lost)


@pytest.mark.parametrize("C", [32, 64])
def test_rows_form(C):
    """Keys <= 16 per bag: no 64-key tile to lose; the forward of the launch with the empty bag, the backward without it."""
    attn_planted(A.attn_case(A.ROWS_BAGS, C), False, ("head",), None, f"rows C{C}")
    attn_planted(A.attn_case(A.ROWS_BWD_BAGS, C), False, ("head",), ("nodelta", "noscale", "head"), f"rows-bwd C{C}", exact=True)
    c = A.attn_case([(n, n) for n in A.CAUSAL_LENS], C, seed=1)
    attn_planted(c, True, ("causal_off1", "head"), None, f"rows causal C{C}")


@pytest.mark.parametrize("C", [32, 64])
def test_general_backward(C):
    attn_planted(A.attn_case(A.GEN_BAGS, C), False, ("lasttile", "head"), ("nodelta", "lasttile", "noscale", "head"), f"gen C{C}")


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("name", ["ragged", "single", "peaked"])
def test_pool_form(name, C):
    bags = {"ragged": A.POOL_RAGGED, "single": A.POOL_SINGLE, "peaked": A.POOL_PEAKED}[name]
    c = A.attn_case(bags, C, peaked=name == "peaked")
    attn_planted(c, False, ("lasttile", "head"), ("nodelta", "lasttile", "noscale", "head"), f"pool {name} C{C}")


@pytest.mark.parametrize("C", [32, 64])
def test_peaked_pool_case_is_what_it_says(C):
    """First query of every bag: scores near +80 on even heads and -80 on odd ones, the largest in tile (64 h + 13) mod n
    / 64 - so the merge of k_attn_pool_merge has its maximum in another tile per head."""
    c = A.attn_case(A.POOL_PEAKED, C, peaked=True)
    for b, (_, n) in enumerate(A.POOL_PEAKED):
        q0 = c["q"][c["q_off"][b]].reshape(A.H, C)
        k = c["k"][c["k_off"][b]:c["k_off"][b + 1]].reshape(n, A.H, C)
        s = torch.einsum("hc,nhc->hn", q0, k) / math.sqrt(C)
        for h in range(A.H):
            sign = 1 if h % 2 == 0 else -1
            assert abs(float(s[h].median()) - sign * A.PEAK_SHIFT) < 8, (b, h, float(s[h].median()))
            assert int(s[h].argmax()) // A.TILE == ((A.TILE * h + 13) % n) // A.TILE, (b, h)
    tiles = {((A.TILE * h + 13) % 200) // A.TILE for h in range(A.H)}
    assert len(tiles) == 4


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("causal", [False, True])
def test_seq_form(causal, C):
    c = A.seq_case(A.SEQ_LENS, C)
    extra = ("causal_off1",) if causal else ()
    attn_planted(c, causal, ("lasttile", "head") + extra, ("nodelta", "lasttile", "noscale", "head") + extra,
                 f"seq {'causal' if causal else 'full'} C{C}")


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("lens", [A.ABS_BAGS, A.ABS_SINGLE], ids=["ragged", "single"])
def test_absorbed_path(lens, C):
    c = A.absorbed_case(lens, C)
    tag = f"absorbed {len(lens)} bags C{C}"
    ref = A.absorbed_ref(c)
    r32 = A.absorbed(c, torch.float32, given=ref)
    blocks = A.absorbed_blocks(c)
    # the two forms are the same function: absorbed float64 = unabsorbed float64 far below any float32 bound
    both = A.flat_err(A.absorbed(c), ref, blocks)
    assert max(both.values()) < 1e-11, max(both, key=both.get)
    for t in blocks:
        for name, ix in blocks[t].items():
            top = float(ref[t][ix].abs().max())
            assert top > 0.0 and math.isfinite(top), (tag, t, name)
    e32 = A.flat_err(r32, ref, blocks)
    assert all(math.isfinite(e) for e in e32.values())
    print(f"case {tag:<28} {len(e32)} blocks, worst e32 {max(e32.values()):.1e}")
    # without the addend the keys' gradient is another tensor: both are references of the GPU test
    assert float((A.absorbed_ref(c, acc=False)["dkeys"] + c["dkeys_acc"] - ref["dkeys"]).abs().max()) < 1e-12
    caught(tag, {m: A.absorbed(c, given=ref, mutate=m) for m in A.ABSORBED_MUTATIONS}, ref, r32, blocks)
    # the one-key bag: dQp is rounding noise of the two terms that cancel, a few 1e-7 of them in float32
    for b, rel in A.onekey_noise(c, ref, r32).items():
        print(f"case {tag:<28} one-key bag {b}: |dQp| / cancelling terms {rel:.1e} in float32")
        assert rel < 16 * 2.0 ** -23 * math.sqrt(A.E)
