"""GPU: the fused landmark-query pass (csrc/landmark_attn.hip, opt-in: nystrom_core(fused_a3=True) / MIL_TM_FUSED_A3=1).
The two entries through the raw C ABI against the float64 restatement of tests/landmark_attn_ref.py, block by block, inside
sentinel buffers; bit-equal repeats; nystrom_core with the route on beside the materialised route against
transmil_ref.core_run; the TransMIL module and a replayed step against the reference's goldens; and the peak memory the route
gives back.  Bounds: k x max(e32, 1e-7) per block with k = landmark_attn_ref.K_LMK (the measured ratios: docs/lab_notes.md),
the module's standing 1e-4 / 2e-3 where the goldens are the reference."""
import pytest
import torch

import landmark_attn_ref as LR
import transmil_ref as R
from fused_attn_common import DEV, MAP_BYTES, SENT, _bits, _check_grads, _core, _guarded, _guards_intact, _lib, _model, _p, _st, rel
from test_transmil_host import golden_bags

pytestmark = pytest.mark.gpu


_refs = {}


def _ref(name, n_pad):
    key = (name, n_pad)
    if key not in _refs:
        qkv, qL, dW, pad = LR.case(name, n_pad)
        _refs[key] = (LR.run(qkv, qL, dW), LR.run(qkv, qL, dW, torch.float32), LR.blocks(n_pad, pad))
    return _refs[key]


def _run_abi(name, n_pad):
    """Forward, then backward from the forward's own W and lse, every buffer between sentinels; returns the four results (CPU)
    after the sentinel checks."""
    lib = _lib()
    qkv, qL, dW, _ = LR.case(name, n_pad)
    n = n_pad * 1536
    qbuf, qv = _guarded(n, qkv)
    qlbuf, qlv = _guarded(8 * 256 * 64, qL)
    dwbuf, dwv = _guarded(8 * 256 * 64, dW)
    wbuf, wv = _guarded(8 * 256 * 64)
    lbuf, lv = _guarded(8 * 256)
    dqlbuf, dqlv = _guarded(8 * 256 * 64)
    dqbuf, dqv = _guarded(n)
    wsf, wsb = lib.mil_tm_lmk_attn_ws_floats(n_pad, 0), lib.mil_tm_lmk_attn_ws_floats(n_pad, 1)
    assert 0 < wsf and 0 < wsb and (n_pad < 512 or max(wsf, wsb) < 8 * 256 * n_pad)
    fbuf, fv = _guarded(wsf)
    bbuf, bv = _guarded(wsb)
    inputs = {"qkv": (qbuf, _bits(qbuf)), "qL": (qlbuf, _bits(qlbuf)), "dW": (dwbuf, _bits(dwbuf))}
    rc = lib.mil_tm_lmk_attn_fwd(_p(qv), _p(qlv), n_pad, _p(wv), _p(lv), _p(fv), _st())
    assert rc == 0, (name, n_pad, rc)
    rc = lib.mil_tm_lmk_attn_bwd(_p(qv), _p(qlv), _p(wv), _p(lv), _p(dwv), n_pad, _p(dqv), _p(dqlv), _p(bv), _st())
    assert rc == 0, (name, n_pad, rc)
    torch.cuda.synchronize()
    for tag, buf in (("W", wbuf), ("lse", lbuf), ("dqL", dqlbuf), ("dqkv", dqbuf), ("ws fwd", fbuf), ("ws bwd", bbuf)):
        _guards_intact(f"{name} {n_pad} {tag}", buf)
    for tag, (buf, before) in inputs.items():
        assert torch.equal(_bits(buf), before), f"{name} {n_pad}: input {tag} changed"
    sent = int(torch.tensor([SENT], dtype=torch.float32).view(torch.int32))
    dqkv = dqv.reshape(n_pad, 1536).cpu()
    assert bool((_bits(dqkv[:, :512]) == sent).all()), f"{name} {n_pad}: columns 0 .. 511 of dqkv were written"
    assert not bool((_bits(dqkv[:, 512:]) == sent).any()), f"{name} {n_pad}: an element of columns 512 .. 1535 was not written"
    for tag, v in (("W", wv), ("lse", lv), ("dqL", dqlv)):
        assert not bool((_bits(v) == sent).any()), f"{name} {n_pad}: an element of {tag} was not written"
    return {"W": wv.reshape(8, 256, 64).cpu(), "lse": lv.reshape(8, 256).cpu(), "dkv": dqkv[:, 512:].contiguous(),
            "dqL": dqlv.reshape(8, 256, 64).cpu()}


@pytest.mark.parametrize("n_pad", LR.SIZES)
@pytest.mark.parametrize("name", LR.CASES)
def test_entries_against_float64(name, n_pad):
    """W, lse, dk | dv, dqL per block: all heads and each, the k and v groups over all rows, the pad rows, the first and last
    16 rows and every 256-row chunk.  `hot` has max|S| = 110: exp without the running maximum overflows float32."""
    got = _run_abi(name, n_pad)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    ref, r32, blks = _ref(name, n_pad)
    LR.hold("stage", f"{name} n_pad {n_pad}", got, ref, r32, blks)


def test_two_runs_give_the_same_bits():
    a, b = _run_abi("ramp_up", 1280), _run_abi("ramp_up", 1280)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("n_pad,peak", [(256, 1.0), (512, 1.0), (256, R.PEAK), (512, R.PEAK)])
def test_nystrom_core_with_the_route_on(n_pad, peak):
    """Both routes against the float64 core on the same inputs, over transmil_ref.core_blocks; they need not agree bit for bit."""
    qkv, w, dO, pad = R.core_case(n_pad, peak)
    ref, r32, blks = R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32), R.core_blocks(n_pad, pad)
    for fused in (False, True):
        got, attn = _core(qkv, w, dO, fused_a3=fused)
        assert attn is None and bool(torch.isfinite(got["dqkv"]).all())
        LR.hold("core", f"n_pad {n_pad} peak {peak} fused_a3 {fused}", got, ref, r32, blks)


def test_attention_outputs_keep_the_materialised_route(monkeypatch):
    """need_attn "cls" and True read the map: with the switch on (keyword or environment) the forward gives the bits of the
    switch off (at this size its split-K products have two addends, so they are reproducible)."""
    geo = R.geometry(250)                                                 # n_pad 512, s 16, pad 255
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn((geo["n_pad"], 1536), generator=g, dtype=torch.float64)
    qkv[:geo["pad"]] = 0
    w = (torch.rand((R.H, 1, R.CONV, 1), generator=g, dtype=torch.float64) * 2 - 1) / R.CONV ** 0.5
    dO = torch.randn((geo["n_pad"], 512), generator=g, dtype=torch.float64)
    cls = dict(need_attn="cls", pad=geo["pad"], s=geo["s"], n=250)
    monkeypatch.delenv("MIL_TM_FUSED_A3", raising=False)
    off, a_off = _core(qkv, w, dO, fused_a3=False, **cls)
    on, a_on = _core(qkv, w, dO, fused_a3=True, **cls)
    monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    env, a_env = _core(qkv, w, dO, **cls)
    assert a_off.shape == (8, 256)
    for got, attn in ((on, a_on), (env, a_env)):
        assert torch.equal(_bits(attn), _bits(a_off))
        assert torch.equal(_bits(got["out"]), _bits(off["out"]))
        assert rel(got["dqkv"], off["dqkv"]) < 1e-5      # the same launches; their split-K sums add atomically, in any order
    with torch.no_grad():
        from mil_amd import ops
        qd, wd = qkv.float().to(DEV), w.float().to(DEV)
        m_off = ops.nystrom_core(qd, wd, True, fused_a3=False)[1]
        m_on = ops.nystrom_core(qd, wd, True)[1]                          # the environment says 1
    assert m_on.shape == (8, 512, 512) and torch.equal(_bits(m_on), _bits(m_off))


def _count_fused_calls(monkeypatch):
    """Counts the calls of the fused forward that _tm_fwd makes: the switch has to reach the kernels."""
    from mil_amd.ops import transmil as T
    calls, inner = [], T.tm_lmk_attn
    monkeypatch.setattr(T, "tm_lmk_attn", lambda *a: (calls.append(1), inner(*a))[1])
    return calls


@pytest.mark.parametrize("tag", ["transmil_N7", "transmil_N250", "transmil_N1000"])
def test_module_eval_against_reference_goldens_with_the_switch_on(tag, golden, monkeypatch):
    """test_gpu_transmil.py::test_module_eval_against_reference_goldens with MIL_TM_FUSED_A3=1: fwd + BCE + bwd against
    tests/golden/transmil_*.npz on the module's standing bounds."""
    from mil_amd import synthetic as syn
    monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    calls = _count_fused_calls(monkeypatch)
    g = golden(tag)
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    model = _model(seed)
    x = torch.cat([torch.randn((n, 768), generator=torch.Generator().manual_seed(seed + 100 + i), dtype=torch.float64)
                   for i, n in enumerate(lengths)], 0).float().to(DEV).requires_grad_(True)
    y = syn.make_labels(seed + 7, len(lengths), 2).to(DEV)
    h, prob = model([x], lengths)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    assert len(calls) == 2 * len(lengths)                                 # two TransLayers per bag
    err = {"h": rel(h, g["h"]), "logits": rel(model.last_logits, g["logits"]),
           "loss": abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))}
    assert err["h"] <= 1e-4 and err["logits"] <= 1e-4 and err["loss"] <= 1e-4, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    worst = _check_grads(model, g, {"dx": x.grad})
    print(f"golden {tag} fused_a3: h {err['h']:.2e} logits {err['logits']:.2e} loss {err['loss']:.2e} worst grad {worst:.2e}")


def test_replay_with_the_switch_on_matches_the_reference_goldens(golden, monkeypatch):
    """test_gpu_transmil_graph.py::test_replay_on_another_length_of_the_side_matches_the_reference_goldens with the switch on:
    the graph of side 32 is captured on N = 990 and replayed on the golden bag of N = 1000."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    monkeypatch.setenv("MIL_TM_FUSED_A3", "1")
    calls = _count_fused_calls(monkeypatch)
    g = golden("transmil_N1000")
    seed, lengths = int(g["seed"]), [int(v) for v in g["lengths"]]
    model = _model(seed)
    st = RaggedTransMILStepper(model, None, B=1, backward=True)
    y = syn.make_labels(seed + 7, 1, 2).to(DEV)
    for i, n in enumerate([990, 990]):
        slot = st.slot([n])
        slot.x[:n].copy_(torch.randn((n, 768), generator=torch.Generator().manual_seed(50 + i)).to(DEV))
        slot.y.copy_(y)
        st.step(slot, [n])
    assert st.n_graphs == 1 and st.replays == 1 and st.eager_steps == 1
    assert len(calls) >= 4                                                # the eager step and the captured one, two layers each
    N = lengths[0]
    assert st.slot([N]) is slot
    slot.x[:N].copy_(golden_bags(seed, lengths)[0].float().to(DEV))
    slot.y.copy_(y)
    loss, prob = st.step(slot, [N])
    assert st.replays == 2 and st.eager_steps == 1 and st.n_graphs == 1
    value = st.read_loss(loss)
    err = {"h": rel(slot.last["h"], g["h"]), "logits": rel(slot.last["logits"], g["logits"]),
           "loss": abs(value - float(g["loss"])) / abs(float(g["loss"]))}
    print(f"replayed golden transmil_N1000 fused_a3: {err}")
    assert err["h"] <= 1e-4 and err["logits"] <= 1e-4 and err["loss"] <= 1e-4, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    print(f"replayed golden transmil_N1000 fused_a3: worst grad {_check_grads(model, g):.2e}")


def test_the_route_gives_back_a_map_of_peak_memory():
    """nystrom_core forward + backward at n_pad = 2048: the materialised route holds A3 and dA3 at the backward's peak, the
    fused one neither and a workspace below one map, so its peak is lower by at least one map (8 x 256 x 2048 floats)."""
    n_pad = 2048
    qkv, w, dO, _ = R.core_case(n_pad)
    peak = {}
    for fused in (False, True, False):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _core(qkv, w, dO, fused_a3=fused)
        peak.setdefault(fused, []).append(torch.cuda.max_memory_allocated() - base)
    print(f"PEAK | n_pad {n_pad} | materialised {peak[False]} | fused {peak[True]} | one map {MAP_BYTES * n_pad}")
    assert min(peak[False]) - peak[True][0] >= MAP_BYTES * n_pad, peak
