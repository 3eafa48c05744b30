"""GPU: the fused token-query pass (csrc/token_attn.hip, opt-in: nystrom_core(fused_a1=True) / MIL_TM_FUSED_A1=1).
The two entries through the raw C ABI against the float64 restatement of tests/token_attn_ref.py, block by block, inside
sentinel buffers; bit-equal repeats; nystrom_core with the route on and off, beside both settings of the landmark-query switch,
against transmil_ref.core_run; the switch off and the attention outputs on the launches of before; the TransMIL module and a
replayed step against the reference's goldens; and the peak memory the route gives back.  Bounds: k x max(e32, 1e-7) per block
with k = token_attn_ref.K_TOK (the measured ratios: docs/lab_notes.md), the module's standing 1e-4 / 2e-3 where the goldens are
the reference."""
import pytest
import torch

import token_attn_ref as TR
import transmil_ref as R
from fused_attn_common import DEV, MAP_BYTES, SENT, _bits, _check_grads, _core, _guarded, _guards_intact, _lib, _model, _p, _st, rel
from test_transmil_host import golden_bags

pytestmark = pytest.mark.gpu


_refs = {}


def _ref(name, n_pad):
    key = (name, n_pad)
    if key not in _refs:
        qkv, kL, U, dO, pad = TR.case(name, n_pad)
        _refs[key] = (TR.run(qkv, kL, U, dO), TR.run(qkv, kL, U, dO, torch.float32), TR.blocks(n_pad, pad))
    return _refs[key]


def _run_abi(name, n_pad):
    """Forward, then backward from the forward's own lse, every buffer between sentinels; returns the five results (CPU) after
    the sentinel checks."""
    lib = _lib()
    qkv, kL, U, dO, _ = TR.case(name, n_pad)
    n, small = n_pad * 1536, 8 * 256 * 64
    qbuf, qv = _guarded(n, qkv)
    kbuf, kv = _guarded(small, kL)
    ubuf, uv = _guarded(small, U)
    dobuf, dov = _guarded(n_pad * 512, dO)
    obuf, ov = _guarded(n_pad * 512)
    lbuf, lv = _guarded(8 * n_pad)
    dqbuf, dqv = _guarded(n)
    dubuf, duv = _guarded(small)
    dkbuf, dkv = _guarded(small)
    wsf, wsb = lib.mil_tm_tok_attn_ws_floats(n_pad, 0), lib.mil_tm_tok_attn_ws_floats(n_pad, 1)
    assert 0 <= wsf and 0 < wsb and (n_pad < 512 or max(wsf, wsb) < 8 * 256 * n_pad)
    fbuf, fv = _guarded(wsf)
    bbuf, bv = _guarded(wsb)
    inputs = {"qkv": (qbuf, _bits(qbuf)), "kL": (kbuf, _bits(kbuf)), "U": (ubuf, _bits(ubuf)), "dO": (dobuf, _bits(dobuf))}
    rc = lib.mil_tm_tok_attn_fwd(_p(qv), _p(kv), _p(uv), n_pad, _p(ov), _p(lv), _p(fv) if wsf else None, _st())
    assert rc == 0, (name, n_pad, rc)
    rc = lib.mil_tm_tok_attn_bwd(_p(qv), _p(kv), _p(uv), _p(lv), _p(dov), n_pad, _p(dqv), _p(duv), _p(dkv), _p(bv), _st())
    assert rc == 0, (name, n_pad, rc)
    torch.cuda.synchronize()
    for tag, buf in (("O", obuf), ("lse", lbuf), ("dqkv", dqbuf), ("dU", dubuf), ("dkL", dkbuf), ("ws fwd", fbuf), ("ws bwd", bbuf)):
        _guards_intact(f"{name} {n_pad} {tag}", buf)
    for tag, (buf, before) in inputs.items():
        assert torch.equal(_bits(buf), before), f"{name} {n_pad}: input {tag} changed"
    sent = int(torch.tensor([SENT], dtype=torch.float32).view(torch.int32))
    dqkv = dqv.reshape(n_pad, 1536).cpu()
    assert bool((_bits(dqkv[:, 512:]) == sent).all()), f"{name} {n_pad}: columns 512 .. 1535 of dqkv were written"
    assert not bool((_bits(dqkv[:, :512]) == sent).any()), f"{name} {n_pad}: an element of columns 0 .. 511 was not written"
    for tag, v in (("O", ov), ("lse", lv), ("dU", duv), ("dkL", dkv)):
        assert not bool((_bits(v) == sent).any()), f"{name} {n_pad}: an element of {tag} was not written"
    return {"O": ov.reshape(n_pad, 512).cpu(), "lse": lv.reshape(8, n_pad).cpu(), "dq": dqkv[:, :512].contiguous(),
            "dU": duv.reshape(8, 256, 64).cpu(), "dkL": dkv.reshape(8, 256, 64).cpu()}


@pytest.mark.parametrize("n_pad", TR.SIZES)
@pytest.mark.parametrize("name", TR.CASES)
def test_entries_against_float64(name, n_pad):
    """O, lse, dq, dU, dkL per block: O and dq over all rows, the pad rows, the first and last 16 rows and every 256-row chunk,
    the others over all heads and each.  dO is nonzero on the pad rows: a kernel that skips them shows in dU.  `hot` has
    max|S| = 110: exp without the row maximum overflows float32."""
    got = _run_abi(name, n_pad)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    ref, r32, blks = _ref(name, n_pad)
    TR.hold("stage", f"{name} n_pad {n_pad}", got, ref, r32, blks)


def test_two_runs_give_the_same_bits():
    a, b = _run_abi("ramp_up", 1280), _run_abi("ramp_up", 1280)
    assert set(a) == {"O", "lse", "dq", "dU", "dkL"}
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def _count_fused_calls(monkeypatch):
    """Counts the calls of the fused forward that _tm_fwd makes: the switch has to reach the kernels."""
    from mil_amd.ops import transmil as T
    calls, inner = [], T.tm_tok_attn
    monkeypatch.setattr(T, "tm_tok_attn", lambda *a: (calls.append(1), inner(*a))[1])
    return calls


@pytest.mark.parametrize("n_pad,peak", [(256, 1.0), (512, 1.0), (256, R.PEAK), (512, R.PEAK)])
def test_nystrom_core_with_the_route_on(n_pad, peak, monkeypatch):
    """The four combinations of the two switches against the float64 core on the same inputs, over transmil_ref.core_blocks;
    they need not agree bit for bit."""
    qkv, w, dO, pad = R.core_case(n_pad, peak)
    ref, r32, blks = R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32), R.core_blocks(n_pad, pad)
    calls = _count_fused_calls(monkeypatch)
    for a1 in (False, True):
        for a3 in (False, True):
            before = len(calls)
            got, attn = _core(qkv, w, dO, fused_a1=a1, fused_a3=a3)
            assert len(calls) - before == int(a1)
            assert attn is None and bool(torch.isfinite(got["dqkv"]).all())
            TR.hold("core", f"n_pad {n_pad} peak {peak} fused_a1 {a1} fused_a3 {a3}", got, ref, r32, blks)


def test_switch_off_issues_the_old_launches(monkeypatch):
    """fused_a1=False never reaches the new entry, and its forward has the bits of a call that does not know the keyword (at
    n_pad 512 the forward's split-K product has two addends, so it is reproducible)."""
    qkv, w, dO, _ = R.core_case(512)
    calls = _count_fused_calls(monkeypatch)
    monkeypatch.delenv("MIL_TM_FUSED_A1", raising=False)
    monkeypatch.delenv("MIL_TM_FUSED_A3", raising=False)
    off, _ = _core(qkv, w, dO, fused_a1=False)
    plain, _ = _core(qkv, w, dO)
    assert len(calls) == 0
    assert torch.equal(_bits(off["out"]), _bits(plain["out"]))
    assert rel(off["dqkv"], plain["dqkv"]) < 1e-5            # the same launches; their split-K sums add atomically, in any order


def test_attention_outputs_keep_the_materialised_route(monkeypatch):
    """need_attn "cls" and True read the map: with the switch on (keyword or environment) the forward gives the bits of the
    switch off and the fused entry is never called."""
    geo = R.geometry(250)                                                 # n_pad 512, s 16, pad 255
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn((geo["n_pad"], 1536), generator=g, dtype=torch.float64)
    qkv[:geo["pad"]] = 0
    w = (torch.rand((R.H, 1, R.CONV, 1), generator=g, dtype=torch.float64) * 2 - 1) / R.CONV ** 0.5
    dO = torch.randn((geo["n_pad"], 512), generator=g, dtype=torch.float64)
    cls = dict(need_attn="cls", pad=geo["pad"], s=geo["s"], n=250)
    calls = _count_fused_calls(monkeypatch)
    monkeypatch.delenv("MIL_TM_FUSED_A1", raising=False)
    monkeypatch.delenv("MIL_TM_FUSED_A3", raising=False)
    off, a_off = _core(qkv, w, dO, fused_a1=False, **cls)
    on, a_on = _core(qkv, w, dO, fused_a1=True, **cls)
    monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
    env, a_env = _core(qkv, w, dO, **cls)
    assert a_off.shape == (8, 256)
    for got, attn in ((on, a_on), (env, a_env)):
        assert torch.equal(_bits(attn), _bits(a_off))
        assert torch.equal(_bits(got["out"]), _bits(off["out"]))
        assert rel(got["dqkv"], off["dqkv"]) < 1e-5      # the same launches; their split-K sums add atomically, in any order
    with torch.no_grad():
        from mil_amd import ops
        qd, wd = qkv.float().to(DEV), w.float().to(DEV)
        o_off, m_off = ops.nystrom_core(qd, wd, True, fused_a1=False)
        o_env, m_env = ops.nystrom_core(qd, wd, True)                     # the environment says 1
        o_on, m_on = ops.nystrom_core(qd, wd, True, fused_a1=True)
    assert m_off.shape == (8, 512, 512)
    for o, m in ((o_env, m_env), (o_on, m_on)):
        assert torch.equal(_bits(m), _bits(m_off)) and torch.equal(_bits(o), _bits(o_off))
    assert len(calls) == 0


@pytest.mark.parametrize("a3", ["0", "1"])
@pytest.mark.parametrize("tag", ["transmil_N7", "transmil_N250", "transmil_N1000"])
def test_module_eval_against_reference_goldens_with_the_switch_on(tag, a3, golden, monkeypatch):
    """test_gpu_transmil.py::test_module_eval_against_reference_goldens with MIL_TM_FUSED_A1=1, alone and beside
    MIL_TM_FUSED_A3=1: fwd + BCE + bwd against tests/golden/transmil_*.npz on the module's standing bounds."""
    from mil_amd import synthetic as syn
    monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
    monkeypatch.setenv("MIL_TM_FUSED_A3", a3)
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
    print(f"golden {tag} fused_a1 (a3 {a3}): h {err['h']:.2e} logits {err['logits']:.2e} loss {err['loss']:.2e} worst grad {worst:.2e}")


def test_replay_with_both_switches_on_matches_the_reference_goldens(golden, monkeypatch):
    """test_gpu_landmark_attn.py::test_replay_with_the_switch_on_matches_the_reference_goldens with both switches on: the graph
    of side 32 is captured on N = 990 and replayed on the golden bag of N = 1000.  One capture."""
    from mil_amd import synthetic as syn
    from mil_amd.transmil_step import RaggedTransMILStepper
    monkeypatch.setenv("MIL_TM_FUSED_A1", "1")
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
    print(f"replayed golden transmil_N1000 fused_a1 + fused_a3: {err}")
    assert err["h"] <= 1e-4 and err["logits"] <= 1e-4 and err["loss"] <= 1e-4, err
    assert torch.equal(prob.detach().cpu().argmax(-1), g["prob"].argmax(-1))
    print(f"replayed golden transmil_N1000 fused_a1 + fused_a3: worst grad {_check_grads(model, g):.2e}")


def test_the_route_gives_back_a_map_of_peak_memory():
    """nystrom_core forward + backward at n_pad = 2048, fused_a3 off throughout: the materialised route holds A1 and dA1 at the
    backward's peak, the fused one neither and a workspace of half a map, so its peak is lower by at least one map
    (8 x 256 x 2048 floats)."""
    n_pad = 2048
    qkv, w, dO, _ = R.core_case(n_pad)
    peak = {}
    for fused in (False, True, False):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _core(qkv, w, dO, fused_a1=fused, fused_a3=False)
        peak.setdefault(fused, []).append(torch.cuda.max_memory_allocated() - base)
    print(f"PEAK | n_pad {n_pad} | materialised {peak[False]} | fused {peak[True]} | one map {MAP_BYTES * n_pad}")
    assert min(peak[False]) - peak[True][0] >= MAP_BYTES * n_pad, peak
