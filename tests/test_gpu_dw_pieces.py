"""GPU: the split-bf16 K loop of the fp32 gate weight gradient (k_gate_bwd_dw2_pieces, the default of the dw2 route) against a
float64 restatement, beside the f32-MFMA loop (MIL_DW_PIECES=0) on the same inputs in the same process.

Shapes: the bench shape (32 x 1024 x 512) in train and eval mode, a ragged total (31 777 rows: not a multiple of 32, not of
kc), a bucketed batch (capacity 32 768, 30 904 true rows on the device, large finite garbage beyond them), and L = 128 and
L = 1024, all on the dw2 route, and "planted": operands whose leading pieces cancel over the rows, on which a missing cross
term would exceed bound (a) 37-fold (tests/test_dw_pieces_host.py shows that on the CPU).  Outputs: dWv, dWu, dbv, dbu, dw, db.

Bounds:
  (a) max|got - ref| <= 1e-4 max|ref| (the project's gradient bar, tests/test_gpu_step_routes.py);
  (b) the new loop's float64 error is at most RATIO_BOUND times the f32 loop's float64 error on the same input, per output
      (floor 1e-7 on the f32 side, the floor of the forward's rule).  RATIO_BOUND is twice the largest ratio measured over
      these shapes (docs/lab_notes.md, "split-bf16 weight gradient").
The two settings must also differ in some bit at the bench shape - the switch reaches the kernel - and one whole step through
mil_image_only_step_run agrees between them within the bars of test_gpu_gate_pieces.py's one-step test."""
import pytest
import torch

from mil_amd import _lib, ops
from mil_amd import synthetic as syn
from mil_amd.bags import BagLayout
from mil_amd.trainer import ImageOnlyTrainer
from step_ref import dw_route, dw_split, keep_from_bits, max_err, num_cu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL_ABS = 1e-4
RATIO_BOUND = 2.0 * 2.05         # twice the largest measured ratio (db at L = 1024, 2.04; docs/lab_notes.md)
NAMES = ("dWv", "dWu", "dbv", "dbu", "dw", "db")


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    torch.cuda.empty_cache()


def _inputs(R, L, seed, train):
    """x, gates = [tanh | sigmoid] of random pre-activations, ds, w, keep words: what the backward of a step would hand over."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((R, L), device=DEV, generator=g)
    pre = torch.randn((R, 384), device=DEV, generator=g)
    gates = torch.cat([torch.tanh(pre[:, :192]), torch.sigmoid(pre[:, 192:])], 1).contiguous()
    ds = torch.randn(R, device=DEV, generator=g) * 1e-3
    w = torch.randn(192, device=DEV, generator=g) * 0.1
    bits = None
    if train:
        bits = torch.randint(-2 ** 31, 2 ** 31, (R, L // 32), device=DEV, generator=g, dtype=torch.int64).to(torch.int32)
    return x, gates, ds, w, bits


def _planted_inputs(R, L, seed):
    """The construction of tests/test_dw_pieces_host.py through the kernel's own staging arithmetic: V = 0, w = 1, ds = 2^-12,
    U = (1 + f') / 2 give dPreV = 2^-13 (1 + f') exactly (dPreU = 0); x[k][j] = s_k c_j + f with balanced signs.  The leading
    pieces cancel over the rows, so a missing (1, 1) term would be 3.7e-3 of max|dWv|: 37x bound (a)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    sgn = torch.ones((R, 1), device=DEV)
    sgn[1::2] = -1.0
    c = (1.0 + torch.rand((1, L), device=DEV, generator=g)).to(torch.bfloat16).float()
    x = sgn * c + 2.0 ** -8 * (0.9 + 0.09 * torch.rand((R, L), device=DEV, generator=g))
    U = 0.5 * (1.0 + 2.0 ** -8 * (0.9 + 0.09 * torch.rand((R, 192), device=DEV, generator=g)))
    gates = torch.cat([torch.zeros((R, 192), device=DEV), U], 1).contiguous()
    return x, gates, torch.full((R,), 2.0 ** -12, device=DEV), torch.ones(192, device=DEV), None


def _ref(x, gates, ds, w, bits, n, xscale):
    """float64: dPreV = ds w U (1 - V^2), dPreU = ds w V U (1 - U); dW = dPre^T (x keep) xscale over the first n rows."""
    L = x.shape[1]
    xd = x[:n].double()
    if bits is not None:
        xd = xd * keep_from_bits(bits[:n], L)
    V, U = gates[:n, :192].double(), gates[:n, 192:].double()
    d, wd = ds[:n].double().unsqueeze(1), w.double().unsqueeze(0)
    pv = d * wd * U * (1 - V * V)
    pu = d * wd * V * U * (1 - U)
    return dict(dWv=pv.t() @ xd * xscale, dWu=pu.t() @ xd * xscale, dbv=pv.sum(0), dbu=pu.sum(0),
                dw=(d * V * U).sum(0), db=d.sum().view(1))


def _run(x, gates, ds, w, bits, xscale, rows=None):
    """partials + fold through the C entries; rows: the true row count on the device (mil_gate_bwd_partials_rows)."""
    R, L = x.shape
    lib = _lib.lib()
    need = lib.mil_gate_bwd_workspace_floats(R, L)
    ws = torch.empty(need, device=DEV, dtype=torch.float32)
    out = dict(dWv=torch.empty((192, L), device=DEV), dWu=torch.empty((192, L), device=DEV), dbv=torch.empty(192, device=DEV),
               dbu=torch.empty(192, device=DEV), dw=torch.empty(192, device=DEV), db=torch.empty(1, device=DEV))
    p = ops._p
    if rows is None:
        rc = lib.mil_gate_bwd_partials(p(x), p(gates), p(ds), p(w), R, L, 192, p(ws), ws.numel(), p(bits), ops._stream())
    else:
        rc = lib.mil_gate_bwd_partials_rows(p(x), p(gates), p(ds), p(w), R, L, 192, p(ws), ws.numel(), p(bits), p(rows),
                                            ops._stream())
    _lib.check(rc, "mil_gate_bwd_partials")
    rc = lib.mil_gate_bwd_reduce(p(ws), R, L, p(out["dWv"]), p(out["dbv"]), p(out["dWu"]), p(out["dbu"]), p(out["dw"]),
                                 p(out["db"]), 0, float(xscale), ops._stream())
    _lib.check(rc, "mil_gate_bwd_reduce")
    torch.cuda.synchronize()
    return out


# id, rows the launch is sized for, L, train, true rows on the device (None: all)
CASES = [
    ("bench_train", 32768, 512, True, None),
    ("bench_eval", 32768, 512, False, None),
    ("ragged_31777", 31777, 512, True, None),
    ("bucket_32768_of_30904", 32768, 512, True, 30904),
    ("L128", 49152, 128, True, None),
    ("L1024", 31000, 1024, False, None),
    ("planted", 32768, 512, False, None),
]


@pytest.mark.parametrize("name,R,L,train,true_rows", CASES, ids=[c[0] for c in CASES])
def test_against_float64_beside_the_f32_loop(name, R, L, train, true_rows, monkeypatch):
    assert dw_route(R, L, num_cu()) == "dw2", (name, dw_route(R, L, num_cu()))
    if name.startswith("ragged"):
        kc = dw_split(R, L, num_cu())[1]
        assert R % 32 != 0 and R % kc != 0, (R, kc)
    n = true_rows if true_rows is not None else R
    planted = name == "planted"
    x, gates, ds, w, bits = _planted_inputs(R, L, 77) if planted else _inputs(R, L, 1000 + R + L, train)
    names = ("dWv", "dbv", "db") if planted else NAMES          # planted: dWu, dbu, dw are exactly zero on both sides
    rows = None
    if true_rows is not None:
        rows = torch.tensor([true_rows], device=DEV, dtype=torch.int32)
        x[n:] *= 1e3                                             # large finite garbage beyond the batch
        ds[n:] = 7.0
    xscale = 2.0 if train else 1.0
    ref = _ref(x, gates, ds, w, bits, n, xscale)
    got = {}
    for pieces in ("1", "0"):
        monkeypatch.setenv("MIL_DW_PIECES", pieces)
        got[pieces] = _run(x, gates, ds, w, bits, xscale, rows)
    err = {s: {k: max_err(got[s][k], ref[k]) for k in names} for s in got}
    ratio = {k: err["1"][k] / max(err["0"][k], 1e-7) for k in names}
    print(f"{name}: pieces " + " ".join(f"{k} {err['1'][k]:.2e}" for k in names) + " | f32 loop " +
          " ".join(f"{k} {err['0'][k]:.2e}" for k in names) + " | ratio " + " ".join(f"{k} {ratio[k]:.3f}" for k in names))
    if planted:
        for k in ("dWu", "dbu", "dw"):
            assert not got["1"][k].any() and not ref[k].any(), (name, k)
    if name.startswith("bench"):
        assert not torch.equal(got["1"]["dWv"], got["0"]["dWv"]) or not torch.equal(got["1"]["dWu"], got["0"]["dWu"]), \
            "MIL_DW_PIECES does not reach the kernel: both settings give the same bits"
    for k in names:
        assert err["1"][k] <= TOL_ABS, (name, k, err["1"][k])
        assert ratio[k] <= RATIO_BOUND, (name, k, ratio[k], err["1"][k], err["0"][k])


def test_one_step_agrees_with_the_f32_loop(monkeypatch):
    """One whole train step through mil_image_only_step_run at the bench shape with either K loop of the weight gradient:
    the forward is untouched (loss, prob, logits equal), the gradients agree within test_gpu_gate_pieces.py's bar."""
    L, lengths = 512, [1024] * 32
    p = syn.image_only_params(95, L=L)
    x = torch.randn(sum(lengths), L, generator=torch.Generator().manual_seed(6)).to(DEV)
    y = syn.make_labels(74, len(lengths)).to(DEV)
    lay = BagLayout.make(lengths, DEV)
    assert dw_route(sum(lengths), L, num_cu()) == "dw2"
    out = {}
    for pieces in ("1", "0"):
        monkeypatch.setenv("MIL_DW_PIECES", pieces)
        tr = ImageOnlyTrainer(p, DEV, lr=1e-3, train_mode=True)
        loss, prob = tr.train_step(x, lay, y)
        torch.cuda.synchronize()
        out[pieces] = (float(loss.item()), prob.cpu().clone(), tr.last["logits"].cpu().clone(), tr.fp.grad.cpu().clone())
    a, b = out["1"], out["0"]
    gdiff = float((a[3] - b[3]).abs().max()) / float(b[3].abs().max())
    print(f"one step: loss {a[0]} / {b[0]}, max grad difference {gdiff:.2e} of max|grad|")
    assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0])
    assert float((a[1] - b[1]).abs().max()) <= 1e-5 * float(b[1].abs().max())
    assert float((a[2] - b[2]).abs().max()) <= 1e-5 * float(b[2].abs().max())
    assert gdiff <= 1e-4
    assert not torch.equal(a[3], b[3]), "MIL_DW_PIECES does not reach the one-call step"
