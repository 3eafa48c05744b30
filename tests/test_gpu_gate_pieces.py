"""GPU: the split-bf16 gate forward of the fp32 one-call step (three bf16 pieces per operand, k_gate_fwd2<.., PW>) - the
weight pieces, their upkeep by the optimizer, and its accuracy against float64 next to the fp32-MFMA forward."""
import pytest
import torch

from mil_amd import _lib, ops
from mil_amd import synthetic as syn
from mil_amd.bags import BagLayout
from mil_amd.trainer import ImageOnlyTrainer
from step_ref import gates_ref, keep_from_bits, max_err, step_route

pytestmark = pytest.mark.gpu

WV, WU = "aggregator.attention_V.0.weight", "aggregator.attention_U.0.weight"
BV, BU = "aggregator.attention_V.0.bias", "aggregator.attention_U.0.bias"
WW, WB = "aggregator.attention_weights.weight", "aggregator.attention_weights.bias"


def split3(w: torch.Tensor):
    """p0 + p1 + p2 == w (round to nearest even at every step; non-finite w: p1 = p2 = 0)."""
    p0 = w.to(torch.bfloat16)
    r = w - p0.float()
    r = torch.where(torch.isfinite(r), r, torch.zeros_like(r))
    p1 = r.to(torch.bfloat16)
    p2 = (r - p1.float()).to(torch.bfloat16)
    return p0, p1, p2


def pieces_layout(Wv: torch.Tensor, Wu: torch.Tensor) -> torch.Tensor:
    """[L/16][3][2][384][8] int16 bit patterns, the layout of mil_gate_pieces."""
    W = torch.cat([Wv, Wu], 0).float()                          # [384, L]
    L = W.shape[1]
    ps = torch.stack([p.view(torch.int16) for p in split3(W)], 0)   # [3, 384, L]
    return ps.view(3, 384, L // 16, 2, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


def device_pieces(Wv: torch.Tensor, Wu: torch.Tensor) -> torch.Tensor:
    out = torch.empty(3 * (Wv.numel() + Wu.numel()), device=Wv.device, dtype=torch.int16)
    rc = _lib.lib().mil_gate_pieces(Wv.data_ptr(), Wu.data_ptr(), out.data_ptr(), Wv.shape[1], ops._stream())
    _lib.check(rc, "mil_gate_pieces")
    return out


def _pw_forward_matches_float64(tr, seed):
    """A forward of 32 x 1024 rows - the split-bf16 K loop, which reads the weight pieces - against float64 from the
    trainer's current masters."""
    dev = torch.device("cuda")
    L, lengths = tr.fp.p(WV).shape[1], [1024] * 32
    assert step_route(sum(lengths), L, 2, tr.train_mode, aligned32=True)["main"] == "fwd2_pw"
    x = torch.randn(sum(lengths), L, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    tr.forward(x, BagLayout.make(lengths, dev), syn.make_labels(seed, len(lengths)).to(dev))
    torch.cuda.synchronize()
    keep = keep_from_bits(tr.last["xbits"], L) if tr.train_mode else None
    rs, rg = gates_ref(x, tr.fp.state_dict(), keep)
    es, eg = max_err(tr.last["scores"], rs), max_err(tr.last["gates"], rg)
    print(f"32 x 1024 forward on the planes: scores {es:.1e} gates {eg:.1e}")
    assert es <= 1e-5 and eg <= 1e-5, (es, eg)


def test_pieces_sum_back_exactly():
    dev = torch.device("cuda")
    L = 512
    g = torch.Generator().manual_seed(11)
    Wv = torch.randn(192, L, generator=g)
    Wu = torch.randn(192, L, generator=g)
    Wv[0] *= 1e30
    Wv[1] *= 1e-25
    Wv[2, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -20)])
    Wu[0] *= 1e-20
    Wu[1] = torch.rand(L, generator=g) * 2.0 ** 60
    got = device_pieces(Wv.to(dev), Wu.to(dev)).cpu()
    assert torch.equal(got, pieces_layout(Wv, Wu))
    W = torch.cat([Wv, Wu], 0)
    ps = got.view(L // 16, 3, 2, 384, 8).permute(1, 3, 0, 2, 4).reshape(3, 384, L)
    ps = [p.view(torch.bfloat16).double() for p in ps]
    assert torch.equal(ps[0] + ps[1] + ps[2], W.double())
    # signed zeros stay zeros in every piece
    assert torch.equal(ps[0][2, :2], torch.zeros(2, dtype=torch.float64)) and float(ps[1][2, :2].abs().sum()) == 0.0


@pytest.mark.parametrize("fused_adam", [True, False])
def test_trainer_planes_follow_the_masters(fused_adam):
    dev = torch.device("cuda")
    L, lengths = 512, [256, 96, 160]
    p = syn.image_only_params(91, L=L)
    tr = ImageOnlyTrainer(p, dev, lr=1e-3, train_mode=True)
    assert tr.gate_pieces
    x = torch.randn(sum(lengths), L, generator=torch.Generator().manual_seed(3)).to(dev)
    y = syn.make_labels(72, len(lengths)).to(dev)
    lay = BagLayout.make(lengths, dev)
    for _ in range(3):
        if fused_adam:
            tr.train_step(x, lay, y)            # Adam in the fold launch
        else:
            tr.forward(x, lay, y)
            tr.backward()
            tr.reduce_and_step()                # MIL_STAGE_ADAM on its own
    torch.cuda.synchronize()
    assert torch.equal(tr._wp.cpu(), pieces_layout(tr.fp.p(WV).cpu(), tr.fp.p(WU).cpu()))
    _pw_forward_matches_float64(tr, 7)
    # a host-side parameter write is followed by a fresh split before the next step reads the planes
    sd = {k: v.clone() * 0.5 for k, v in tr.fp.state_dict().items()}
    tr.load_model_state_dict(sd)
    tr.forward(x, lay)
    torch.cuda.synchronize()
    assert torch.equal(tr._wp.cpu(), pieces_layout(tr.fp.p(WV).cpu(), tr.fp.p(WU).cpu()))
    _pw_forward_matches_float64(tr, 8)


def _ref64(x, p, keep=None):
    x = x.double()
    if keep is not None:
        x = x * keep.double() * 2.0
    v = torch.tanh(x @ p[WV].double().t() + p[BV].double())
    u = torch.sigmoid(x @ p[WU].double().t() + p[BU].double())
    s = (v * u) @ p[WW].double().view(-1) + p[WB].double()
    return s, torch.cat([v, u], 1)


def _keep_from_bits(bits: torch.Tensor, L: int) -> torch.Tensor:
    b = bits.cpu().view(torch.int32).long() & 0xFFFFFFFF
    shifts = torch.arange(32)
    return ((b.unsqueeze(-1) >> shifts) & 1).view(b.shape[0], L).float()


def _relerr(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _forward(pieces, p, x, lay, y, train, dev):
    tr = ImageOnlyTrainer(p, dev, train_mode=train)
    tr.gate_pieces = pieces
    tr.forward(x, lay, y)
    torch.cuda.synchronize()
    last = tr.last
    keep = _keep_from_bits(last["xbits"], x.shape[1]) if train else None
    return last["scores"].cpu(), last["gates"].cpu(), keep


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shape", [(32, 1024), (40, 832)])
def test_accuracy_against_float64(shape, train):
    dev = torch.device("cuda")
    B, n = shape
    L = 512
    p = syn.image_only_params(93, L=L)
    x = torch.randn(B * n, L, generator=torch.Generator().manual_seed(5))
    y = syn.make_labels(73, B).to(dev)
    lay = BagLayout.make([n] * B, dev)
    xd = x.to(dev)
    errs = {}
    for pieces in (True, False):
        s, g, keep = _forward(pieces, p, xd, lay, y, train, dev)
        rs, rg = _ref64(x, p, keep)
        errs[pieces] = (_relerr(s, rs), _relerr(g, rg))
    print(f"shape {shape} train {train}: split-bf16 (scores, gates) {errs[True]}, fp32 MFMA {errs[False]}")
    for i in range(2):
        assert errs[True][i] <= 1.5 * max(errs[False][i], 1e-7), (errs, i)


def test_one_step_agrees_with_fp32_mfma_path():
    dev = torch.device("cuda")
    L, lengths = 512, [1024] * 32
    p = syn.image_only_params(95, L=L)
    x = torch.randn(sum(lengths), L, generator=torch.Generator().manual_seed(6)).to(dev)
    y = syn.make_labels(74, len(lengths)).to(dev)
    lay = BagLayout.make(lengths, dev)
    out = {}
    for pieces in (True, False):
        # 32 x 1024 rows: both arms run k_gate_fwd2 (split-bf16 and fp32-MFMA K loops), not the 32-row kernel
        assert step_route(sum(lengths), L, 2, True, aligned32=True, pieces=pieces)["main"] == ("fwd2_pw" if pieces else "fwd2")
        tr = ImageOnlyTrainer(p, dev, lr=1e-3, train_mode=True)
        tr.gate_pieces = pieces
        loss, prob = tr.train_step(x, lay, y)
        torch.cuda.synchronize()
        out[pieces] = (float(loss.item()), prob.cpu().clone(), tr.last["logits"].cpu().clone(), tr.fp.grad.cpu().clone())
    a, b = out[True], out[False]
    assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0])
    assert float((a[1] - b[1]).abs().max()) <= 1e-5 * float(b[1].abs().max())
    assert float((a[2] - b[2]).abs().max()) <= 1e-5 * float(b[2].abs().max())
    assert float((a[3] - b[3]).abs().max()) <= 1e-4 * float(b[3].abs().max())
