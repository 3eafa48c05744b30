"""Host: the arithmetic of the split-bf16 weight gradient (k_gate_bwd_dw2_pieces), emulated in torch on the CPU.

dW = dPre^T x with every fp32 operand value split into three exact bf16 pieces (gp_split3) and the six cross terms (p, q),
p + q <= 2, accumulated in fp32.  Shown here, at a reduced row count:
  * the pieces sum back to the fp32 value exactly;
  * the six-term product's error against float64 is of the order of a plain fp32 product's;
  * a planted omission - the (1, 1) term dropped, or only the terms p + q <= 1 kept - exceeds the GPU test's bound
    (tests/test_gpu_dw_pieces.py: max|got - ref| <= 1e-4 max|ref|) by at least 10x on some output block, so that bound can see
    a missing term.  The operands are chosen for that: a dropped term of order 2^-16 relative shows only where the kept
    terms do not drown it, so the leading pieces are made to cancel over the rows while the second pieces (as large as bf16
    allows: fractions just below half a bf16 ulp, one sign) add up; tests/test_gpu_dw_pieces.py runs the same construction
    through the kernel (its case "planted")."""
import torch

TOL_GPU = 1e-4
R, L, D = 4096, 128, 64


def split3(v: torch.Tensor):
    """gp_split3 on finite fp32 values: p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1), round to nearest even."""
    p0 = v.to(torch.bfloat16).float()
    r = v - p0
    p1 = r.to(torch.bfloat16).float()
    p2 = (r - p1).to(torch.bfloat16).float()
    return p0, p1, p2


def pieces_product(a: torch.Tensor, b: torch.Tensor, terms):
    """sum over (p, q) in terms of a_p^T b_q, each term an fp32 matrix product accumulated in fp32, smallest first."""
    pa, pb = split3(a), split3(b)
    acc = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float32)
    for p, q in terms:
        acc = acc + pa[p].t() @ pb[q]
    return acc


SIX = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]


def _operands(seed):
    """dPre from random gates / ds / w and a keep-masked x, as the kernel stages them (fp32 arithmetic)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, L, generator=g)
    keep = (torch.rand(R, L, generator=g) < 0.5).float()
    pre = torch.randn(R, 2 * D, generator=g)
    V, U = torch.tanh(pre[:, :D]), torch.sigmoid(pre[:, D:])
    ds = torch.randn(R, 1, generator=g) * 1e-3
    w = torch.randn(1, D, generator=g) * 0.1
    a = (ds * w) * U
    t = a * V
    dpre = torch.cat([a - t * V, t - t * U], 1)
    return dpre, x * keep


def _relerr(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def test_pieces_sum_back_exactly():
    dpre, xk = _operands(1)
    for v in (dpre, xk):
        p0, p1, p2 = split3(v)
        assert torch.equal((p0.double() + p1.double() + p2.double()).float(), v)
        assert torch.equal(p0[v == 0], torch.zeros_like(p0[v == 0]))        # a dropped element splits to three zeros
        assert not p1[v == 0].any() and not p2[v == 0].any()


def test_six_terms_are_as_good_as_a_plain_fp32_product():
    dpre, xk = _operands(2)
    ref = dpre.double().t() @ xk.double()
    e_six = _relerr(pieces_product(dpre, xk, SIX), ref)
    e_f32 = _relerr(dpre.t() @ xk, ref)
    print(f"six-term split-bf16 {e_six:.2e}, plain fp32 {e_f32:.2e}")
    assert e_six <= 2.0 * max(e_f32, 1e-7)
    assert e_six <= TOL_GPU / 100


def _planted_operands():
    """Operands whose leading pieces cancel over the rows while their second pieces add up: x[k][j] = s_k c_j + f with
    balanced signs s_k, a bf16 value c_j in [1, 2) and a fraction f just below half a bf16 ulp (p0 = s_k c_j, p1 ~ f > 0);
    dPre[k][i] = 2^-13 (1 + f'), likewise (p0 = 2^-13, p1 ~ 2^-13 f').  The sum over k of the (0, 0) products is zero, the
    result is carried by the (0, 1) and (1, 0) terms, and the (1, 1) term is ~2^-8 of it, all of one sign."""
    g = torch.Generator().manual_seed(3)
    s = torch.ones(R, 1)
    s[1::2] = -1.0
    c = (1.0 + torch.rand(1, L, generator=g)).to(torch.bfloat16).float()
    xk = s * c + 2.0 ** -8 * (0.9 + 0.09 * torch.rand(R, L, generator=g))
    dpre = 2.0 ** -13 * (1.0 + 2.0 ** -8 * (0.9 + 0.09 * torch.rand(R, 2 * D, generator=g)))
    return dpre, xk


def test_a_planted_omission_exceeds_the_gpu_bound_tenfold():
    dpre, xk = _planted_operands()
    ref = dpre.double().t() @ xk.double()
    full = pieces_product(dpre, xk, SIX)
    e_full = _relerr(full, ref)
    print(f"planted operands: six terms {e_full:.2e}")
    assert e_full <= TOL_GPU / 100                                   # the complete product passes the GPU bound with room
    omissions = {"without (1, 1)": [t for t in SIX if t != (1, 1)],
                 "p + q <= 1 only": [t for t in SIX if sum(t) <= 1]}
    for name, terms in omissions.items():
        got = pieces_product(dpre, xk, terms)
        # per 32 x 32 output block (an MFMA tile), against the bound the GPU test applies: 1e-4 max|ref|
        err = (got.double() - ref).abs().view(2 * D // 32, 32, L // 32, 32).amax(dim=(1, 3)) / ref.abs().max()
        worst = float(err.max())
        print(f"planted operands, {name}: worst block {worst:.2e} = {worst / TOL_GPU:.1f} x the GPU bound")
        assert worst >= 10 * TOL_GPU, (name, worst)
