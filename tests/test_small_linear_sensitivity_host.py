"""CPU: what the per-block bounds of tests/test_gpu_small_linear_stages.py can see.

The GPU bound of a block is k x max(e32, 1e-7), k <= 16, with e32 the error of the float32 restatement of the same entry on
the CPU against float64 (tests/small_linear_ref.py).  Over the GPU file's own run lists, inputs and blocks:
  a. the closed forms equal torch autograd to 1e-12 in float64;
  b. every block has a non-zero reference, except the planted one (row N - 1 of dW behind a dead ReLU column), which is
     exactly zero; the float32 restatement is finite on every block;
  c. every planted error (mutate= of the restatement), measured in float64 against the clean float64 result, exceeds the
     bound at the cap k = 16 by a factor of 10 on at least one block of at least one run.
pytest -s lists the covering run, block and margin of every planted error and the smallest margin.  Nothing here reads the
code under test."""
import functools
import math

import torch

import small_linear_ref as S

MARGIN = 10.0
FWD_OUT = ("y", "xin", "xn", "mean", "rstd")
SENT = -12345.678


def _fwd_out(r):
    return {n: v for n, v in r.items() if n in FWD_OUT}


def _dw_runs():
    return [dict(M=m, N=n, K=k, act=a, outs=("dW", "db")) for m in S.DW_ROWS
            for (n, k), a in dict.fromkeys(zip(S.DW_ALL, S.DW_ACTS))]


# stage -> (runs, restatement of a run, blocks of a run)
STAGES = {
    "fwd": (S.fwd_runs(False) + S.fwd_runs(True), lambda r, *a: _fwd_out(S.run_fwd(r, *a)), lambda r: S.lin_blocks(r["M"], r["N"], r["K"])),
    "bwd": (S.bwd_runs(False) + S.bwd_runs(True), S.run_bwd, lambda r: S.lin_blocks(r["M"], r["N"], r["K"])),
    "bwd_split": (S.split_runs(), S.run_split,
                  lambda r: {"parts": S.part_blocks(r["nsplit"], r["M"], r["K"]), "dx": S.row_blocks(r["M"], r["K"])}),
    "ln_fwd": (S.ln_fwd_runs(), lambda r, *a: _fwd_out(S.run_fwd(r, *a)), lambda r: S.lin_blocks(r["M"], r["N"], r["K"])),
    "ln_bwd": (S.ln_bwd_runs(), S.run_ln_bwd, lambda r: S.ln_bwd_blocks(r["M"], r["K"])),
    "dw_grouped": (_dw_runs(), S.run_dw, lambda r: S.lin_blocks(r["M"], r["N"], r["K"])),
}


def _dwdb(r):
    return "dW" in r["outs"] or "db" in r["outs"]


# (stage, planted error, the runs it applies to)
PLANTED = [
    ("fwd", "k_last16", lambda r: True),
    ("fwd", "k_chunk2", lambda r: r["K"] > S.KCH),
    ("fwd", "xin_x", lambda r: r["x2"]),
    ("bwd", "odd_last_row", lambda r: r["M"] % 2 and _dwdb(r)),
    ("bwd", "rows32", lambda r: r["M"] > 32 and _dwdb(r)),
    ("bwd", "k_last16", lambda r: "dx" in r["outs"]),
    ("bwd", "k_chunk2", lambda r: "dx" in r["outs"] and r["N"] > S.KCH),
    ("bwd", "skip_dy3", lambda r: r["extras"][1]),
    ("bwd", "missing_w1", lambda r: any(r["extras"]) and not all(r["extras"])),
    ("bwd", "dysum_after", lambda r: r["dysum"] and r["act"]),
    ("bwd", "gelu_from_out", lambda r: r["act"] == 3),
    ("bwd", "sigmoid_y", lambda r: r["act"] == 4),
    ("bwd_split", "split_range", lambda r: True),
    ("ln_fwd", "onepass", lambda r: True),
    ("ln_fwd", "eps_outside", lambda r: True),
    ("ln_fwd", "var_e1", lambda r: True),
    ("ln_fwd", "xin_x", lambda r: r["x2"]),
    ("ln_bwd", "rows32", lambda r: r["M"] > 32 and "dgamma" in r["outs"]),
    ("ln_bwd", "skip_g3", lambda r: r["pat"][1]),
    ("ln_bwd", "skip_g5", lambda r: r["pat"][3]),
    ("ln_bwd", "missing_w1", lambda r: not all(r["pat"])),
    ("ln_bwd", "no_xhat_term", lambda r: True),
    ("ln_bwd", "no_gamma", lambda r: True),
    ("dw_grouped", "odd_last_row", lambda r: r["M"] % 2),
    ("dw_grouped", "rows32", lambda r: r["M"] > 32),
]


@functools.lru_cache(maxsize=None)
def _clean(stage, i):
    runs, fn, blocks = STAGES[stage]
    return fn(runs[i]), fn(runs[i], torch.float32), blocks(runs[i])


def _margin(mut, ref, r32, blocks):
    best = (0.0, None, 0.0, 0.0)
    for t in mut:
        e32, em = S.block_err(r32[t], ref[t], blocks[t]), S.block_err(mut[t], ref[t], blocks[t])
        for b in em:
            m = em[b] / S.bound(e32[b], S.K_CAP)
            if m > best[0]:
                best = (m, f"{t}.{b}", em[b], e32[b])
    return best


def test_closed_forms_equal_autograd():
    for M, N, K in ((7, 48, 32), (33, 512, 256), (64, 256, 528)):
        for act in range(5):
            c = S.lin_case(M, N, K, act)
            ag = S.autograd_linear(c["x"], c["W"], c["b"], act, c["residual"], c["x2"], c["dy"])
            f = S.fwd(c["x"], c["W"], c["b"], act, c["residual"], c["x2"])
            b = S.bwd(c["dy"], f["pre"] if act == 3 else f["a"], act, f["xin"], c["W"])
            for n, got in (("y", f["y"]), ("dx", b["dx"]), ("dW", b["dW"]), ("db", b["db"])):
                err = S.block_err(got, ag[n], {"all": (Ellipsis,)})["all"]
                assert err <= 1e-12, (M, N, K, act, n, err)
    for M, K in ((7, 48), (33, 512)):
        c = S.ln_bwd_case(M, K)
        g = c["g1"] + c["g2"] + c["g3"] + c["g4"] + c["g5"]
        beta = S.lin_case(M, 16, S.E, 0, True)["beta"]
        ag = S.autograd_ln(c["u"], c["gamma"], beta, S.EPS, c["W"], g)
        f = S.ln_fwd(c["u"], c["gamma"], beta, S.EPS, torch.eye(S.E, dtype=torch.float64))
        b = S.ln_bwd([c[n] for n in ("g1", "g2", "g3", "g4", "g5")], c["u"], f["mean"], f["rstd"], c["gamma"], c["W"])
        b["xn"] = f["xn"]
        for n in ("xn", "du", "dx", "dgamma", "dbeta"):
            err = S.block_err(b[n], ag[n], {"all": (Ellipsis,)})["all"]
            assert err <= 1e-12, (M, K, n, err)
    a, b4, c4, d4 = (torch.randn(1020, dtype=torch.float64) for _ in range(4))
    assert torch.equal(S.sum4(a, b4, c4, d4)["out"], a + b4 + (c4 + d4)) and torch.equal(S.sum4(a, b4)["out"], a + b4)


def test_every_block_has_teeth():
    """(b): no block but the planted one has an all-zero reference; the planted one is exactly zero in both dtypes."""
    for stage, (runs, _, _) in STAGES.items():
        n, worst = 0, 0.0
        for i, run in enumerate(runs):
            ref, r32, blocks = _clean(stage, i)
            for t in ref:
                e32 = S.block_err(r32[t], ref[t], blocks[t])
                for name, ix in blocks[t].items():
                    top = float(ref[t][ix].abs().max())
                    if S.expected_zero(run.get("act", 0), run.get("N", 0), t, name):
                        assert top == 0.0 and e32[name] == 0.0, (stage, run, t, name, top)
                    else:
                        assert top > 0.0 and math.isfinite(top) and math.isfinite(e32[name]), (stage, run, t, name, top)
                n += len(e32)
                worst = max(worst, max(e32.values()))
        print(f"stage {stage:<11} {len(runs):3d} runs, {n:6d} blocks, worst e32 {worst:.1e}")
    relu = [r for r in STAGES["bwd"][0] if r["act"] == 2 and "dW" in r["outs"]]
    assert relu, "no run holds the planted zero block"


def test_planted_errors_exceed_the_bounds():
    smallest = (math.inf, None)
    for stage, mutate, applies in PLANTED:
        runs, fn, _ = STAGES[stage]
        best = (0.0, None, None, 0.0, 0.0)
        for i, run in enumerate(runs):
            if not applies(run):
                continue
            ref, r32, blocks = _clean(stage, i)
            m, blk, em, e32 = _margin(fn(run, torch.float64, mutate), ref, r32, blocks)
            if m > best[0]:
                best = (m, run, blk, em, e32)
        m, run, blk, em, e32 = best
        assert run is not None, (stage, mutate, "applies to no run")
        print(f"planted {stage + '.' + mutate:<24} margin {m:10.1f}x on {blk:<12} (error {em:.1e}, e32 {e32:.1e}) run: {S.tag(run)}")
        assert m >= MARGIN, (stage, mutate, m, blk, run)
        if m < smallest[0]:
            smallest = (m, f"{stage}.{mutate}")
    print(f"smallest margin {smallest[0]:.1f}x ({smallest[1]})")


def test_row_written_one_slot_down_is_seen():
    """Clamped row M - 1 written to row M's slot of xn: the slot lies in the guard rows behind the output, which the GPU test
    compares with the sentinel bit for bit; stated here as a block of its own over the padded tensor."""
    for run in S.ln_fwd_runs()[:3]:
        M = run["M"]
        ref, r32 = S.run_fwd(run)["xn"], S.run_fwd(run, torch.float32)["xn"]
        guard = torch.full((3, S.E), SENT, dtype=torch.float64)
        pad = lambda t: torch.cat([t.double(), guard])                                         # noqa: E731
        mut = pad(ref)
        mut[M] = ref[M - 1]
        blocks = {"guard": (slice(M, M + 3),)}
        em, e32 = S.block_err(mut, pad(ref), blocks)["guard"], S.block_err(pad(r32), pad(ref), blocks)["guard"]
        m = em / S.bound(e32, S.K_CAP)
        print(f"planted ln_fwd.xn_row_clamp      margin {m:10.1f}x on xn.guard (error {em:.1e}) run: {S.tag(run)}")
        assert e32 == 0.0 and m >= MARGIN


def test_ln_fwd_in_the_kernels_summation_order():
    """The normalisation of mil_linear_small_ln_fwd in float32 numpy, sums in the kernel's order (small_linear_ref.
    ln_norm_in_kernel_order), over the GPU test's ln_fwd runs.  With the mean of the centred row added back every block of
    xn, mean, rstd is within the bound at k = 16; the single float32 sum the kernel had before is not, on rows of mean 30
    (10.3 x max(e32, 1e-7) on a row of xn, which the product behind it carried to 16.2 on y: lab notes, finding 3)."""
    worst = {True: (0.0, None), False: (0.0, None)}
    for run in S.ln_fwd_runs():
        c = S.lin_case(run["M"], run["N"], S.E, run["act"], True)
        ref, r32, blocks = S.run_fwd(run), S.run_fwd(run, torch.float32), S.lin_blocks(run["M"], run["N"], S.E)
        for corrected in (True, False):
            got = S.ln_norm_in_kernel_order(c["x"], c["gamma"], c["beta"], S.EPS, corrected)
            for t in got:
                e32, eg = S.block_err(r32[t], ref[t], blocks[t]), S.block_err(got[t], ref[t], blocks[t])
                for b in eg:
                    ratio = eg[b] / max(e32[b], S.FLOOR)
                    if ratio > worst[corrected][0]:
                        worst[corrected] = (ratio, f"{t}.{b} M {run['M']} (error {eg[b]:.2e}, e32 {e32[b]:.2e})")
    for corrected in (True, False):
        print(f"kernel order, {'corrected mean' if corrected else 'one float32 sum'}: largest ratio {worst[corrected][0]:.2f} on {worst[corrected][1]}")
    assert worst[True][0] <= S.K_CAP / 2 and worst[False][0] > 8.0
