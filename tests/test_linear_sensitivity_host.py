"""CPU: what the per-block bounds of tests/test_gpu_linear_stages.py can see.

The GPU bound of a block is k x max(e32, 1e-7), k <= 16, with e32 the error of the float32 restatement of the same entry on
the CPU against float64 (tests/linear_ref.py).  Over the GPU file's own run lists, inputs and blocks, with the routes the rules
give at 256 compute units:
  a. the restatement, in every route's arithmetic order, equals the plain product / torch autograd to 1e-12 in float64;
  b. every block has a non-zero, finite reference, except the guard blocks, which hold the sentinel exactly, and the rows
     behind a bucket's 64-row boundary, which are exactly zero;
  c. every planted error (mutate= of the restatement), measured in float64 against the clean float64 result, exceeds the
     bound at the cap k = 16 by a factor of 10 on at least one block of at least one run.
pytest -s lists the covering run, block and margin of every planted error.  Nothing here loads the library."""
import functools
import math

import torch

import linear_ref as R

MARGIN = 10.0
RUNS = {"gemm": R.gemm_runs(), "bwd_params": R.bwd_runs()}
for _r in R.other_runs():
    RUNS.setdefault(_r["entry"], []).append(_r)


def _route(run):
    return R.route_of(run) if run["entry"] in ("gemm", "bwd_params") else None


@functools.lru_cache(maxsize=None)
def _clean(entry, i):
    run = RUNS[entry][i]
    c = R.run_inputs(run)
    return R.restate(run, inputs=c), R.restate(run, torch.float32, inputs=c), R.blocks_of(run)


def _tiled(run):
    return R.GEMM_MUTATIONS and run["N"] % (64 if run["kernel"] == "G64N" else 128) != 0 and run["N"] > 128


# (entry, planted error, the runs it applies to: f(run, route))
PLANTED = [
    ("gemm", "k_last_slice", lambda r, p: True),
    ("gemm", "split_missing", lambda r, p: p["S"] > 1),
    ("gemm", "bias_per_split", lambda r, p: p["S"] > 1 and r["bias"]),
    ("gemm", "act_per_partial", lambda r, p: p["S"] > 1 and r["act"]),
    ("gemm", "tail_res_offset", lambda r, p: p["kernel"] == "TAIL" and r["res"]),
    ("gemm", "tail_aux_offset", lambda r, p: p["kernel"] == "TAIL" and r["aux"] == 1),
    ("gemm", "tail_aux_offset", lambda r, p: p["kernel"] == "TAIL" and r["aux"] == 2),
    ("gemm", "tail_c_offset", lambda r, p: p["kernel"] == "TAIL"),
    ("gemm", "acc_overwrite", lambda r, p: r["acc"]),
    ("gemm", "aux1_post", lambda r, p: r["aux"] == 1 and r["act"]),
    ("gemm", "aux2_from_out", lambda r, p: r["aux"] == 2),
    ("gemm", "last_row", lambda r, p: r["rows"] is None),
    ("gemm", "col_shift", lambda r, p: _tiled(r)),
    ("gemm", "guard_write", lambda r, p: r["strided"]),
    ("gemm", "stale_behind", lambda r, p: r["rows"] is not None and r["rows"] + 63 < r["M"]),
    ("gemm", "zero_last_group", lambda r, p: r["rows"] is not None),
    ("bwd_params", "dact_from_dy", lambda r, p: r["act"]),
    ("bwd_params", "db_last_split", lambda r, p: p["S"] > 1),
    ("bwd_params", "dw_rows_mult", lambda r, p: p["kernel"] == "TN2"),
    ("bwd_params", "dw_rows_mult", lambda r, p: p["kernel"] == "TN_AX"),
    ("bwd_params", "rows_ignored", lambda r, p: p["kernel"] == "TN2" and r["rows"] is not None and r["rows"] < r["M"]),
    ("bwd_params", "acc_overwrite", lambda r, p: r["acc"]),
    ("bwd_params", "guard_write", lambda r, p: r["strided"]),
    ("colsum", "acc_overwrite", lambda r, p: r["acc"]),
    ("colsum", "last_chunk", lambda r, p: r["M"] > 256),
    ("act_bwd", "dact_from_dy", lambda r, p: True),
    ("mid_fwd", "k_last8", lambda r, p: True),
    ("mid_fwd", "last_row", lambda r, p: True),
    ("mid_bwd", "k_last8", lambda r, p: True),
    ("mid_bwd", "dw_rows_mult", lambda r, p: r["M"] % 8),
    ("mid_bwd", "dact_from_dy", lambda r, p: r["act"]),
]


def _plain_gemm(run, c):
    Aop = c["A"] if run["a_mode"] == 0 else c["A"].t()
    v = Aop @ (c["B"].t() if run["b_mode"] == 0 else c["B"])
    if c["bias"] is not None:
        v = v + c["bias"]
    pre = v
    if run["aux"] == 2:
        v = v * R.dgelu(c["pre"])
    v = R.act_fwd(v, run["act"])
    if c["residual"] is not None:
        v = v + c["residual"]
    if c["C0"] is not None:
        v = v + c["C0"]
    return v, pre


def test_restatement_equals_the_plain_product():
    """(a) over every run: the product, parameter gradients and column sums in each route's order against the one-line form."""
    whole = {"all": (Ellipsis,)}
    err = lambda a, b: R.block_err(a, b, whole)["all"]                                       # noqa: E731
    for entry, runs in RUNS.items():
        for i, run in enumerate(runs):
            ref, c, N, K = _clean(entry, i)[0], R.run_inputs(run), run["N"], run["K"]
            if entry == "gemm":
                v, pre = _plain_gemm(run, c)
                n = run["rows"] if run["rows"] is not None else run["M"]
                assert err(ref["C"][:n, :N], v[:n]) <= 1e-12, R.tag(run)
                if run["aux"] == 1:
                    assert err(ref["aux"][:, :N], pre) <= 1e-12, R.tag(run)
            elif entry == "bwd_params":
                n = run["rows"] if run["rows"] is not None else run["M"]
                g = R.dact(c["dy"], c["y"], run["act"])[:n]
                dW, db = g.t() @ c["x"][:n], g.sum(0)
                if run["acc"]:
                    dW, db = dW + c["dW0"], db + c["db0"]
                assert err(ref["dW"][:, :K], dW) <= 1e-12 and err(ref["db"], db) <= 1e-12, R.tag(run)
            elif entry == "colsum":
                assert err(ref["out"], c["Y"].sum(0) + (c["out0"] if run["acc"] else 0)) <= 1e-12
    for M, N, K, act in ((70, 136, 64, 1), (333, 512, 96, 2), (1000, 1056, 64, 0)):          # the mid kernels against autograd
        c = R.bwd_case(M, N, K, 0)
        x, W, b = (c[n].clone().requires_grad_(True) for n in ("x", "W", "b"))
        y = R.act_fwd(torch.nn.functional.linear(x, W, b), act) + c["residual"]
        y.backward(c["dy"])
        f = R.mid_fwd(c["x"], c["W"], c["b"], act, c["residual"])["y"]
        g = R.mid_bwd(c["dy"], f - c["residual"], act, c["x"], c["W"])
        pr = R.bwd_params(c["dy"], f - c["residual"], act, c["x"], R.bwd_params_route(M, N, K))
        assert err(f, y.detach()) <= 1e-12 and err(g["dx"], x.grad) <= 1e-12 and err(g["dW"], W.grad) <= 1e-12
        assert err(g["db"], b.grad) <= 1e-12 and err(pr["dW"], W.grad) <= 1e-12 and err(pr["db"], b.grad) <= 1e-12
        assert err(R.act_bwd(c["dy"], f - c["residual"], act)["dpre"] @ c["W"], x.grad) <= 1e-12


def test_every_block_has_teeth():
    """(b): a guard block holds the sentinel, the rows behind a bucket are zero, every other block's reference is non-zero
    and finite; the float32 restatement meets the two exact kinds exactly and is finite elsewhere."""
    kinds = set()
    for entry, runs in RUNS.items():
        n, worst = 0, 0.0
        for i, run in enumerate(runs):
            ref, r32, blocks = _clean(entry, i)
            for t in ref:
                e32 = R.block_err(r32[t], ref[t], blocks[t])
                for name, ix in blocks[t].items():
                    blk, kind = ref[t][ix], R.expected(name)
                    assert blk.numel() > 0, (R.tag(run), t, name)
                    if kind == "sentinel":
                        assert bool((blk == R.SENT).all()) and e32[name] == 0.0, (R.tag(run), t, name)
                    elif kind == "zero":
                        assert bool((blk == 0).all()) and e32[name] == 0.0, (R.tag(run), t, name)
                    else:
                        top = float(blk.abs().max())
                        assert top > 0.0 and math.isfinite(top) and math.isfinite(e32[name]), (R.tag(run), t, name, top)
                        assert not bool((blk == R.SENT).any()), (R.tag(run), t, name, "an output element was never written")
                    kinds.add(kind)
                    worst = max(worst, e32[name])
                n += len(e32)
        print(f"entry {entry:<11} {len(runs):3d} runs, {n:5d} blocks, worst e32 {worst:.1e}")
    assert kinds == {None, "sentinel", "zero"}


def test_planted_errors_exceed_the_bounds():
    smallest = (math.inf, None)
    for entry, mutate, applies in PLANTED:
        best = (0.0, None, None, 0.0, 0.0)
        order = sorted(range(len(RUNS[entry])), key=lambda i: RUNS[entry][i]["M"] * RUNS[entry][i]["N"] * max(1, RUNS[entry][i]["K"]))
        for i in order:
            run = RUNS[entry][i]
            if not applies(run, _route(run)):
                continue
            ref, r32, blocks = _clean(entry, i)
            mut = R.restate(run, torch.float64, mutate)
            for t in mut:
                e32, em = R.block_err(r32[t], ref[t], blocks[t]), R.block_err(mut[t], ref[t], blocks[t])
                for b in em:
                    m = em[b] / R.bound(e32[b], R.K_CAP)
                    if m > best[0]:
                        best = (m, run, f"{t}.{b}", em[b], e32[b])
            if best[0] >= MARGIN:
                break                                                   # cheapest covering run first: no need to try the taller ones
        m, run, blk, em, e32 = best
        assert run is not None, (entry, mutate, "applies to no run")
        print(f"planted {entry + '.' + mutate:<28} margin {m:10.3g}x on {blk:<12} (error {em:.1e}, e32 {e32:.1e}) run: {R.tag(run)}")
        assert m >= MARGIN, (entry, mutate, m, blk, R.tag(run))
        if m < smallest[0]:
            smallest = (m, f"{entry}.{mutate}")
    print(f"smallest margin {smallest[0]:.1f}x ({smallest[1]})")
