"""CPU: what the per-block bounds of tests/test_gpu_norm_softmax_stages.py can see.

The GPU bound of a block is k x max(e32, 1e-7), k <= 16, with e32 the error of the float32 restatement of the same entry on
the CPU against float64 (tests/norm_softmax_ref.py).  Over the GPU file's own run lists, inputs and blocks:
  a. the closed forms equal torch autograd to 1e-12 in float64;
  b. every block has a non-zero reference and a finite float32 restatement, except the padding columns of the two softmax
     stages and the bag without rows of the segment sum, which are exactly zero in both;
  c. every planted error (mutate= of the restatement), measured in float64 against the clean float64 result, exceeds the
     bound at the cap k = 16 by a factor of 10 on at least one block of at least one run.
pytest -s lists the covering run, block and margin of every planted error and the smallest margin.  Nothing here reads the
code under test."""
import math

import torch

import norm_softmax_ref as N

MARGIN = 10.0

# stage -> (runs, restatement of a run, blocks of a run)
STAGES = {
    "ln_fwd": (N.ln_fwd_runs(), N.run_ln_fwd, N.run_ln_blocks),
    "ln_bwd": (N.ln_bwd_runs(), N.run_ln_bwd, N.run_ln_blocks),
    "ln_bagrow_bwd": (N.bagrow_bwd_runs(), N.run_ln_bwd, N.run_ln_blocks),
    "col_softmax": (N.col_fwd_runs(), N.run_col_fwd, N.run_col_blocks),
    "col_softmax_bwd": (N.col_bwd_runs(), N.run_col_bwd, N.run_col_blocks),
    "row_softmax": (N.row_runs(), N.run_row_fwd, N.run_row_blocks),
    "row_softmax_bwd": (N.row_runs(), N.run_row_bwd, N.run_row_blocks),
    "segment_colsum": (N.seg_runs(), N.run_seg, N.run_seg_blocks),
}


def _tiled(r):
    return r["rows"] > N.LN_SMALL


def _chunks(r):
    return max(r["lens"]) > N.CHUNK


# (stage, planted error, the runs it applies to); the 8200-row LayerNorm runs are left to the one error that needs them
PLANTED = [
    ("ln_fwd", "onepass", lambda r: True),
    ("ln_fwd", "eps_outside", lambda r: True),
    ("ln_fwd", "var_e1", lambda r: True),
    ("ln_fwd", "wrong_bag", lambda r: r["bags"] is not None and r["rows"] > 1),
    ("ln_bwd", "no_xhat_term", lambda r: r["rows"] <= 1000),
    ("ln_bwd", "skip_dres", lambda r: r["dres"] and r["rows"] <= 1000),
    ("ln_bwd", "wg_last_row", lambda r: r["params"] and r["rows"] <= 1000),
    ("ln_bwd", "partial_lost", lambda r: r["params"] and _tiled(r) and r["rows"] <= 1000),
    ("ln_bwd", "stale_empty", lambda r: r["params"] and r["rows"] == 8200),
    ("ln_bagrow_bwd", "boundary_first_bag", lambda r: r["rows"] <= 1200),
    ("ln_bagrow_bwd", "bag_last_block", lambda r: r["rows"] <= 1200),
    ("col_softmax", "last_chunk_sum", _chunks),
    ("col_softmax", "no_rescale", _chunks),
    ("col_softmax", "max_first_chunk", _chunks),
    ("col_softmax", "pad_not_zeroed", lambda r: r["ld"] > r["TH"]),
    ("col_softmax_bwd", "wrong_group", lambda r: sum(n > 0 for n in r["lens"]) > 1),
    ("col_softmax_bwd", "pad_not_zeroed", lambda r: r["ld"] > r["TH"]),
    ("row_softmax", "skip_last_token", lambda r: r["T"] > 1),
    ("row_softmax", "stride_T", lambda r: r["T"] not in (1, N.H)),
    ("row_softmax", "pad_not_zeroed", lambda r: r["ld"] > r["T"] * N.H),
    ("row_softmax_bwd", "skip_last_token", lambda r: r["T"] > 1),
    ("row_softmax_bwd", "stride_T", lambda r: r["T"] not in (1, N.H)),
    ("segment_colsum", "skip_i4", lambda r: True),
    ("segment_colsum", "last_chunk", lambda r: r["ws"]),
]


def _margin(mut, ref, r32, blocks):
    best = (0.0, None, 0.0, 0.0)
    for t in mut:
        e32, em = N.block_err(r32[t], ref[t], blocks[t]), N.block_err(mut[t], ref[t], blocks[t])
        for b in em:
            m = em[b] / N.bound(e32[b], N.K_CAP)
            if m > best[0]:
                best = (m, f"{t}.{b}", em[b], e32[b])
    return best


def _equal(got, want, what):
    err = N.block_err(got, want, {"all": (Ellipsis,)})["all"]
    assert err <= 1e-12, (what, err)


def test_closed_forms_equal_autograd():
    for rows, E, kind, bags in ((5, 64, "unit", None), (65, 128, "unit", None), (257, 512, "scales", None), (245, 256, "unit", (70, 16, 16, 143))):
        c = N.ln_case(rows, E, kind, bags)
        dres = c["dres"] if bags is None else None                    # the bag-row form has no residual gradient
        ag = N.autograd_ln(c["x"], c["gamma"], c["beta"], c["dy"], dres, c.get("o"), c.get("row_bag"))
        f = N.ln_fwd(c["x"], c["gamma"], c["beta"], N.EPS, c.get("o"), c.get("row_bag"))
        b = N.ln_bwd(c["x"], c["gamma"], c["dy"], f["mean"], f["rstd"], dres, True, c.get("o"), c.get("row_bag"), c.get("row_off"))
        _equal(f["y"], ag["y"], (rows, E, "y"))
        for n in b:
            _equal(b[n], ag[n], (rows, E, n))
    # the softmax backwards on the 3 randn cases: behind a planted peak dS is a difference of nearly equal terms, and two
    # float64 evaluations of it agree to 1e-16 of the inputs, not to 1e-12 of dS
    for run in (N.col_fwd_runs()[0], N.col_fwd_runs()[10], N.col_fwd_runs()[16]):
        c, TH = N.col_case(run["lens"], run["ld"], run["TH"], run["kind"]), run["TH"]
        ag = N.autograd_col_softmax(c["S"], c["dA"], c["off"], TH)
        A = N.grp_col_softmax(c["S"], c["off"], TH)["A"]
        _equal(A[:, :TH], ag["A"], (run, "A"))
        _equal(N.grp_col_softmax_bwd(A, c["dA"], c["off"], TH)["dS"][:, :TH], ag["dS"], (run, "dS"))
    for run in [r for r in N.row_runs() if r["kind"] == "randn3"][::2]:
        c, TT = N.row_case(run["R"], run["ld"], run["T"], run["kind"]), run["T"] * N.H
        ag = N.autograd_row_softmax(c["S"], c["dA"], run["T"])
        A = N.row_softmax_t(c["S"], run["T"])["A"]
        _equal(A[:, :TT], ag["A"], (run, "A"))
        _equal(N.row_softmax_t_bwd(A, c["dA"], run["T"])["dS"][:, :TT], ag["dS"], (run, "dS"))
    for run in N.seg_runs():
        Y, off = N.seg_case(run["lens"], run["E"]), N.offsets(run["lens"])
        want = torch.zeros(len(run["lens"]), run["E"], dtype=torch.float64).index_add_(0, N.row_bag_of(run["lens"]), Y)
        assert off[-1] == Y.shape[0]
        _equal(N.run_seg(run)["out"], want, run)


def test_every_block_has_teeth():
    """(b): no block but the padding columns and the bag without rows has an all-zero reference; those are exactly zero in
    both dtypes."""
    for stage, (runs, fn, blocks_of) in STAGES.items():
        n, nzero, worst = 0, 0, 0.0
        for run in runs:
            ref, r32, blocks = fn(run), fn(run, torch.float32), blocks_of(run)
            for t in ref:
                e32 = N.block_err(r32[t], ref[t], blocks[t])
                for name, ix in blocks[t].items():
                    if ref[t][ix].numel() == 0:
                        continue
                    top = float(ref[t][ix].abs().max())
                    if N.expected_zero(name):
                        assert top == 0.0 and e32[name] == 0.0, (stage, run, t, name, top)
                        nzero += 1
                    else:
                        assert top > 0.0 and math.isfinite(top) and math.isfinite(e32[name]), (stage, run, t, name, top)
                n += len(e32)
                worst = max(worst, max(e32.values()))
        print(f"stage {stage:<16} {len(runs):3d} runs, {n:6d} blocks ({nzero} exactly zero), worst e32 {worst:.1e}")


def test_planted_errors_exceed_the_bounds():
    smallest = (math.inf, None)
    for stage, mutate, applies in PLANTED:
        runs, fn, blocks_of = STAGES[stage]
        best = (0.0, None, None, 0.0, 0.0)
        for run in runs:
            if not applies(run):
                continue
            m, blk, em, e32 = _margin(fn(run, torch.float64, mutate), fn(run), fn(run, torch.float32), blocks_of(run))
            if m > best[0]:
                best = (m, run, blk, em, e32)
        m, run, blk, em, e32 = best
        assert run is not None, (stage, mutate, "applies to no run")
        print(f"planted {stage + '.' + mutate:<36} margin {m:12.1f}x on {blk:<18} (error {em:.1e}, e32 {e32:.1e}) run: {N.tag(run)}")
        assert m >= MARGIN, (stage, mutate, m, blk, run)
        if m < smallest[0]:
            smallest = (m, f"{stage}.{mutate}")
    print(f"smallest margin {smallest[0]:.1f}x ({smallest[1]})")


def test_plans_cover_the_routes():
    """The case lists reach what the issue names: 63 partials, 512 workgroups of 17 rows with empty ones behind, a bag over
    at least 49 workgroups, every bag at least one workgroup long, and the workspace plans 9 / 16 / 64 chunks."""
    assert N.ln_bwd_nblocks(1000) == 63 and (N.ln_bwd_nblocks(8200), N.ln_rows_per_blk(8200)) == (512, 17)
    assert len(N.ln_ranges(8200)) == 483 and len(N.ln_ranges(64)) == 1 and len(N.ln_ranges(65)) == 5
    for bags in N.BAGROW_BAGS:
        rpb = N.ln_rows_per_blk(sum(bags))
        assert min(bags) >= rpb, bags
    assert N.ln_rows_per_blk(245) == 16 and N.ln_rows_per_blk(1116) == 16 and 800 // 16 >= 49
    assert N.col_ws_plan(1, 2049, 96) == (9, 228) and N.col_ws_plan(3, 4000, 96) == (16, 250) and N.col_ws_plan(1, 16500, 96) == (64, 258)
    assert N.col_ws_plan(9, 2049, 96) is None and N.col_ws_plan(1, 2048, 96) is None


def test_col_softmax_bwd_in_the_kernels_summation_order():
    """sum_rows A dA of mil_grp_col_softmax_bwd in float32 numpy, rows added in the kernel's order
    (norm_softmax_ref.col_bwd_in_kernel_order), on the 1024-row peaked run: with the sum in double and the tail on its two
    float parts every block of the group is within the bound at the stage's k; with the float32 sum the kernel had before, the
    column blocks behind a planted maximum are not within the cap (A = 0.98 there, dS of that row is a difference of nearly
    equal terms, and every row added behind the large one rounds at its size: lab notes, finding 1)."""
    run = next(r for r in N.col_bwd_runs() if r["lens"][0] == 1024 and r["kind"] == "peaked")
    c, n, TH = N.col_case(run["lens"], run["ld"], run["TH"], run["kind"]), run["lens"][0], run["TH"]
    ref, r32 = N.run_col_bwd(run), N.run_col_bwd(run, torch.float32)
    blocks = {b: ix for b, ix in N.run_col_blocks(run)["dS"].items() if b.startswith("g0.")}
    e32 = N.block_err(r32["dS"], ref["dS"], blocks)
    worst = {}
    for double_sum in (True, False):
        eg = N.block_err(N.col_bwd_in_kernel_order(c["A"], c["dA"], n, TH, double_sum)["dS"], ref["dS"], blocks)
        b = max(eg, key=lambda k: eg[k] / max(e32[k], N.FLOOR))
        worst[double_sum] = eg[b] / max(e32[b], N.FLOOR)
        print(f"kernel order, {'sum in double' if double_sum else 'float32 sum'}: largest ratio {worst[double_sum]:.2f} on dS.{b} "
              f"(error {eg[b]:.2e}, e32 {e32[b]:.2e})")
    assert worst[True] <= N.K_STAGE["col_softmax_bwd"] and worst[False] > N.K_CAP
