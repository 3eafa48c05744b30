"""Restatements of the stages every fusion step runs between its attention kernels, for any float dtype: the LayerNorm
entries of csrc/attention.hip (plain and with the per-bag row o[row_bag] added on the way in), their backwards (residual
gradient, frozen parameters, per-bag column sums of dx), the two softmax stages of the multi-token absorbed attention
(csrc/absorbed_attn.hip: over the rows of each group per column, over the T tokens of each (row, head)) with their backwards,
and the per-bag column sum.  float64 is the reference, the same code in float32 on the CPU gives `e32`; mutate= plants one
error (tests/test_norm_softmax_sensitivity_host.py shows that the per-block bounds of tests/test_gpu_norm_softmax_stages.py
see each of them).  Every backward takes the forward's saved tensors as arguments, so the float32 rounding of the float64
forward can be fed to the entry and to both dtypes alike.  The module also holds the case lists, the launch plans as the
header documents them (the GPU test compares them with the library's) and the block maps.  Test-side helper: nothing here
reads the code under test."""
import functools

import torch

from transmil_ref import FLOOR, K_CAP, block_err, bound, flat_err  # noqa: F401  (re-exported to the test files)

EPS = 1e-5
SENT = -12345.678                    # what the GPU test fills outputs and workspaces with (fused_attn_common.SENT)
H = 8                                # heads of the absorbed attention
PEAK = 12.0                          # the planted column / token maximum of the peaked softmax cases
CHUNK = 256                          # rows of a block-map chunk of the column softmax, and of a partial of the segment sum
LN_SMALL = 64                        # rows up to which the LayerNorm backward is one workgroup

LN_FWD_MUTATIONS = ("onepass", "eps_outside", "var_e1", "wrong_bag")
LN_BWD_MUTATIONS = ("no_xhat_term", "skip_dres", "wg_last_row", "partial_lost", "stale_empty", "boundary_first_bag",
                    "bag_last_block")
COL_MUTATIONS = ("last_chunk_sum", "no_rescale", "max_first_chunk", "wrong_group", "pad_not_zeroed")
ROW_MUTATIONS = ("skip_last_token", "stride_T", "pad_not_zeroed")
SEG_MUTATIONS = ("skip_i4", "last_chunk")


def f32exact(t):
    return t.float().double()


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------- launch plans, as include/mil_hip.h states them
def ln_bwd_nblocks(rows):
    """mil_layernorm_bwd_blocks: 16 rows per workgroup, at most 512 workgroups."""
    return max(1, min(512, (rows + 15) // 16))


def ln_rows_per_blk(rows):
    """mil_layernorm_bagrow_rows_per_block, and the tiled backward's rows per workgroup."""
    nb = ln_bwd_nblocks(rows)
    return (rows + nb - 1) // nb


def ln_ranges(rows, tiled=None):
    """Row range of every backward workgroup that owns a row: one workgroup up to 64 rows (the bag-row form is always tiled)."""
    tiled = rows > LN_SMALL if tiled is None else tiled
    rpb = ln_rows_per_blk(rows) if tiled else rows
    return [(r, min(rows, r + rpb)) for r in range(0, rows, rpb)]


def col_ws_plan(G, max_rows, ld):
    """(nch, rch) of the workspace form of the column softmax, or None where the one-launch form is taken."""
    if G > 8 or max_rows <= 2048 or ld < 32 or ld > 128:
        return None
    nch = min(64, (max_rows + 255) // 256)
    return nch, (max_rows + nch - 1) // nch


def col_ws_floats(G, max_rows, ld):
    p = col_ws_plan(G, max_rows, ld)
    return 0 if p is None else G * p[0] * 2 * ld


def offsets(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def row_bag_of(lens):
    return torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))


# --------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, gamma, beta, eps=EPS, o=None, row_bag=None, mutate=None):
    """y = (u - mean) rstd gamma + beta over the last dim, u = x (+ o[row_bag]); biased variance, eps inside the root.
    "onepass": var = E[u^2] - mean^2 with the two moments exact and each rounded to float32 once (what the formula costs in
    float32 under any summation order); "wrong_bag": the first row of every later bag takes the o of the bag before it."""
    assert mutate is None or mutate in LN_FWD_MUTATIONS, mutate
    u = x
    if o is not None:
        rb = row_bag.clone()
        if mutate == "wrong_bag":
            first = torch.nonzero(rb[1:] != rb[:-1])[:, 0] + 1
            rb[first] = rb[first - 1]
        u = x + o[rb]
    n = u.shape[1]
    mean = u.mean(1, keepdim=True)
    if mutate == "onepass":
        m32, sq32 = mean.double().float(), (u.double() * u.double()).mean(1, keepdim=True).float()
        var = (sq32 - m32 * m32).clamp_min(0).to(u.dtype)
    else:
        d = u - mean
        var = (d * d).sum(1, keepdim=True) / (n - 1 if mutate == "var_e1" else n)
    rstd = 1 / (var.sqrt() + eps) if mutate == "eps_outside" else 1 / torch.sqrt(var + eps)
    return {"y": (u - mean) * rstd * gamma + beta, "mean": mean[:, 0], "rstd": rstd[:, 0]}


def ln_bwd(x, gamma, dy, mean, rstd, dres=None, params=True, o=None, row_bag=None, row_off=None, tiled=None, mutate=None):
    """xhat = (u - mean) rstd from the GIVEN statistics, g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres),
    dgamma = sum_rows dy xhat, dbeta = sum_rows dy (params), d_o[b] = sum of dx over the rows of bag b (with o).
    "wg_last_row": the last row of every workgroup's range does not enter dgamma / dbeta; "partial_lost": the middle
    workgroup's rows do not; "stale_empty": every workgroup behind the last row contributes the workspace's fill instead of
    zero; "boundary_first_bag": the first row of a bag that starts inside a workgroup's range is summed into the bag before
    it; "bag_last_block": the rows of a bag in the last workgroup that meets it are left out of d_o."""
    assert mutate is None or mutate in LN_BWD_MUTATIONS, mutate
    rows = x.shape[0]
    u = x if o is None else x + o[row_bag]
    xhat = (u - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    s1, s2 = g.mean(1, keepdim=True), (g * xhat).mean(1, keepdim=True)
    dx = rstd[:, None] * (g - s1 - (0 if mutate == "no_xhat_term" else xhat * s2))
    if dres is not None and mutate != "skip_dres":
        dx = dx + dres
    out = {"dx": dx}
    ranges = ln_ranges(rows, True if o is not None else tiled)
    if params:
        w = torch.ones(rows, 1, dtype=x.dtype)
        if mutate == "wg_last_row":
            w[[b - 1 for _, b in ranges]] = 0
        if mutate == "partial_lost":
            a, b = ranges[len(ranges) // 2]
            w[a:b] = 0
        out["dgamma"], out["dbeta"] = (w * dy * xhat).sum(0), (w * dy).sum(0)
        if mutate == "stale_empty":
            empty = ln_bwd_nblocks(rows) - len(ranges)
            out["dgamma"], out["dbeta"] = out["dgamma"] + empty * SENT, out["dbeta"] + empty * SENT
    if o is not None:
        rpb = ln_rows_per_blk(rows)
        d_o = torch.stack([dx[row_off[b]:row_off[b + 1]].sum(0) for b in range(len(row_off) - 1)])
        for b in range(len(row_off) - 1):
            lo, hi = row_off[b], row_off[b + 1]
            if mutate == "boundary_first_bag" and b > 0 and hi > lo and lo % rpb:
                d_o[int(row_bag[lo - 1])] += dx[lo]
                d_o[b] -= dx[lo]
            if mutate == "bag_last_block" and hi > lo:
                d_o[b] -= dx[max(lo, (hi - 1) // rpb * rpb):hi].sum(0)
        out["d_o"] = d_o
    return out


# --------------------------------------------------------------------------- the softmax stages
def _last_chunk(n):
    return CHUNK * ((n - 1) // CHUNK)


def grp_col_softmax(S, grp_off, TH, mutate=None):
    """A[r, c] = exp(S[r, c] - max) / sum over the rows r of the group, per column c < TH; columns >= TH are zero.
    "last_chunk_sum": the last (partial) 256-row chunk of a group does not enter the column sum; "no_rescale": the chunks'
    sums, each taken against its own maximum, are added as they are; "max_first_chunk": the rows are rewritten against the
    maximum of the first chunk, the sum taken against the true one; "pad_not_zeroed": the padding columns keep their input."""
    assert mutate is None or mutate in COL_MUTATIONS, mutate
    A = S.clone() if mutate == "pad_not_zeroed" else torch.zeros_like(S)
    for g in range(len(grp_off) - 1):
        r0, r1 = grp_off[g], grp_off[g + 1]
        if r1 <= r0:
            continue
        s = S[r0:r1, :TH]
        m = s.max(0).values
        e = torch.exp(s - m)
        l = e.sum(0)
        if mutate == "last_chunk_sum" and r1 - r0 > CHUNK:
            l = e[:_last_chunk(r1 - r0)].sum(0)
        if mutate == "no_rescale":
            l = sum(torch.exp(c - c.max(0).values).sum(0) for c in s.split(CHUNK))
        if mutate == "max_first_chunk":
            e = torch.exp(s - s[:CHUNK].max(0).values)
        A[r0:r1, :TH] = e / l
    return {"A": A}


def grp_col_softmax_bwd(A, dA, grp_off, TH, mutate=None):
    """dS = A (dA - sum_rows A dA) per (group, column < TH), zero behind.  "wrong_group": the sum of the next non-empty group."""
    assert mutate is None or mutate in COL_MUTATIONS, mutate
    dS = torch.full_like(A, SENT) if mutate == "pad_not_zeroed" else torch.zeros_like(A)
    live = [g for g in range(len(grp_off) - 1) if grp_off[g + 1] > grp_off[g]]
    cd = {g: (A[grp_off[g]:grp_off[g + 1], :TH] * dA[grp_off[g]:grp_off[g + 1], :TH]).sum(0) for g in live}
    for i, g in enumerate(live):
        r0, r1 = grp_off[g], grp_off[g + 1]
        c = cd[live[(i + 1) % len(live)]] if mutate == "wrong_group" else cd[g]
        dS[r0:r1, :TH] = A[r0:r1, :TH] * (dA[r0:r1, :TH] - c)
    return {"dS": dS}


def col_bwd_in_kernel_order(A, dA, n, TH, double_sum=True):
    """dS of the first group (n <= 1024 rows) in float32 numpy with the summation order of k_grp_col_softmax_bwd<32>: thread
    (row lane rl of 32, column) adds rows rl, rl + 32, .. in turn (fused multiply-add), lanes rl = 2 w and 2 w + 1 of wave w are
    added, then the 16 waves in turn.  double_sum: the sum in double and the tail a ((d - hi) - lo) on its two float parts, as
    the kernel has it; False: everything in float32, as it had it before (docs/lab_notes.md, fusion norm and softmax stages,
    finding 1)."""
    import numpy as np
    f, RL = np.float32, 32
    a = np.zeros((RL * 32, TH), f)
    d = np.zeros((RL * 32, TH), f)
    a[:n], d[:n] = A[:n, :TH].numpy().astype(f), dA[:n, :TH].numpy().astype(f)
    a3, d3 = a.reshape(32, RL, TH), d.reshape(32, RL, TH)                # [i, rl, c]: row rl + 32 i
    if double_sum:
        cd = (a3.astype(np.float64) * d3.astype(np.float64)).sum((0, 1))
        hi = cd.astype(f)
        lo = (cd - hi.astype(np.float64)).astype(f)
        out = a * ((d - hi).astype(f) - lo).astype(f)
    else:
        acc = np.zeros((RL, TH), f)
        for i in range(32):
            acc = (acc.astype(np.float64) + a3[i].astype(np.float64) * d3[i].astype(np.float64)).astype(f)
        wave = (acc[0::2] + acc[1::2]).astype(f)
        cd = wave[0]
        for w in range(1, 16):
            cd = (cd + wave[w]).astype(f)
        out = a * (d - cd).astype(f)
    dS = torch.zeros_like(A)
    dS[:n, :TH] = torch.from_numpy(out[:n].astype(np.float64))
    return {"dS": dS}


def _tok_view(S, T):
    return S[:, :T * H].reshape(S.shape[0], T, H)


def row_softmax_t(S, T, mutate=None):
    """Softmax over the T tokens of each (row, head): column t H + h; columns >= T H are zero.  "skip_last_token": token
    T - 1 does not enter the sum; "stride_T": token t of head h is read at column (h + t T) mod T H."""
    assert mutate is None or mutate in ROW_MUTATIONS, mutate
    A = S.clone() if mutate == "pad_not_zeroed" else torch.zeros_like(S)
    s = _tok_view(S, T)
    if mutate == "stride_T":
        idx = (torch.arange(H)[None, :] + T * torch.arange(T)[:, None]) % (T * H)
        s = S[:, idx.reshape(-1)].reshape(S.shape[0], T, H)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    l = e[:, :T - 1].sum(1, keepdim=True) if mutate == "skip_last_token" and T > 1 else e.sum(1, keepdim=True)
    A[:, :T * H] = (e / l).reshape(S.shape[0], T * H)
    return {"A": A}


def row_softmax_t_bwd(A, dA, T, mutate=None):
    assert mutate is None or mutate in ROW_MUTATIONS, mutate
    dS = torch.full_like(A, SENT) if mutate == "pad_not_zeroed" else torch.zeros_like(A)
    a, d = _tok_view(A, T), _tok_view(dA, T)
    if mutate == "stride_T":
        idx = (torch.arange(H)[None, :] + T * torch.arange(T)[:, None]) % (T * H)
        d = dA[:, idx.reshape(-1)].reshape(A.shape[0], T, H)
    cd = (a * d)[:, :T - 1].sum(1, keepdim=True) if mutate == "skip_last_token" and T > 1 else (a * d).sum(1, keepdim=True)
    dS[:, :T * H] = (a * (d - cd)).reshape(A.shape[0], T * H)
    return {"dS": dS}


def segment_colsum(Y, row_off, rows_per_chunk, mutate=None):
    """out[b] = sum of Y over the rows of bag b.  Chunks of rows_per_chunk rows from the bag's first row; inside a chunk
    four row lanes take rows i, i + 4 as a pair.  "skip_i4": the second row of every pair is skipped; "last_chunk": the rows
    behind the last full chunk boundary are."""
    assert mutate is None or mutate in SEG_MUTATIONS, mutate
    out = []
    for b in range(len(row_off) - 1):
        y = Y[row_off[b]:row_off[b + 1]]
        w = torch.ones(y.shape[0], 1, dtype=Y.dtype)
        k = torch.arange(y.shape[0]) % rows_per_chunk
        if mutate == "skip_i4":
            w[(k // 4) % 2 == 1] = 0
        if mutate == "last_chunk" and y.shape[0] > rows_per_chunk:
            w[rows_per_chunk * ((y.shape[0] - 1) // rows_per_chunk):] = 0
        out.append((w * y).sum(0))
    return {"out": torch.stack(out)}


# --------------------------------------------------------------------------- torch autograd of the same operations
def autograd_ln(x, gamma, beta, dy, dres=None, o=None, row_bag=None):
    t = {n: v.detach().clone().requires_grad_(True) for n, v in (("x", x), ("gamma", gamma), ("beta", beta), ("o", o)) if v is not None}
    u = t["x"] if o is None else t["x"] + t["o"][row_bag]
    y = torch.nn.functional.layer_norm(u, (x.shape[1],), t["gamma"], t["beta"], EPS)
    (y * dy).sum().backward() if dres is None else ((y * dy).sum() + (t["x"] * dres).sum()).backward()
    out = {"y": y.detach(), "dx": t["x"].grad, "dgamma": t["gamma"].grad, "dbeta": t["beta"].grad}
    if o is not None:
        out["d_o"] = t["o"].grad
    return out


def autograd_col_softmax(S, dA, grp_off, TH):
    s = S.detach().clone().requires_grad_(True)
    parts = [torch.softmax(s[grp_off[g]:grp_off[g + 1], :TH], 0) for g in range(len(grp_off) - 1)]
    A = torch.cat(parts)
    (A * dA[:, :TH]).sum().backward()
    return {"A": A.detach(), "dS": s.grad[:, :TH]}


def autograd_row_softmax(S, dA, T):
    s = S.detach().clone().requires_grad_(True)
    A = torch.softmax(_tok_view(s, T), 1).reshape(S.shape[0], T * H)
    (A * dA[:, :T * H]).sum().backward()
    return {"A": A.detach(), "dS": s.grad[:, :T * H]}


# --------------------------------------------------------------------------- block makers
def _cols64(E):
    return {f"c{j}": slice(64 * j, 64 * (j + 1)) for j in range(E // 64)}


def _row_sets(rows, ranges):
    out = {"all": slice(None), "first16": slice(0, min(16, rows)), "last16": slice(max(0, rows - 16), rows)}
    out.update({f"wg{i}": slice(a, b) for i, (a, b) in enumerate(ranges)})
    return out


def ln_blocks(rows, E, ranges, row_off=None):
    """[rows, E] tensors: all rows, the first and last 16, every backward workgroup's range, each over the 64-column groups;
    mean / rstd over the same row sets; dgamma, dbeta per 64 columns; d_o per bag and 64 columns."""
    rs, cs = _row_sets(rows, ranges), _cols64(E)
    mat = {f"{r}.{c}": (ri, ci) for r, ri in rs.items() for c, ci in cs.items()}
    vec = {r: (ri,) for r, ri in rs.items()}
    par = {c: (ci,) for c, ci in cs.items()}
    out = {"y": mat, "dx": mat, "mean": vec, "rstd": vec, "dgamma": par, "dbeta": par}
    if row_off is not None:
        out["d_o"] = {f"bag{b}.{c}": (b, ci) for b in range(len(row_off) - 1) for c, ci in cs.items()}
    return out


def col_blocks(grp_off, ld, TH, bwd=False):
    """Per (group, column) over all rows; per (group, 256-row chunk) over the live columns; the last partial chunk of each
    group; the padding columns (exactly zero).  bwd: a group of one row has A = 1 and dS = 1 (dA - dA), exactly zero."""
    out = {"all": (slice(None), slice(0, TH))}
    for g in range(len(grp_off) - 1):
        r0, r1 = grp_off[g], grp_off[g + 1]
        if r1 <= r0:
            continue
        if bwd and r1 - r0 == 1:
            out[f"zero_g{g}"] = (slice(r0, r1), slice(0, TH))
            continue
        out.update({f"g{g}.col{c}": (slice(r0, r1), c) for c in range(TH)})
        out.update({f"g{g}.chunk{j}": (slice(r0 + CHUNK * j, min(r1, r0 + CHUNK * (j + 1))), slice(0, TH))
                    for j in range((r1 - r0 + CHUNK - 1) // CHUNK)})
        out[f"g{g}.tail"] = (slice(r0 + _last_chunk(r1 - r0), r1), slice(0, TH))
    if ld > TH:
        out["pad"] = (slice(None), slice(TH, ld))
    return out


def row_blocks(R, ld, T):
    """Per head (its T columns); per 256 (row, head) threads = 32 rows of all heads; the padding columns (exactly zero)."""
    out = {"all": (slice(None), slice(0, T * H))}
    out.update({f"h{h}": (slice(None), slice(h, T * H, H)) for h in range(H)})
    out.update({f"t{j}": (slice(32 * j, min(R, 32 * (j + 1))), slice(0, T * H)) for j in range((R + 31) // 32)})
    if ld > T * H:
        out["pad"] = (slice(None), slice(T * H, ld))
    return out


def seg_blocks(lens, E):
    """Per bag and 64 columns (the last group partial); a bag without rows is exactly zero."""
    out = {"all": (Ellipsis,)}
    for b, n in enumerate(lens):
        out.update({f"{'bag' if n else 'empty'}{b}.c{j}": (b, slice(64 * j, min(E, 64 * (j + 1)))) for j in range((E + 63) // 64)})
    return out


def expected_zero(name):
    """The blocks whose reference is exactly zero: padding columns, the bag without rows, the backward of a one-row group."""
    return name.startswith(("pad", "empty", "zero"))


# --------------------------------------------------------------------------- the cases (shared by the host and GPU tests)
LN_E = (64, 128, 256, 512)
LN_FWD_ROWS = (1, 3, 5, 257)
LN_BWD_ROWS = (1, 16, 17, 63, 64, 65, 1000, 8200)
LN_BWD_E = (128, 512)
BAGROW_BAGS = ((70, 16, 16, 143), (800, 16, 300), (5000, 17, 3183))
BAGROW_E = (256, 512)
COL_LDTH = ((32, 24), (96, 80), (96, 96), (128, 96), (128, 80), (40, 33))     # (ld, TH): T = 3, 10, 12 of H = 8, and the raw 33 of 40
ROW_T = (1, 2, 10, 16)
ROW_R = (1, 33, 1001)
SEG_BAGS = (1, 3, 4, 5, 8, 9, 0, 257, 600)
SEG_E = (64, 96, 512)


def fwd_bags(rows):
    """Three bags over `rows` rows (the later ones empty where the rows run out)."""
    return (rows - 2 * (rows // 3), rows // 3, rows // 3)


def ln_fwd_runs():
    """x = 100 + randn on every other run, one run with row scales 1e-3 .. 1e3, one without stats."""
    out = []
    for i, E in enumerate(LN_E):
        for j, rows in enumerate(LN_FWD_ROWS):
            for bag in (False, True):
                kind = "scales" if (E, rows, bag) == (256, 257, False) else ("m100" if (i + j + bag) % 2 == 0 else "unit")
                out.append(dict(E=E, rows=rows, bags=fwd_bags(rows) if bag else None, x=kind,
                                stats=(E, rows, bag) != (128, 5, False)))
    return out


def ln_bwd_runs():
    out = []
    for i, rows in enumerate(LN_BWD_ROWS):
        for j, E in enumerate(LN_BWD_E):
            for dres in (False, True):
                for params in (True, False):
                    out.append(dict(E=E, rows=rows, bags=None, x="m100" if (i + j + dres) % 2 == 0 else "unit", dres=dres,
                                    params=params))
    return out


def bagrow_bwd_runs():
    return [dict(E=E, rows=sum(b), bags=b, x="m100" if (i + j) % 2 == 0 else "unit", dres=False, params=True)
            for i, b in enumerate(BAGROW_BAGS) for j, E in enumerate(BAGROW_E)]


def _col_runs(routes):
    out = []
    for i, (lens, hint, ws, ldth) in enumerate(routes):
        for k, kind in enumerate(("randn3", "peaked")):
            ld, TH = COL_LDTH[(2 * i + k) % len(COL_LDTH)] if ldth is None else ldth
            out.append(dict(lens=lens, ld=ld, TH=TH, hint=max(lens) if hint is None else hint, ws=ws, kind=kind))
    return out


WS_ROUTES = (((2049,), None, True, None), ((2600, 2100, 4000), None, True, None), ((16500,), None, True, None),
             ((2049, 300, 1, 0, 257, 256, 255, 513, 100), None, True, None))


def col_fwd_runs():
    """(lens, hint, workspace, (ld, TH) or the cycle): CW = 32, 8, 2 at the smallest length that selects them; the re-reading
    loop at hint 0 and behind 32 768 rows; the four workspace cases (the last, G = 9, falls back to one launch)."""
    return _col_runs((((2048, 1, 0), None, False, None), ((2049, 1, 0), None, False, None), ((8193, 1, 0), None, False, None),
                      ((2049, 1, 0), 0, False, None), ((32800, 1, 0), None, False, (32, 24))) + WS_ROUTES)


def col_bwd_runs():
    return _col_runs((((1024, 1, 0), None, False, None), ((1025, 1, 0), None, False, None), ((4097, 1, 0), None, False, None),
                      ((1025, 1, 0), 0, False, None), ((16400, 1, 0), None, False, (32, 24))) + WS_ROUTES)


def row_runs():
    out = []
    for i, T in enumerate(ROW_T):
        for ld in dict.fromkeys((T * H, 32 * ((T * H + 31) // 32))):
            for j, R in enumerate(ROW_R):
                out.append(dict(T=T, ld=ld, R=R, kind=("randn3", "peaked")[(i + j + (ld > T * H)) % 2]))
    return out


def seg_runs():
    """max_rows = 600: the workspace form sums three 256-row chunks (the last partial), without one a single chunk."""
    return [dict(E=E, lens=SEG_BAGS, ws=ws, max_rows=600) for E in SEG_E for ws in (True, False)]


@functools.lru_cache(maxsize=16)
def ln_case(rows, E, kind, bags=None):
    """float32-exact inputs in float64.  kind "m100": x = 100 + randn (variance by subtraction would lose it); "unit": randn
    + 0.5; "scales": randn rows scaled 1e-3 .. 1e3.  gamma = 1 + 0.1 randn, beta = 0.1 randn; with bags o [B, E] randn."""
    g = _gen(rows, E, len(kind), 0 if bags is None else len(bags) + 1)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)                          # noqa: E731
    x = r(rows, E)
    if kind == "m100":
        x = x + 100.0
    elif kind == "unit":
        x = x + 0.5
    else:
        x = x * torch.logspace(-3, 3, rows, dtype=torch.float64)[:, None]
    c = dict(x=x, gamma=1.0 + 0.1 * r(E), beta=0.1 * r(E), dy=r(rows, E), dres=r(rows, E))
    if bags is not None:
        c["o"] = r(len(bags), E)
    c = {n: f32exact(t) for n, t in c.items()}
    if bags is not None:
        c["row_bag"], c["row_off"] = row_bag_of(bags), offsets(bags)
    f = ln_fwd(c["x"], c["gamma"], c["beta"], EPS, c.get("o"), c.get("row_bag"))
    c["mean"], c["rstd"] = f32exact(f["mean"]), f32exact(f["rstd"])          # what the backward is fed
    return c


def run_ln_fwd(run, dtype=torch.float64, mutate=None):
    c = ln_case(run["rows"], run["E"], run["x"], run["bags"])
    t = lambda n: c[n].to(dtype) if n in c else None                                         # noqa: E731
    return ln_fwd(t("x"), t("gamma"), t("beta"), EPS, t("o"), c.get("row_bag"), mutate)


def run_ln_bwd(run, dtype=torch.float64, mutate=None):
    c = ln_case(run["rows"], run["E"], run["x"], run["bags"])
    t = lambda n: c[n].to(dtype) if n in c else None                                         # noqa: E731
    return ln_bwd(t("x"), t("gamma"), t("dy"), t("mean"), t("rstd"), t("dres") if run["dres"] else None, run["params"], t("o"),
                  c.get("row_bag"), c.get("row_off"), mutate=mutate)


def run_ln_blocks(run):
    bag = run["bags"] is not None
    return ln_blocks(run["rows"], run["E"], ln_ranges(run["rows"], True if bag and "dres" in run else None),
                     offsets(run["bags"]) if bag else None)


@functools.lru_cache(maxsize=8)
def col_case(lens, ld, TH, kind):
    """S [rows, ld] (padding columns 7 + randn: never read, and zero afterwards), dA [rows, ld], A = the float32 rounding of
    the float64 forward.  "randn3": 3 randn; "peaked": randn with PEAK planted per (group, column) - in the group's last
    partial 256-row chunk for the even columns, in its row 0 for the odd ones."""
    off = offsets(lens)
    g = _gen(sum(lens), ld, TH, len(kind), len(lens))
    S = torch.randn((off[-1], ld), generator=g, dtype=torch.float64) * (3.0 if kind == "randn3" else 1.0)
    dA = torch.randn((off[-1], ld), generator=g, dtype=torch.float64)
    S[:, TH:] += 7.0
    if kind == "peaked":
        for i, n in enumerate(lens):
            for c in range(TH if n else 0):
                t0 = _last_chunk(n)
                S[off[i] + (t0 + (5 * c) % (n - t0) if c % 2 == 0 else 0), c] = PEAK
    S, dA = f32exact(S), f32exact(dA)
    return dict(S=S, dA=dA, A=f32exact(grp_col_softmax(S, off, TH)["A"]), off=off)


def run_col_fwd(run, dtype=torch.float64, mutate=None):
    c = col_case(run["lens"], run["ld"], run["TH"], run["kind"])
    return grp_col_softmax(c["S"].to(dtype), c["off"], run["TH"], mutate)


def run_col_bwd(run, dtype=torch.float64, mutate=None):
    c = col_case(run["lens"], run["ld"], run["TH"], run["kind"])
    return grp_col_softmax_bwd(c["A"].to(dtype), c["dA"].to(dtype), c["off"], run["TH"], mutate)


def run_col_blocks(run):
    off = offsets(run["lens"])
    return {"A": col_blocks(off, run["ld"], run["TH"]), "dS": col_blocks(off, run["ld"], run["TH"], True)}


@functools.lru_cache(maxsize=None)
def row_case(R, ld, T, kind):
    """As col_case over the tokens: "peaked" plants PEAK at token T - 1 of the even (row, head) threads, at token 0 of the odd."""
    g = _gen(R, ld, T, len(kind))
    S = torch.randn((R, ld), generator=g, dtype=torch.float64) * (3.0 if kind == "randn3" else 1.0)
    dA = torch.randn((R, ld), generator=g, dtype=torch.float64)
    S[:, T * H:] += 7.0
    if kind == "peaked":
        idx = torch.arange(R * H).reshape(R, H)
        v = _tok_view(S, T).clone()
        v[:, T - 1][idx % 2 == 0] = PEAK
        v[:, 0][idx % 2 == 1] = PEAK
        S[:, :T * H] = v.reshape(R, T * H)
    S, dA = f32exact(S), f32exact(dA)
    return dict(S=S, dA=dA, A=f32exact(row_softmax_t(S, T)["A"]))


def run_row_fwd(run, dtype=torch.float64, mutate=None):
    return row_softmax_t(row_case(run["R"], run["ld"], run["T"], run["kind"])["S"].to(dtype), run["T"], mutate)


def run_row_bwd(run, dtype=torch.float64, mutate=None):
    c = row_case(run["R"], run["ld"], run["T"], run["kind"])
    return row_softmax_t_bwd(c["A"].to(dtype), c["dA"].to(dtype), run["T"], mutate)


def run_row_blocks(run):
    b = row_blocks(run["R"], run["ld"], run["T"])
    if run["T"] > 1:
        return {"A": b, "dS": b}
    # one token: A = 1 and dS = 1 (dA - dA), exactly zero
    return {"A": b, "dS": {("zero_" + n if n != "pad" else n): ix for n, ix in b.items()}}


@functools.lru_cache(maxsize=None)
def seg_case(lens, E):
    return f32exact(torch.randn((sum(lens), E), generator=_gen(sum(lens), E, 3), dtype=torch.float64) + 0.25)


def run_seg(run, dtype=torch.float64, mutate=None):
    return segment_colsum(seg_case(run["lens"], run["E"]).to(dtype), offsets(run["lens"]), CHUNK if run["ws"] else run["max_rows"], mutate)


def run_seg_blocks(run):
    return {"out": seg_blocks(run["lens"], run["E"])}


def tag(run):
    return " ".join(f"{k} {'-'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in run.items())


# k of bound(e32, k) per stage: the next power of two above twice the largest ratio gpu_err / max(e32, 1e-7) that the first
# full run on an MI355X showed at the cap (the table "fusion norm and softmax stages" in docs/lab_notes.md), capped at K_CAP
K_STAGE = {"ln_fwd": 4, "ln_bwd": 4, "ln_bagrow_bwd": 4, "col_softmax": 16, "col_softmax_bwd": 4, "row_softmax": 8,
           "row_softmax_bwd": 2, "segment_colsum": 4}


def hold(stage, case, got, ref, r32, blocks):
    """Every block of every tensor of `got` within bound(e32, K_STAGE[stage]) of `ref`; prints the worst block per tensor
    first.  A block whose reference is all zero is met exactly or not at all (block_err)."""
    bad, worst = [], 0.0
    for t in got:
        e32, eg = block_err(r32[t], ref[t], blocks[t]), block_err(got[t], ref[t], blocks[t])
        w = max(eg, key=lambda b: eg[b] / max(e32[b], FLOOR))
        ratio = eg[w] / max(e32[w], FLOOR)
        worst = max(worst, ratio)
        print(f"RATIO | {stage} | {case} | {t}.{w} | gpu {eg[w]:.2e} | e32 {e32[w]:.2e} | {ratio:.2f}")
        bad += [(t, b, e, e32[b]) for b, e in eg.items() if not e <= bound(e32[b], K_STAGE[stage])]
    assert not bad, (stage, case, bad[:8])
    return worst
