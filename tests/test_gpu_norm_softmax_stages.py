"""GPU: the LayerNorm entries of csrc/attention.hip, the two softmax stages of csrc/absorbed_attn.hip, the per-bag row
broadcast and its segment sum, each C entry on its own (raw ABI through _lib.lib()) against the float64 restatement of
tests/norm_softmax_ref.py, per block: max|got - ref| / max|ref| over a block <= k x max(e32, 1e-7), e32 being what the float32
restatement loses on the CPU over the same block.  tests/test_norm_softmax_sensitivity_host.py shows what these bounds see;
the k of each stage (norm_softmax_ref.K_STAGE) comes from the measured ratios in docs/lab_notes.md.  Every backward is fed the
float32 rounding of the float64 forward, as is the float32 restatement: one entry under test at a time.

Sentinels, compared bit for bit: 64 floats in front of and behind every output and workspace; every workspace is filled with
the sentinel first, and what the fold reads of it must have been written; the in-place softmax buffers carry three guard rows
behind the last group; padding columns come out as +0.0.  Every entry runs twice on the same inputs and must give the same
bits (there are no atomics)."""

import pytest
import torch

import norm_softmax_ref as N
from fused_attn_common import DEV, GUARD, SENT, _bits, _lib, _p, _st

pytestmark = pytest.mark.gpu

SENT_BITS = int(torch.tensor(SENT, dtype=torch.float32).view(torch.int32))
GUARD_ROWS = 3


class Buf:
    """numel floats on the device between GUARD sentinel floats in front and `tail` behind, all sentinel or `fill` inside."""

    def __init__(self, numel, fill=None, tail=GUARD):
        self.n = numel
        self.buf = torch.full((GUARD + numel + tail,), SENT, device=DEV, dtype=torch.float32)
        self.view = self.buf[GUARD:GUARD + numel]
        if fill is not None:
            self.view.copy_(fill.reshape(-1).to(torch.float32))
        self.p = _p(self.view)

    def intact(self):
        b = _bits(self.buf)
        return bool((b[:GUARD] == SENT_BITS).all()) and bool((b[GUARD + self.n:] == SENT_BITS).all())

    def untouched(self):
        return bool((_bits(self.buf) == SENT_BITS).all())

    def written(self, n=None):
        return bool((_bits(self.view[:self.n if n is None else n]) != SENT_BITS).all())

    def get(self, *shape):
        return self.view.detach().cpu().reshape(shape)


def _rows_buf(rows, ld, fill=None):
    """[rows, ld] with GUARD_ROWS sentinel rows behind it (and GUARD floats in front)."""
    return Buf(rows * ld, fill, tail=GUARD_ROWS * ld + GUARD)


def _dev(t):
    return t.to(torch.float32).contiguous().to(DEV)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _op(b):
    return None if b is None else b.p


def _twice(case, once):
    """once() -> {name: CPU tensor}; run twice, same bits."""
    a, b = once(), once()
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), f"{case}: {n} differs between two runs"
    return a


def _intact(case, **bufs):
    torch.cuda.synchronize()
    for n, b in bufs.items():
        assert b is None or b.intact(), f"{case}: wrote outside {n}"


def _pad_is_zero(case, t, live):
    if t.shape[1] > live:
        assert bool((_bits(t[:, live:]) == 0).all()), f"{case}: padding columns are not +0.0"


def test_plans_match_the_library():
    """The launch plans that the block maps are built from are the library's."""
    L = _lib()
    for rows in (1, 16, 17, 64, 65, 245, 1000, 1116, 8192, 8193, 8200, 40000):
        assert L.mil_layernorm_bwd_blocks(rows) == N.ln_bwd_nblocks(rows), rows
        assert L.mil_layernorm_bagrow_rows_per_block(rows) == N.ln_rows_per_blk(rows), rows
    for run in N.col_fwd_runs() + N.col_bwd_runs():
        G, m = len(run["lens"]), max(run["lens"])
        assert L.mil_grp_col_softmax_workspace_floats(G, m, run["ld"]) == N.col_ws_floats(G, m, run["ld"]), run


# --------------------------------------------------------------------------- LayerNorm
def _ln_inputs(run):
    c = N.ln_case(run["rows"], run["E"], run["x"], run["bags"])
    d = {n: _dev(c[n]) for n in ("x", "gamma", "beta", "dy", "dres")}
    d["stats"] = _dev(torch.stack([c["mean"], c["rstd"]], 1))
    if run["bags"] is not None:
        d.update(o=_dev(c["o"]), row_bag=_i32(c["row_bag"]), row_off=_i32(c["row_off"]))
    return d


def test_ln_fwd():
    """mil_layernorm_fwd and mil_layernorm_bagrow_fwd (B = 3): E 64 .. 512 (the generic kernel and the 16-byte one), rows 1, 3,
    5, 257 (the partial four-row workgroup); x = 100 + randn on every other run, one run with row scales 1e-3 .. 1e3; y, mean
    and rstd as tensors of their own; once with stats = NULL."""
    L = _lib()
    for run in N.ln_fwd_runs():
        rows, E, case, d = run["rows"], run["E"], N.tag(run), _ln_inputs(run)

        def once():
            y, stats = Buf(rows * E), Buf(rows * 2) if run["stats"] else None
            if run["bags"] is None:
                rc = L.mil_layernorm_fwd(_p(d["x"]), _p(d["gamma"]), _p(d["beta"]), rows, E, N.EPS, y.p, _op(stats), _st())
            else:
                rc = L.mil_layernorm_bagrow_fwd(_p(d["x"]), _p(d["o"]), _p(d["row_bag"]), _p(d["gamma"]), _p(d["beta"]), rows, E, N.EPS,
                                                y.p, _op(stats), _st())
            assert rc == 0, case
            _intact(case, y=y, stats=stats)
            got = {"y": y.get(rows, E)}
            if stats is not None:
                got["mean"], got["rstd"] = stats.get(rows, 2)[:, 0].contiguous(), stats.get(rows, 2)[:, 1].contiguous()
            return got
        N.hold("ln_fwd", case, _twice(case, once), N.run_ln_fwd(run), N.run_ln_fwd(run, torch.float32), N.run_ln_blocks(run))


def _ln_bwd_call(L, run, d, entry="res"):
    rows, E, case = run["rows"], run["E"], N.tag(run)
    nb = N.ln_bwd_nblocks(rows)
    dx = Buf(rows * E)
    dg, db, ws = (Buf(E), Buf(E), Buf(nb * 2 * E)) if run["params"] else (None, None, None)
    head = (_p(d["x"]), _p(d["gamma"]), _p(d["dy"]), _p(d["stats"]))
    tail = (rows, E, dx.p, _op(dg), _op(db), _op(ws), _st())
    if entry == "res":
        rc = L.mil_layernorm_bwd_res(*head, _p(d["dres"]) if run["dres"] else None, *tail)
    else:
        rc = L.mil_layernorm_bwd(*head, *tail)
    assert rc == 0, case
    _intact(case, dx=dx, dgamma=dg, dbeta=db, workspace=ws)
    if run["params"] and rows > N.LN_SMALL:
        assert ws.written(), f"{case}: the fold read a partial that no workgroup wrote"
    got = {"dx": dx.get(rows, E)}
    if run["params"]:
        got.update(dgamma=dg.get(E), dbeta=db.get(E))
    return got


@pytest.mark.parametrize("rows", N.LN_BWD_ROWS)
def test_ln_bwd(rows):
    """mil_layernorm_bwd_res: the one-workgroup kernel at 1, 16, 17, 63, 64 rows; the tiled one at 65, 1000 (63 partials: the
    fold's four-in-flight loop and its tail) and 8200 rows (512 workgroups of 17 rows, those behind row 8199 own nothing and
    must still write their partials); E 128 and 512, with and without dres, parameters trainable and frozen (dgamma = dbeta =
    workspace = NULL: dx alone is written)."""
    L = _lib()
    for run in N.ln_bwd_runs():
        if run["rows"] == rows:
            case, d = N.tag(run), _ln_inputs(run)
            got = _twice(case, lambda: _ln_bwd_call(L, run, d))
            N.hold("ln_bwd", case, got, N.run_ln_bwd(run), N.run_ln_bwd(run, torch.float32), N.run_ln_blocks(run))


def test_ln_bwd_is_bwd_res_without_dres():
    L = _lib()
    for run in N.ln_bwd_runs():
        if run["rows"] in (17, 1000) and run["E"] == 512 and run["params"] and not run["dres"]:
            d = _ln_inputs(run)
            a, b = _ln_bwd_call(L, run, d, "res"), _ln_bwd_call(L, run, d, "plain")
            for n in a:
                assert torch.equal(_bits(a[n]), _bits(b[n])), (N.tag(run), n)


@pytest.mark.parametrize("bags", N.BAGROW_BAGS, ids=lambda b: "-".join(map(str, b)))
def test_ln_bagrow_bwd(bags):
    """mil_layernorm_bagrow_bwd within its precondition: boundaries off the 16-row grid with a bag of one workgroup's length
    over two workgroups; a bag over 50 workgroups (the per-bag fold's four-in-flight loop); 8200 rows in ranges of 17.  d_o per
    bag and 64 columns."""
    L = _lib()
    for run in N.bagrow_bwd_runs():
        if run["bags"] != bags:
            continue
        rows, E, B, case, d = run["rows"], run["E"], len(bags), N.tag(run), _ln_inputs(run)
        assert min(bags) >= L.mil_layernorm_bagrow_rows_per_block(rows)

        def once():
            dx, d_o, dg, db = Buf(rows * E), Buf(B * E), Buf(E), Buf(E)
            ws = Buf(N.ln_bwd_nblocks(rows) * 4 * E)
            rc = L.mil_layernorm_bagrow_bwd(_p(d["x"]), _p(d["o"]), _p(d["row_bag"]), _p(d["row_off"]), B, _p(d["gamma"]), _p(d["dy"]),
                                            _p(d["stats"]), rows, E, dx.p, d_o.p, dg.p, db.p, ws.p, _st())
            assert rc == 0, case
            _intact(case, dx=dx, d_o=d_o, dgamma=dg, dbeta=db, workspace=ws)
            assert ws.written(len(N.ln_ranges(rows, True)) * 4 * E), f"{case}: the fold read a partial that no workgroup wrote"
            return {"dx": dx.get(rows, E), "d_o": d_o.get(B, E), "dgamma": dg.get(E), "dbeta": db.get(E)}
        N.hold("ln_bagrow_bwd", case, _twice(case, once), N.run_ln_bwd(run), N.run_ln_bwd(run, torch.float32), N.run_ln_blocks(run))


# --------------------------------------------------------------------------- column softmax
def _col_call(L, run, c, bwd, ws_on):
    """One call of the forward (in place) or backward; ws_on: through the *_ws entry with a sentinel-filled workspace."""
    off, ld, TH, G, case = c["off"], run["ld"], run["TH"], len(run["lens"]), N.tag(run)
    rows, goff = off[-1], _i32(off)
    wsf = N.col_ws_floats(G, run["hint"], ld)
    ws = Buf(max(wsf, 4096)) if ws_on else None
    if bwd:
        A, dA, out = _dev(c["A"]), _dev(c["dA"]), _rows_buf(rows, ld)
        if ws_on:
            rc = L.mil_grp_col_softmax_bwd_ws(_p(A), _p(dA), ld, _p(goff), G, run["hint"], TH, out.p, ws.p, _st())
        else:
            rc = L.mil_grp_col_softmax_bwd(_p(A), _p(dA), ld, _p(goff), G, run["hint"], TH, out.p, _st())
    else:
        out = _rows_buf(rows, ld, c["S"])
        if ws_on:
            rc = L.mil_grp_col_softmax_ws(out.p, ld, _p(goff), G, run["hint"], TH, ws.p, _st())
        else:
            rc = L.mil_grp_col_softmax(out.p, ld, _p(goff), G, run["hint"], TH, _st())
    assert rc == 0, case
    _intact(case, out=out, workspace=ws)
    if ws_on:
        assert ws.written(wsf) if wsf else ws.untouched(), f"{case}: workspace"
    got = out.get(rows, ld)
    _pad_is_zero(case, got, TH)
    return {"dS" if bwd else "A": got}


def _col_test(runs, stage, fn, bwd):
    L = _lib()
    for run in runs:
        case, c = N.tag(run), N.col_case(run["lens"], run["ld"], run["TH"], run["kind"])
        got = _twice(case, lambda: _col_call(L, run, c, bwd, run["ws"]))
        if run["ws"] and N.col_ws_plan(len(run["lens"]), run["hint"], run["ld"]) is None:
            one = _col_call(L, run, c, bwd, False)                  # G = 9: the workspace entry takes the one-launch form
            for n in got:
                assert torch.equal(_bits(got[n]), _bits(one[n])), f"{case}: differs from the one-launch form"
        N.hold(stage, case, got, fn(run), fn(run, torch.float32), N.run_col_blocks(run))


def test_col_softmax():
    """mil_grp_col_softmax / _ws: CW = 32, 8, 2 at 2048, 2049, 8193 rows, the re-reading loop at hint 0 and at 32 800 rows, the
    two-launch workspace form at G = 1 (2049 and 16 500 rows: 9 and the capped 64 chunks) and G = 3 (empty chunks), G = 9 with a
    workspace; a group of one row and one of none beside every one-launch group; ld 32 .. 128 and TH = 33 of ld = 40; 3 randn
    and a planted column maximum per route."""
    _col_test(N.col_fwd_runs(), "col_softmax", N.run_col_fwd, False)


def test_col_softmax_bwd():
    """mil_grp_col_softmax_bwd / _ws: the same at the backward's thresholds (1024, 1025, 4097 rows; 16 400 re-read)."""
    _col_test(N.col_bwd_runs(), "col_softmax_bwd", N.run_col_bwd, True)


# --------------------------------------------------------------------------- row softmax
def _row_test(stage, fn, bwd):
    L = _lib()
    for run in N.row_runs():
        R, ld, T, case = run["R"], run["ld"], run["T"], N.tag(run)
        c = N.row_case(R, ld, T, run["kind"])

        def once():
            if bwd:
                A, dA, out = _dev(c["A"]), _dev(c["dA"]), _rows_buf(R, ld)
                rc = L.mil_row_softmax_t_bwd(_p(A), _p(dA), ld, R, T, N.H, out.p, _st())
            else:
                out = _rows_buf(R, ld, c["S"])
                rc = L.mil_row_softmax_t(out.p, ld, R, T, N.H, _st())
            assert rc == 0, case
            _intact(case, out=out)
            got = out.get(R, ld)
            _pad_is_zero(case, got, T * N.H)
            return {"dS" if bwd else "A": got}
        N.hold(stage, case, _twice(case, once), fn(run), fn(run, torch.float32), N.run_row_blocks(run))


def test_row_softmax():
    """mil_row_softmax_t: T 1, 2, 10, 16 of H = 8, ld = T H and the next multiple of 32, R 1, 33, 1001 (R H no multiple of 256)."""
    _row_test("row_softmax", N.run_row_fwd, False)


def test_row_softmax_bwd():
    _row_test("row_softmax_bwd", N.run_row_bwd, True)


# --------------------------------------------------------------------------- segment sum
def test_segment_colsum():
    """mil_segment_colsum: bags of 1 .. 9, 0, 257 and 600 rows, E 64, 96, 512, max_rows 600; with a workspace three 256-row chunks
    (the last partial) and the fold, without one a single chunk."""
    L = _lib()
    for run in N.seg_runs():
        E, lens, case = run["E"], run["lens"], N.tag(run)
        B, Y, off = len(lens), _dev(N.seg_case(lens, E)), _i32(N.offsets(lens))

        def once():
            out = Buf(B * E)
            ws = Buf(3 * B * E) if run["ws"] else None
            rc = L.mil_segment_colsum(_p(Y), _p(off), B, run["max_rows"], E, out.p, _op(ws), _st())
            assert rc == 0, case
            _intact(case, out=out, workspace=ws)
            assert ws is None or ws.written(), f"{case}: the fold read a partial that no workgroup wrote"
            return {"out": out.get(B, E)}
        N.hold("segment_colsum", case, _twice(case, once), N.run_seg(run), N.run_seg(run, torch.float32), N.run_seg_blocks(run))


# --------------------------------------------------------------------------- single roundings and copies: bit for bit
BAGS = (5, 0, 7, 21)                 # 33 rows: 33 E / 4 = 528 float4 at E = 64, no multiple of 256


def test_add_pe_and_add_bag_row_bit_exact():
    L = _lib()
    rows, B = sum(BAGS), len(BAGS)
    bag, off = N.row_bag_of(BAGS), N.offsets(BAGS)
    for E in (64, 100):
        g = torch.Generator().manual_seed(E)
        x, pe, o = (torch.randn(s, generator=g) for s in ((rows, E), (max(BAGS), E), (B, E)))
        pos = torch.arange(rows) - torch.tensor(off)[bag]
        xd, ped, od, bagd, offd = _dev(x), _dev(pe), _dev(o), _i32(bag), _i32(off)
        out = Buf(rows * E)
        assert L.mil_add_pe(_p(xd), _p(ped), _p(bagd), _p(offd), rows, E, out.p, _st()) == 0
        _intact(f"add_pe E {E}", out=out)
        assert torch.equal(out.get(rows, E), x + pe[pos]), E
        out = Buf(rows * E)
        assert L.mil_add_bag_row(_p(xd), _p(od), _p(bagd), rows, E, out.p, _st()) == 0
        _intact(f"add_bag_row E {E}", out=out)
        assert torch.equal(out.get(rows, E), x + o[bag]), E


def test_embed_tokens_bit_exact():
    L = _lib()
    nseq, ctx, W, V = 3, 5, 64, 50                                  # 240 float4
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, V, (nseq, ctx), generator=g)
    table, pos = torch.randn((V, W), generator=g), torch.randn((ctx, W), generator=g)
    out = Buf(nseq * ctx * W)
    idd, td, pd = ids.to(DEV), _dev(table), _dev(pos)
    assert L.mil_embed_tokens(_p(idd), _p(td), _p(pd), nseq, ctx, W, out.p, _st()) == 0
    _intact("embed_tokens", out=out)
    assert torch.equal(out.get(nseq, ctx, W), table[ids] + pos)


@pytest.mark.parametrize("ctx", [5, 77])
def test_gather_eot_bit_exact(ctx):
    """The row at the largest id: at position 0, at the last position, a tie (the first wins) between two lanes and, at 77
    tokens, between two trips of one lane."""
    L = _lib()
    W, big = 96, 49407
    g = torch.Generator().manual_seed(ctx)
    ties = [(1, 3)] + ([(10, 40), (3, 67), (70, 6)] if ctx == 77 else [])
    nseq = 3 + len(ties)
    ids = torch.randint(0, 1000, (nseq, ctx), generator=g)
    ids[0, 0], ids[1, ctx - 1] = big, big
    ids[2, ctx // 2] = big
    want = [0, ctx - 1, ctx // 2]
    for i, (a, b) in enumerate(ties):
        ids[3 + i, a], ids[3 + i, b] = big, big
        want.append(min(a, b))
    x = torch.randn((nseq, ctx, W), generator=g)
    out = Buf(nseq * W)
    idd, xd = ids.to(DEV), _dev(x)
    assert L.mil_gather_eot(_p(idd), _p(xd), nseq, ctx, W, out.p, _st()) == 0
    _intact(f"gather_eot ctx {ctx}", out=out)
    assert torch.equal(out.get(nseq, W), x[torch.arange(nseq), torch.tensor(want)])
