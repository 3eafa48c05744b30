"""CPU: the route the library plans for the tiled fp32 linear (mil_gemm_route, mil_linear_bwd_params_route: the plans its
launches execute) against the rules restated in tests/linear_ref.py, field by field, over shapes that bracket every
threshold of the dispatch at 64, 256 and 304 compute units; and the workspace queries against the routes' needs.  Host
arithmetic only: with ncu > 0 the queries make no device call."""
import ctypes

import pytest

import linear_ref as R

NCUS = (64, 256, 304)
NS = (64, 132, 512, 520, 2048)
KS = (32, 64, 128, 224, 256, 288, 512, 2048)
MODES = ((0, 0), (0, 1), (1, 1))
# (residual, aligned16): a residual or an unaligned operand is what keeps a shape off the NT2 kernel
VARIANTS = ((False, True), (False, False), (True, True))


def _around(v):
    return [v - 1, v, v + 1]


def sweep_rows(N, ncu):
    """M on both sides of every threshold of the dispatch for this N and CU count."""
    ct, ct64, slots = -(-N // 128), -(-N // 64), 2 * ncu
    ms = {1, 4, 63, 64, 65, 2047, 2048, 2049, 2052}
    for tiles, cols in ((3 * ncu // 2, ct), (ncu // 2, ct), (16, ct64)):                     # t64, the bucketed t64, t
        rt = -(-tiles // cols)
        ms.update(m for r in (rt - 1, rt) for m in _around(64 * r) if m > 0)
    if N % 256 == 0:                                                                         # the NT2 fill rule
        for tiles in (3 * ncu // 4, 7 * ncu // 8, ncu, 7 * ncu // 4, 2 * ncu):
            rt = -(-tiles // (N // 256))
            ms.update(m for r in (rt - 1, rt, rt + 1) for m in (256 * r - 255, 256 * r) if m > 0)
    if ct <= slots:                                                                          # whole rounds +- 1 tile, 0.7 of a round
        per = slots // ct
        full = (7 * slots) // (10 * ct)
        for rounds in (1, 2):
            base = rounds * per
            for r in (base - 1, base, base + 1, base + 2, base + full, base + full + 1, base + per // 2):
                ms.update((128 * r - 127, 128 * r))
    return sorted(m for m in ms if 0 < m <= 80000)


def _lib():
    from mil_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("ncu", NCUS)
def test_gemm_route_equals_the_rules(ncu):
    seen, n = set(), 0
    for N in NS:
        for M in sweep_rows(N, ncu):
            for K in KS:
                for a_mode, b_mode in MODES:
                    if a_mode == 1 and M % 4:
                        continue
                    for ws in (True, False):
                        for bucketed in ((False, True) if a_mode == 0 else (False,)):
                            for res, al in VARIANTS:
                                kw = dict(a_mode=a_mode, b_mode=b_mode, act=1, residual=res, workspace=ws, bucketed=bucketed,
                                          aligned16=al, ncu=ncu)
                                got, want = R.lib_gemm_route(M, N, K, **kw), R.gemm_route(M, N, K, **kw)
                                assert got == want, (M, N, K, kw, got, want)
                                seen.add((got["kernel"], got["S"] > 1))
                                n += 1
    want = {("NT2", False), ("G64", False), ("G64N", False), ("G64N", True), ("TAIL", True), ("NT", False), ("NT", True),
            ("NN", False), ("NN", True), ("TN", False), ("TN", True)}
    assert seen == want, (ncu, sorted(want - seen), sorted(seen - want))
    print(f"ncu {ncu}: {n} shapes, every kernel form met")


def test_gemm_route_reads_the_other_arguments():
    """What else keeps a shape off the NT2 kernel, and what the query refuses."""
    M, N, K = 7168, 2048, 64
    assert R.lib_gemm_route(M, N, K)["kernel"] == R.gemm_route(M, N, K)["kernel"] == "NT2"
    for kw in (dict(act=3), dict(accumulate=True), dict(aux_mode=1), dict(aux_mode=2), dict(ldc=N - 4), dict(lda=K + 4), dict(bucketed=True),
               dict(lda=1 << 22)):
        got, want = R.lib_gemm_route(M, N, K, **kw), R.gemm_route(M, N, K, **kw)
        assert got == want and (got["kernel"] == "NT") == (kw != dict(lda=K + 4)), (kw, got, want)
    lib, p = _lib(), ctypes.create_string_buffer(64)
    for args in ((0, 512, 64, 0, 0), (64, 512, 48, 0, 0), (66, 512, 64, 1, 1), (64, 130, 64, 0, 1), (64, 512, 64, 1, 0)):
        M, N, K, a, b = args
        assert lib.mil_gemm_route(M, N, K, a, b, K if a == 0 else M, K if b == 0 else N, N, 0, 0, 0, 0, 1, 0, 1, 256, p) == -22, args
    assert lib.mil_gemm_route(64, 512, 64, 0, 0, 64, 64, 512, 0, 0, 0, 0, 1, 0, 1, 256, None) == -22
    assert lib.mil_gemm_route(64, 512, 64, 1, 1, 64, 512, 512, 0, 0, 0, 0, 1, 1, 1, 256, p) == -22            # a bucket of a_mode 1


@pytest.mark.parametrize("ncu", NCUS)
def test_bwd_params_route_equals_the_rules(ncu):
    seen = set()
    rows_list = sorted({4, 31, 33, 65, 1000, 4092, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 33000} |
                       {m for t in (1, 2, 4, 16, 32) for m in _around(512 * max(1, ncu // t)) if m > 0})
    for rows in rows_list:
        for n_out in (128, 132, 256, 512, 2048):
            for k_in in (128, 132, 512, 1024):
                for kw in (dict(), dict(aligned16=False), dict(ldy=n_out), dict(lddy=n_out + 8, ldy=n_out + 8, ldx=k_in + 8),
                           dict(ldx=1 << 21)):
                    kw["ncu"] = ncu
                    got, want = R.lib_bwd_params_route(rows, n_out, k_in, **kw), R.bwd_params_route(rows, n_out, k_in, **kw)
                    assert got == want, (rows, n_out, k_in, kw, got, want)
                    seen.add(got["kernel"])
    assert seen == {"TN2", "TN_AX"}, (ncu, seen)


def test_workspace_queries_cover_every_route_of_the_shape():
    """mil_gemm_workspace_floats / mil_linear_bwd_params_workspace_floats know neither the leading dimensions nor the flags of
    the call: they must cover the need of every route the shape can take on the current device (ncu = 0)."""
    lib = _lib()
    for N in NS:
        for M in sweep_rows(N, 256):
            for K in KS:
                for a_mode, b_mode in MODES:
                    if a_mode == 1 and M % 4:
                        continue
                    have = lib.mil_gemm_workspace_floats(M, N, K, a_mode)
                    for bucketed in ((False, True) if a_mode == 0 else (False,)):
                        for res, al in VARIANTS:
                            need = R.lib_gemm_route(M, N, K, a_mode=a_mode, b_mode=b_mode, residual=res, bucketed=bucketed, aligned16=al,
                                                    ncu=0)["need"]
                            assert have >= need, (M, N, K, a_mode, b_mode, bucketed, res, al, have, need)
    for rows in (65, 1000, 4095, 4096, 4099, 8192, 33000):
        for n_out in (128, 132, 512, 2048):
            for k_in in (128, 132, 512, 1024):
                have = lib.mil_linear_bwd_params_workspace_floats(rows, n_out, k_in)
                for kw in (dict(), dict(aligned16=False), dict(lddy=n_out + 8, ldx=k_in + 8), dict(ldx=1 << 21)):
                    need = R.lib_bwd_params_route(rows, n_out, k_in, ncu=0, **kw)["need"]
                    assert have >= need, (rows, n_out, k_in, kw, have, need)


def test_the_run_lists_reach_the_kernels_they_name():
    """Every gemm / bwd_params run of the GPU file takes, by the rules at 256 CUs, the kernel it is listed for."""
    for run in R.gemm_runs() + R.bwd_runs():
        r = R.route_of(run)
        assert r["kernel"] == run["kernel"], (R.tag(run), r)
        assert R.lib_route_of(run, 256) == r, (R.tag(run), r)
