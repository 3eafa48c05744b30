"""CPU: the route the library plans for the fp32 gate step (mil_gate_step_route, the plan its launches execute) against
tests/step_ref.py::step_route, the independent statement of the rules, over shapes that bracket every threshold.  Pure
host arithmetic on both sides: no device, no memory behind the shapes."""
import ctypes
import itertools

import pytest

from mil_amd import _lib
from step_ref import lib_route, step_route

NCU = (64, 256, 304)
LS = (128, 256, 512, 768, 1024, 2048, 4096, 4224)
CS = (2, 3, 5)
FLAGS = list(itertools.product((False, True), repeat=3))          # aligned32, bucketed, pieces
KEEP = ((False, False), (True, False), (False, True))             # (train, given_bits): eval, train, eval-like with given keep bits


def rows_around_thresholds(ncu: int, L: int) -> list:
    """Row counts on both sides of every threshold of the plan for ncu compute units and width L."""
    rows = set()
    for k in range(3 * ncu // 4 - 2, 3 * ncu // 4 + 3):            # r32 <-> 128-row tiles: fewer tiles than 3/4 of the CUs
        rows.update((128 * k - 1, 128 * k, 128 * k + 1))
    for tiles in (32 * ncu, 64 * ncu):                              # RT of the r32 launch: ncu and 2 ncu tiles of 32 rows
        rows.update((tiles - 1, tiles, tiles + 1))
    for m in (1, 2, 4):                                             # whole rounds of the grid + a tail
        rows.update(128 * ncu * m + t for t in (0, 1, 40, 64, 65, 1000, 1024, 1025))
    smax = ncu // (3 * (L // 128))                                  # KG = 2 once a row chunk is 512 rows deep
    if smax >= 1:
        rows.update((512 * smax - 1, 512 * smax, 512 * smax + 1))
    at = -(-(1 << 29) // L)                                         # k_gate_bwd_dw2's 32-bit offsets: R L < 2^29
    rows.update((at - 1, at))
    return sorted(rows)


@pytest.mark.parametrize("ncu", NCU)
def test_library_route_equals_the_mirror(ncu, monkeypatch):
    monkeypatch.delenv("MIL_FUSE_POOL", raising=False)
    bad, n, want_n = [], 0, 0
    for L in LS:
        rows = rows_around_thresholds(ncu, L)
        assert len(rows) >= 40 and rows[0] > 0
        want_n += len(rows) * len(CS) * len(KEEP) * len(FLAGS)
        for R, C, (train, given), (aligned32, bucketed, pieces) in itertools.product(rows, CS, KEEP, FLAGS):
            kw = dict(aligned32=aligned32, bucketed=bucketed, pieces=pieces, ncu=ncu, given_bits=given)
            want = step_route(R, L, C, train, **kw)
            have = lib_route(R, L, C, train, **kw)
            n += 1
            diff = {k: (have[k], v) for k, v in want.items() if have[k] != v}
            if diff:
                bad.append(f"R={R} L={L} C={C} train={train} {kw}: (library, mirror) {diff}")
    assert n == want_n and n > 15000, (n, want_n)
    assert not bad, f"{len(bad)} of {n} shapes differ:\n" + "\n".join(bad[:50])


def test_sweep_reaches_every_value_of_every_field():
    """The shapes above are not all on one side of a rule: each value a field can take turns up."""
    seen = {}
    for ncu, L in itertools.product(NCU, LS):
        for R, (train, given), flags in itertools.product(rows_around_thresholds(ncu, L), KEEP, FLAGS):
            r = step_route(R, L, 2, train, aligned32=flags[0], bucketed=flags[1], pieces=flags[2], ncu=ncu, given_bits=given)
            for k in ("main", "rt", "tail", "tail_kernel", "tail_rt", "bits", "pool", "dw"):
                seen.setdefault(k, set()).add(r[k])
            seen.setdefault("tail_rows", set()).add(min(r["tail_rows"], 65))
    assert seen == dict(main={"r32", "fwd2", "fwd2_pw", "legacy"}, rt={None, 1, 2, 3}, tail={None, "small", "big"},
                        tail_kernel={None, "linear_small", "r32"}, tail_rt={None, 1}, bits={None, "given", "in_kernel", "generator"},
                        pool={"fused", "alone"}, dw={"dw<1>", "dw<2>", "dw2"}, tail_rows={0, 1, 40, 64, 65})


def test_route_query_agrees_with_the_workspace_size_and_rejects_bad_shapes():
    lib = _lib.lib()
    p = _lib.GateRoute()
    for R, L in ((7600, 512), (32768, 512), (33792, 1024), (1, 128)):
        assert lib.mil_gate_step_route(R, L, 2, 1, 0, 0, 0, 0, 0, ctypes.byref(p)) == 0
        assert lib.mil_gate_bwd_workspace_floats(R, L) == p.S * 384 * L + p.S * (L // 128) * 4 * 192
        assert (p.S - 1) * p.kc < R <= p.S * p.kc and p.kc % 32 == 0
    assert lib.mil_gate_step_route(4096, 96, 2, 1, 0, 0, 0, 0, 256, ctypes.byref(p)) == 0 and p.dw == -1    # no dW kernel for L % 128 != 0
    assert lib_route(4096, 96, 2, False, ncu=256)["dw"] is None
    for R, L, C in ((0, 512, 2), (4096, 0, 2), (4096, 520, 2), (4096, 512, 0)):
        assert lib.mil_gate_step_route(R, L, C, 1, 0, 0, 0, 0, 256, ctypes.byref(p)) == -22        # MIL_EINVAL
    assert lib.mil_gate_step_route(4096, 512, 2, 1, 0, 0, 0, 0, 256, None) == -22
