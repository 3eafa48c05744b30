"""CPU: when the fp32 step takes its deferred-pool route (no pool pass over x: hrow from the gate forward's K loop, M from the
weight gradient and the fold).  Every condition of the plan (gate_route_plan, csrc/gate_fwd.hip) is violated on its own, and the
library's report for the step descriptor (mil_image_only_step_route: host arithmetic, no pointer is followed) must refuse the
route each time; with all of them met it must grant it.  Also the trainer's count of the bags (slots) a row chunk touches."""
import ctypes

import pytest

from mil_amd import _lib
from mil_amd.trainer import ImageOnlyTrainer

NCU = 256
FAKE = 0x1000            # a non-null "device pointer": the report reads no memory
ALL = _lib.STAGE_ALL | _lib.STAGE_POOL_FUSED | _lib.STAGE_POOL_DEFERRED
ENV = ("MIL_POOL_DEFERRED", "MIL_DW_PIECES", "MIL_TAIL_H", "MIL_FUSE_POOL")


def _step(R=32768, L=512, B=32, C=2, train=1):
    a = _lib.ImageOnlyStep()
    a.struct_bytes = ctypes.sizeof(_lib.ImageOnlyStep)
    a.R, a.L, a.B, a.C, a.T = R, L, B, C, R // 32
    a.train = train
    for f in ("x", "y", "tile_map", "bag_tile_off", "Wv", "bv", "Wu", "bu", "w", "b", "Wf", "bf", "scores", "gates", "partials",
              "hrow", "ds", "dw_ws", "M", "Mdrop", "xbits", "mbits", "Wp", "mpart"):
        setattr(a, f, FAKE)
    a.mpart_floats = _lib.lib().mil_pool_deferred_workspace_floats(R, L)
    a.dw_chunk_bags = 2
    return a


def _route(a, stages=ALL):
    r = _lib.GateRoute()
    assert _lib.lib().mil_image_only_step_route(ctypes.byref(a), stages, NCU, ctypes.byref(r)) == 0
    return r


DEFAULT_ON = True        # MIL_POOL_DEFERRED unset: the route is on where it applies


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MIL_POOL_DEFERRED", "1")


@pytest.mark.parametrize("train", [0, 1])
def test_the_route_is_granted_when_every_condition_holds(train):
    r = _route(_step(train=train))
    assert r.pool_deferred == 1 and r.pool_fused == 0
    assert r.main == 2 and r.tail == 0 and r.dw == 2                       # FWD2_PW, no tail rows, DW2
    assert _lib.lib().mil_pool_deferred_workspace_floats(32768, 512) == r.S * _lib.POOL_DEFERRED_SLOTS * 16 * 512
    for bags in (1, _lib.POOL_DEFERRED_SLOTS):
        a = _step(train=train)
        a.dw_chunk_bags = bags
        assert _route(a).pool_deferred == 1


def test_without_the_hint_the_plan_is_todays():
    a = _step()
    r = _route(a, _lib.STAGE_ALL | _lib.STAGE_POOL_FUSED)
    assert r.pool_deferred == 0 and r.pool_fused == 1
    old = _lib.GateRoute()
    assert _lib.lib().mil_gate_step_route(a.R, a.L, a.C, 1, 2, 1, 1, 0, NCU, ctypes.byref(old)) == 0
    for f, _ in _lib.GateRoute._fields_:
        assert getattr(r, f) == getattr(old, f), f
    # the hint with a stage subset: the same answer for every call of the step
    for stages in (_lib.STAGE_TAIL, _lib.STAGE_GATE_BWD, _lib.STAGE_REDUCE | _lib.STAGE_ADAM,
                   _lib.STAGE_GATE_FWD | _lib.STAGE_DROPBITS):
        assert _route(a, stages | _lib.STAGE_POOL_DEFERRED).pool_deferred == 1
        assert _route(a, stages).pool_deferred == 0


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


VIOLATIONS = {
    "bf16 x": _set(x_bf16=1),
    "no weight pieces: the forward is not on the split-bf16 loop": _set(Wp=None),
    "C != 2": _set(C=3),
    "no labels": _set(y=None),
    "no hrow": _set(hrow=None),
    "lengths on the device": _set(bag_len_dev=FAKE),
    "bucketed rows": _set(rows_dev=FAKE),
    "chunk bags unknown": _set(dw_chunk_bags=0),
    "a chunk touches more than MP_SLOTS bags": _set(dw_chunk_bags=_lib.POOL_DEFERRED_SLOTS + 1),
    "no workspace": _set(mpart=None),
    "workspace too small": _set(mpart_floats=_lib.POOL_DEFERRED_SLOTS * 16 * 512),
    "a partial tile: T * 32 != R": _set(T=1025),
    "a few long bags: the tail is k_tail_stats / k_tail_apply": _set(B=8),
}


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_one_violated_condition_refuses_the_route(what):
    a = _step()
    VIOLATIONS[what](a)
    assert _route(a).pool_deferred == 0, what


@pytest.mark.parametrize("R,L,B,why", [
    (11264, 512, 11, "fewer 128-row tiles than 3/4 of the CUs: the forward is k_gate_fwd_r32"),
    (32768 + 64, 512, 32, "rows beyond whole rounds leave k_gate_fwd2"),
    (1 << 20, 512, 1024, "R L >= 2^29: the weight gradient is not on the dw2 plan"),
    (32768, 1024, 32, "L != 512: no head rows in the forward's LDS"),
    (32768, 256, 32, "L != 512"),
])
def test_shapes_off_the_route(R, L, B, why):
    a = _step(R=R, L=L, B=B)
    a.T = (R + 31) // 32
    assert _route(a).pool_deferred == 0, why


@pytest.mark.parametrize("var,val", [("MIL_POOL_DEFERRED", "0"), ("MIL_DW_PIECES", "0"), ("MIL_TAIL_H", "0")])
def test_switches_are_read_per_call(monkeypatch, var, val):
    a = _step()
    assert _route(a).pool_deferred == 1
    monkeypatch.setenv(var, val)
    assert _route(a).pool_deferred == 0
    monkeypatch.setenv(var, "1")
    assert _route(a).pool_deferred == 1


def test_the_default_without_the_variable(monkeypatch):
    monkeypatch.delenv("MIL_POOL_DEFERRED")
    assert _route(_step()).pool_deferred == int(DEFAULT_ON)


def test_bad_descriptors_are_rejected():
    r = _lib.GateRoute()
    a = _step()
    assert _lib.lib().mil_image_only_step_route(None, ALL, NCU, ctypes.byref(r)) == -22
    assert _lib.lib().mil_image_only_step_route(ctypes.byref(a), ALL, NCU, None) == -22
    a.struct_bytes -= 8
    assert _lib.lib().mil_image_only_step_route(ctypes.byref(a), ALL, NCU, ctypes.byref(r)) == -22


class _Lay:
    def __init__(self, lengths):
        self.lengths = list(lengths)


@pytest.mark.parametrize("lengths,want", [
    ([1024] * 32, 3),                                                       # 1568-row chunks: [1568, 3136) touches three bags
    ([1024] * 24, 3),                                                       # 1184-row chunks: [7104, 8288) touches three bags
    ([160, 192, 160, 4096, 2048, 1024, 3072, 512, 4096, 4096, 2048, 3072], 4),
    ([96] * 5 + [4096] * 5 + [3616], 6),
    ([0, 1024, 0] + [1024] * 23, 3),                                        # an empty bag between two others takes a slot
    ([1024, 0, 0, 0] + [1024] * 23, 5),
])
def test_the_trainer_counts_the_bags_of_a_row_chunk(lengths, want):
    R = sum(lengths)
    r = _lib.GateRoute()
    assert _lib.lib().mil_gate_step_route(R, 512, 2, 1, 0, 0, 0, 0, NCU, ctypes.byref(r)) == 0
    # the reference count: every row's bag, chunk by chunk; a slot is the bag index relative to the chunk's first bag
    bag_of = [b for b, n in enumerate(lengths) for _ in range(n)]
    brute = max(max(bag_of[c0:c0 + r.kc]) - min(bag_of[c0:c0 + r.kc]) + 1 for c0 in range(0, R, r.kc))
    assert brute == want
    assert ImageOnlyTrainer._chunk_bags(_Lay(lengths), R, 512, 2) == want
