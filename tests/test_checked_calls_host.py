"""CPU: `_lib.checked()`, the handle whose status-returning entries raise by themselves (ctypes errcheck), beside `_lib.lib()`,
the raw one.  Only entries that return before any HIP call are invoked: no device is touched."""
from ctypes import byref

import pytest

from mil_amd import _lib


def test_errcheck_sits_on_the_status_entries_of_the_checked_handle_only():
    raw, chk = _lib.lib(), _lib.checked()
    assert raw is not chk
    assert _lib.VALUE_RETURNING <= set(_lib.SIGNATURES)
    for name in _lib.SIGNATURES:
        want = None if name in _lib.VALUE_RETURNING else _lib._raise_on_status
        assert getattr(chk, name).errcheck is want, name
        assert getattr(raw, name).errcheck is None, name


def test_a_bad_status_raises_with_the_entry_name_on_checked_and_returns_on_raw():
    route = _lib.GateRoute()
    with pytest.raises(_lib.MilHipError) as e:
        _lib.checked().mil_gate_step_route(0, 512, 2, 1, 0, 0, 0, 0, 256, byref(route))
    assert "mil_gate_step_route" in str(e.value) and "MIL_EINVAL" in str(e.value)
    assert _lib.lib().mil_gate_step_route(0, 512, 2, 1, 0, 0, 0, 0, 256, byref(route)) == -22
    with pytest.raises(_lib.MilHipError, match="mil_gate_pieces"):
        _lib.checked().mil_gate_pieces(None, None, None, 512, None)      # the null check returns before any HIP call


def test_a_good_status_and_a_value_entry_pass_through():
    route = _lib.GateRoute()
    assert _lib.checked().mil_gate_step_route(4096, 512, 2, 1, 0, 0, 0, 0, 256, byref(route)) == 0
    blocks = _lib.checked().mil_layernorm_bwd_blocks(245)
    assert isinstance(blocks, int) and blocks == _lib.lib().mil_layernorm_bwd_blocks(245)
