"""Test-side helpers of the fixed-order TransMIL sums (mil_tm_*_fixed, ops deterministic=True) that tests/transmil_ref.py does
not hold: operand layouts for the strided product, the row-gather backward as an ascending float32 sum, the workspace formulas
and a recorder of the C-ABI entries a piece of code launches."""
import contextlib

import torch

SENT = -12345.678                    # the sentinel; the bit pattern is what is compared
FIXED = ("mil_tm_bgemm_fixed", "mil_tm_row_gather_bwd_fixed", "mil_tm_pinv_init_bwd_fixed", "mil_tm_resconv_bwd_fixed",
         "mil_tm_ppeg_bwd_fixed")
WS = ("mil_tm_bgemm_ws_floats", "mil_tm_row_gather_ws_floats", "mil_tm_pinv_ws_floats", "mil_tm_resconv_ws_floats",
      "mil_tm_ppeg_ws_floats")
ATOMIC = ("mil_tm_row_gather_bwd", "mil_tm_pinv_init_bwd", "mil_tm_resconv_bwd", "mil_tm_ppeg_bwd")


def layout(kind, b, r, c):
    """(numel, offset, (stride batch, stride row, stride col)) of a [b, r, c] operand; every index stays below numel."""
    if kind == "plain":
        lay = (b * r * c, 0, (r * c, c, 1))
    elif kind == "T":                       # each batch stored column-major
        lay = (b * r * c, 0, (r * c, 1, r))
    elif kind == "padded":                  # rows 5 floats apart, 3 floats in front: gaps the entry must leave alone
        lay = (3 + b * r * (c + 5), 3, (r * (c + 5), c + 5, 1))
    elif kind == "merged_out":              # head b's 64 columns of [r, 512] merged-head rows: b <= 8, c <= 64
        assert b <= 8 and c <= 64, (b, c)
        lay = (r * 512, 0, (64, 512, 1))
    else:
        raise KeyError(kind)
    numel, off, st = lay
    assert off + (b - 1) * st[0] + (r - 1) * st[1] + (c - 1) * st[2] < numel, (kind, b, r, c)
    return lay


def place(T, kind, fill=0.0):
    """float32 CPU buffer holding T [b, r, c] in the layout, `fill` elsewhere; a mask of the elements it owns; offset, strides."""
    b, r, c = T.shape
    numel, off, st = layout(kind, b, r, c)
    buf = torch.full((numel,), fill, dtype=torch.float32)
    torch.as_strided(buf, (b, r, c), st, off).copy_(T)
    mask = torch.zeros(numel, dtype=torch.bool)
    torch.as_strided(mask, (b, r, c), st, off).fill_(True)
    return buf, mask, off, st


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def gather_bwd_ordered(dd, idx, src_rows):
    """(dsrc [src_rows, E], dextra [E]) in float32 on the CPU: row r of dd added onto its target for r = 0, 1, 2 .. in that
    order, every sum starting from zero - the order mil_tm_row_gather_bwd_fixed states."""
    dsrc = torch.zeros((src_rows, dd.shape[1]), dtype=torch.float32)
    dex = torch.zeros(dd.shape[1], dtype=torch.float32)
    for r, i in enumerate(idx):
        if i >= 0:
            dsrc[i] = dsrc[i] + dd[r]
        elif i == -2:
            dex = dex + dd[r]
    return dsrc, dex


def ws_floats(name, *a):
    """The workspace formulas of include/mil_hip.h, restated."""
    if name == "mil_tm_bgemm_ws_floats":
        batch, M, N, splits = a
        return splits * batch * M * N if splits > 1 and min(batch, M, N) > 0 else 0
    if name == "mil_tm_row_gather_ws_floats":
        return 3 * a[0] if a[0] > 0 else 0
    if name == "mil_tm_pinv_ws_floats":
        return 256
    if name == "mil_tm_resconv_ws_floats":
        return -(-a[0] // 256) * 8 * 33 if a[0] > 0 else 0
    if name == "mil_tm_ppeg_ws_floats":
        return -(-a[0] // 8) * 50 * 512 if a[0] > 0 else 0
    raise KeyError(name)


def max_naming(idx, src_rows):
    """The largest number of entries of idx that name one source row."""
    t = torch.as_tensor(idx, dtype=torch.int64)
    t = t[t >= 0]
    return int(torch.bincount(t, minlength=src_rows).max()) if t.numel() else 0


class _Recorder:
    """Stands in for the handle _lib.checked() returns: every entry looked up on it is noted, as (name, splits) for the two
    products and (name, None) otherwise, then the real function runs."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            splits = args[20] if name in ("mil_tm_bgemm", "mil_tm_bgemm_fixed") else None
            self._log.append((name, splits))
            return fn(*args)
        return call


@contextlib.contextmanager
def recorded():
    """The list of (entry, splits) that code inside the block launches through _lib.checked()."""
    from mil_amd import _lib
    log = []
    orig = _lib.checked
    rec = _Recorder(orig(), log)
    _lib.checked = lambda: rec
    try:
        yield log
    finally:
        _lib.checked = orig
