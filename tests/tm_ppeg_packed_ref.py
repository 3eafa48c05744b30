"""Test-side helpers of the packed PPEG (mil_tm_ppeg_*_packed, ops.tm_ppeg_packed, TransMIL.packed_ppeg) that tests/transmil_ref.py
does not hold: the entries' names, the table restated, the shared stage case, the float64 / float32 references of the sums that
cross bags, and a restatement of the packed kernel in which the three mistakes it can make silently can be planted."""
import functools
import math

import torch

import transmil_ref as R

NAMES = ("mil_tm_ppeg_fwd_packed", "mil_tm_ppeg_bwd_packed", "mil_tm_ppeg_packed_ws_floats", "mil_tm_ppeg_bwd_packed_fixed")
SIZES = ("mil_tm_ppeg_packed_ws_floats",)
STATUS = tuple(n for n in NAMES if n not in SIZES)
SINGLE = ("mil_tm_ppeg_fwd", "mil_tm_ppeg_bwd", "mil_tm_ppeg_bwd_fixed")           # what a packed PPEG step must not launch

# a grid narrower than the 7 x 7 window first, a one-cell bag between larger ones, exactly one chunk of 8 grid rows (8), a chunk and
# a tail (9), two chunks and a tail (17) last; and one bag alone.  Rows 10, 82, 2, 65, 290.
SIDES = ((3, 9, 1, 8, 17), (9,))
CUT = {"proj": slice(0, 7), "proj1": slice(1, 6), "proj2": slice(2, 5)}             # dW7 is the whole 7 x 7 map, dW5 / dW3 its centre


def row_off(sides):
    off = [0]
    for s in sides:
        off.append(off[-1] + 1 + s * s)
    return off


def bag_rows(sides, b):
    off = row_off(sides)
    return slice(off[b], off[b + 1])


def chunks(sides):
    return sum((s + 7) // 8 for s in sides)


def dims(sides):
    """(gmax, cmax, zmax): what the launches and the table's length take from (nb, R) alone."""
    nb, rows = len(sides), row_off(sides)[-1]
    gmax = math.isqrt(nb * (rows - nb))
    return gmax, min(gmax, (gmax + 7 * nb) // 8), (math.isqrt(rows - 2 * nb + 1) + 7) // 8


def table(sides):
    """row_off [nb + 1] | side [nb] | grow_off [nb + 1] | chunk_off [nb + 1] | bag_of_gridrow [gmax] | bag_of_chunk [cmax], -1 behind
    the bags' grid rows and chunks - restated, not imported from the code under test."""
    gmax, cmax, _ = dims(sides)
    grow, chunk, bag_g, bag_c = [0], [0], [], []
    for b, s in enumerate(sides):
        grow.append(grow[-1] + s)
        chunk.append(chunk[-1] + (s + 7) // 8)
        bag_g += [b] * s
        bag_c += [b] * ((s + 7) // 8)
    assert len(bag_g) <= gmax and len(bag_c) <= cmax, (sides, gmax, cmax)
    return (row_off(sides) + list(sides) + grow + chunk + bag_g + [-1] * (gmax - len(bag_g)) + bag_c + [-1] * (cmax - len(bag_c)))


@functools.lru_cache(maxsize=None)
def stage_case(sides):
    """(p, x, dy): ONE weight set for all bags (R.ppeg_case of the first side) and random packed rows [R, 512] in ALL rows, the
    cls rows included - float64 holding float32 values, so that the GPU reads exactly what the references read."""
    p = {k: v.float().double() for k, v in R.ppeg_case(sides[0])[0].items()}
    rows = row_off(sides)[-1]
    g = torch.Generator().manual_seed(5000 + 31 * rows + len(sides))
    x = torch.randn((rows, 512), generator=g, dtype=torch.float32).double()
    dy = torch.randn((rows, 512), generator=g, dtype=torch.float32).double()
    return p, x, dy


@functools.lru_cache(maxsize=None)
def per_bag(sides, dtype=torch.float64):
    """R.ppeg_run of every bag on its own slice (computed once, left unchanged)."""
    p, x, dy = stage_case(sides)
    return tuple(R.ppeg_run(p, x[bag_rows(sides, b)], dy[bag_rows(sides, b)], s, dtype) for b, s in enumerate(sides))


def grad_sums(sides, dtype=torch.float64):
    """{dproj.weight, dproj.bias, ..}: the sums over the bags of R.ppeg_run's parameter gradients, bag 0 first."""
    runs = per_bag(sides, dtype)
    out = {"d" + n: runs[0]["d" + n].clone() for n in R.PPEG_NAMES}
    for r in runs[1:]:
        for k in out:
            out[k] = out[k] + r[k]
    return out


def grad_blocks():
    return {"d" + n: R.whole() for n in R.PPEG_NAMES}


def got_grads(dWf, db):
    """What the kernels' dWf [512, 1, 7, 7] and db [512] mean for the six parameters."""
    out = {}
    for name, sl in CUT.items():
        out[f"d{name}.weight"] = dWf[:, :, sl, sl]
        out[f"d{name}.bias"] = db
    return out


# ---- the packed kernel restated tap by tap, with the three mistakes it can make silently
def folded(p, dtype):
    W7, W5, W3 = (p["pos_layer." + n + ".weight"].to(dtype) for n in ("proj", "proj1", "proj2"))
    Wf = W7 + torch.nn.functional.pad(W5, (1, 1, 1, 1)) + torch.nn.functional.pad(W3, (2, 2, 2, 2))
    Wf = Wf.reshape(512, 7, 7).clone()
    Wf[:, 3, 3] += 1
    bias = sum(p["pos_layer." + n + ".bias"].to(dtype) for n in ("proj", "proj1", "proj2"))
    return Wf, bias


def packed_ref(sides, dtype=torch.float64, flip=False, plant=None):
    """y [R, 512] (flip: dx from dy, the transposed map without bias) of the packed PPEG as k_tm_ppeg_packed states it: per bag
    the grid at row_off[b] + 1, side s_b, a tap skipped where it leaves the bag's own s_b x s_b grid, the cls row passed through.
    plant: "side" - bag b addressed with the side of the next bag (the last: of the one before); "window" - a tap skipped only
    where its ROW leaves the packed rows [0, R), not where it leaves the bag's grid; "cls" - the grid at row_off[b], the + 1 of
    the cls row lost.  Rows a mistaken kernel would not write stay 0; a row it would read behind R wraps to the front."""
    p, x, dy = stage_case(sides)
    src = (dy if flip else x).to(dtype)
    Wf, bias = folded(p, dtype)
    if flip:
        bias = torch.zeros_like(bias)
    off, rows = row_off(sides), row_off(sides)[-1]
    out = torch.zeros_like(src)
    sgn = -1 if flip else 1
    for b, own in enumerate(sides):
        s = own
        if plant == "side":
            s = sides[b + 1] if b + 1 < len(sides) else sides[b - 1]
        base = off[b] + (0 if plant == "cls" else 1)
        out[off[b]] = src[off[b]]                                        # the cls row
        i, j = torch.meshgrid(torch.arange(s), torch.arange(s), indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
        acc = bias.expand(s * s, 512).clone()
        for a in range(7):
            for c in range(7):
                ii, jj = i + sgn * (a - 3), j + sgn * (c - 3)
                r = base + ii * s + jj
                ok = (r >= 0) & (r < rows) if plant == "window" else (ii >= 0) & (ii < s) & (jj >= 0) & (jj < s)
                acc = acc + ok.to(dtype)[:, None] * Wf[:, a, c][None, :] * src[r % rows]
        cells = (base + torch.arange(s * s)) % rows
        out[cells] = acc
    return out
