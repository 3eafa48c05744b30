"""Test-side helpers of the batched landmark-side chain (mil_tm_pinv_init_bags*, ops.nystrom_core_bags, TransMIL.batch_bags)
that tests/transmil_ref.py and tests/tm_fixed_ref.py do not hold: the shared cases, the float64 core with the pseudo-inverse's
scale given from outside (the planted error "one scale for the whole batch"), and a recorder that also notes a product's batch."""
import contextlib
import functools

import torch

import transmil_ref as R

NAMES = ("mil_tm_pinv_init_bags", "mil_tm_pinv_init_bwd_bags", "mil_tm_pinv_init_bwd_bags_fixed", "mil_tm_pinv_ws_floats_bags")
SINGLE = ("mil_tm_pinv_init", "mil_tm_pinv_init_bwd", "mil_tm_pinv_init_bwd_fixed")
PRODUCTS = ("mil_tm_bgemm", "mil_tm_bgemm_fixed", "mil_tm_bgemm_pieces", "mil_tm_bgemm_pieces_fixed")
SCALE_WORDS, ARG_WORDS = 3 + 2 * R.H, 1 + R.H             # per bag: floats of `scale`, ints of `arg`
BAG = R.H * R.M * R.M                                     # elements of one bag's A2

# the grouped entries alone: three bags whose scales differ by more than 1 % and whose arg-max columns are the first, an
# inner and the last of a bag
STAGE_CASES = (dict(seed=5, col_head=3, col=77), dict(seed=6, col_head=0, col=0), dict(seed=7, col_head=7, col=255))
STAGE_ARGS = (3 * R.M + 77, 0, 7 * R.M + 255)
# the whole core: two bags of different n_pad and a peaked one, which holds the largest maxima of the three
CORE_CASES = ((256, 1.0), (512, 1.0), (256, R.PEAK))


@functools.lru_cache(maxsize=None)
def stage_case(i):
    """(a2, dZ, float64 reference, float32 restatement) of stage case i, computed once and never modified."""
    a2, dZ = R.pinv_case(**STAGE_CASES[i])
    return a2, dZ, R.pinv_run(a2, dZ), R.pinv_run(a2, dZ, torch.float32)


@functools.lru_cache(maxsize=None)
def core_ref(i):
    """(qkv, w, dO, pad, float64 reference, float32 restatement) of core case i, computed once and never modified.  The
    three cases share one res_conv weight (bag 0's): one module weight serves all bags of a step."""
    n_pad, peak = CORE_CASES[i]
    qkv, _, dO, pad = R.core_case(n_pad, peak)
    w = R.core_case(CORE_CASES[0][0], CORE_CASES[0][1])[1]
    return qkv, w, dO, pad, R.core_run(qkv, w, dO), R.core_run(qkv, w, dO, torch.float32)


def a2_of(qkv):
    """The softmaxed landmark map [8, 256, 256] of R.core, in qkv's dtype."""
    n_pad = qkv.shape[0]
    q, k, _ = qkv.chunk(3, dim=-1)
    q, k = (t.reshape(-1, R.H, R.DH).transpose(0, 1) for t in (q, k))
    l = n_pad // R.M
    qL = (q * R.DH ** -0.5).reshape(R.H, R.M, l, R.DH).sum(2) / l
    kL = k.reshape(R.H, R.M, l, R.DH).sum(2) / l
    return (qL @ kL.transpose(-1, -2)).softmax(-1)


def own_maxima(qkv):
    """(largest row abs-sum, largest column abs-sum) over the bag's 8 heads: the two factors of its scale."""
    a = a2_of(qkv).abs()
    return float(a.sum(-1).max()), float(a.sum(-2).max())


def core_scaled(qkv, Wconv, s):
    """R.core with Z0 = a2^T / s for a GIVEN number s instead of the bag's own maxima: what a kernel that took the scale over
    the whole batch would compute for this bag."""
    n_pad = qkv.shape[0]
    q, k, v = qkv.chunk(3, dim=-1)
    q, k, v = (t.reshape(-1, R.H, R.DH).transpose(0, 1) for t in (q, k, v))
    q = q * R.DH ** -0.5
    l = n_pad // R.M
    qL = q.reshape(R.H, R.M, l, R.DH).sum(2) / l
    kL = k.reshape(R.H, R.M, l, R.DH).sum(2) / l
    a1 = (q @ kL.transpose(-1, -2)).softmax(-1)
    a2 = (qL @ kL.transpose(-1, -2)).softmax(-1)
    a3 = (qL @ k.transpose(-1, -2)).softmax(-1)
    z = a2.transpose(-1, -2) / s
    I = torch.eye(R.M, dtype=qkv.dtype)
    for _ in range(R.ITERS):
        xz = a2 @ z
        z = 0.25 * z @ (13 * I - (xz @ (15 * I - (xz @ (7 * I - xz)))))
    out = (a1 @ z) @ (a3 @ v)
    return out.transpose(0, 1).reshape(n_pad, R.H * R.DH) + R.resconv(qkv, Wconv)


def core_scaled_run(qkv, w, dO, s):
    q, wr = (t.detach().double().clone().requires_grad_(True) for t in (qkv, w))
    out = core_scaled(q, wr, s)
    out.backward(dO.double())
    return {"out": out.detach(), "dqkv": q.grad, "dw": wr.grad.reshape(R.H, R.CONV)}


class _Recorder:
    """tm_fixed_ref._Recorder that also notes a product's batch: (name, splits, batch) for the four product entries
    (args[20], args[13]), (name, None, None) otherwise."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            if name in PRODUCTS:
                self._log.append((name, args[20], args[13], tuple(args[14:17])))
            else:
                self._log.append((name, None, None, None))
            return fn(*args)
        return call


@contextlib.contextmanager
def recorded():
    """The list of (entry, splits, batch, (M, N, K)) that code inside the block launches through _lib.checked()."""
    from mil_amd import _lib
    log = []
    orig = _lib.checked
    rec = _Recorder(orig(), log)
    _lib.checked = lambda: rec
    try:
        yield log
    finally:
        _lib.checked = orig
