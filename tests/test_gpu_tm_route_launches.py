"""GPU: what one TransMIL forward + backward launches, route by route (ops.tm_route).  The value tests hold the routes to each
other's numbers; a launch that moved, or ran twice with the same result, passes them all.  Here the ordered list of entry names
that go through _lib.checked() is compared with tests/golden/tm_route_launches.json, recorded by record() below on the commit in
front of the one that merged the three step bodies - the project's own output, a list of names per route."""
import json
import os

import pytest
import torch

from tm_bags_ref import recorded

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tm_route_launches.json")
LENGTHS = [3, 17, 260]          # sides 2, 5, 17; n_pad 256, 256, 512: two single-block bags and a two-block one
SWITCHES = ("fused_cls", "deterministic", "gemm_pieces", "batch_bags", "packed", "packed_ppeg", "packed_cls")
ENV = ("MIL_TM_FUSED_A1", "MIL_TM_FUSED_A3", "MIL_TM_FUSED_CLS", "MIL_TM_DETERMINISTIC", "MIL_TM_PIECES", "MIL_TM_BATCH_BAGS",
       "MIL_TM_PACKED", "MIL_TM_PACKED_PPEG", "MIL_TM_PACKED_CLS")
# route -> the module's switches, the environment of the fused passes, need_attn, train / eval
ROUTES = {
    "each": dict(),
    "each_fused_a1_a3": dict(env=dict(MIL_TM_FUSED_A1="1", MIL_TM_FUSED_A3="1")),
    "batched": dict(batch_bags=True),
    "batched_deterministic": dict(batch_bags=True, deterministic=True),
    "packed": dict(packed=True),
    "packed_ppeg": dict(packed=True, packed_ppeg=True),
    "packed_ppeg_deterministic_pieces3": dict(packed=True, packed_ppeg=True, deterministic=True, gemm_pieces=3),
    "packed_ppeg_cls_eval": dict(packed=True, packed_ppeg=True, packed_cls=True, need_attn="cls", train=False),
    "each_fused_cls_eval": dict(fused_cls=True, need_attn="cls", train=False),
}


def _model():
    """One model for all routes, in train mode, with the keep bits of a bag-by-bag pass forced: no route draws any."""
    from mil_amd import synthetic as syn
    from mil_amd.model.dim1 import TransMIL
    net = TransMIL(n_classes=2, L=768)
    net.load_state_dict(syn.transmil_params(13, 768, 2))
    net = net.to(DEV).train()
    net._drop_seed = 1234
    x = torch.randn((sum(LENGTHS), 768), generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        net(x, LENGTHS)
    net.force_bits = [tuple(b.clone() for b in pair) for pair in net.last_bits]
    return net, x


def _launches(net, x, spec):
    """The entry names of one forward + backward under the switches of `spec`, in launch order."""
    saved = {k: os.environ.pop(k, None) for k in ENV}
    try:
        os.environ.update(spec.get("env", {}))
        for name in SWITCHES:
            setattr(net, name, spec.get(name))
        net.train(spec.get("train", True))
        net.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_(True)
        with recorded() as log:
            h, _ = net(xd, LENGTHS, need_attn=spec.get("need_attn", False))
            h.sum().backward()
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return [entry[0] for entry in log]


def record(path=FIXTURE):
    """Writes the fixture.  Run by hand (`python tests/test_gpu_tm_route_launches.py`), once, on the commit whose launches are
    to be kept."""
    net, x = _model()
    with open(path, "w") as f:
        json.dump({route: _launches(net, x, spec) for route, spec in ROUTES.items()}, f, indent=0)
        f.write("\n")


@pytest.fixture(scope="module")
def model():
    return _model()


def test_the_fixture_names_every_route():
    with open(FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(ROUTES)
    assert all(len(names) > 50 for names in want.values())
    assert len({tuple(names) for names in want.values()}) == len(ROUTES)        # no two routes launch the same list


@pytest.mark.parametrize("route", list(ROUTES))
def test_launches_are_the_recorded_ones(model, route):
    with open(FIXTURE) as f:
        want = json.load(f)[route]
    got = _launches(*model, ROUTES[route])
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (route, len(got), len(want), first, got[first:first + 4], want[first:first + 4])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mil_amd  # noqa: F401
    record(*sys.argv[1:2])
