"""CPU, no library launch: the route of a TransMIL step is resolved in one place (ops.tm_route) and both graph steppers key their
graphs by it.  The table of tm_route against a restatement of its rules; every key the steppers gave before the route existed,
unchanged; the fused switches, which no key used to name, now part of it exactly where they change the launches; and
train_ddp.build_model setting every flag on every TransMIL module."""
import argparse
import dataclasses
import itertools
from types import SimpleNamespace

import pytest

SWITCHES = ("deterministic", "gemm_pieces", "batch_bags", "packed", "packed_ppeg", "packed_cls", "fused_cls")
ENV = {"deterministic": "MIL_TM_DETERMINISTIC", "gemm_pieces": "MIL_TM_PIECES", "batch_bags": "MIL_TM_BATCH_BAGS",
       "packed": "MIL_TM_PACKED", "packed_ppeg": "MIL_TM_PACKED_PPEG", "packed_cls": "MIL_TM_PACKED_CLS",
       "fused_cls": "MIL_TM_FUSED_CLS"}
FUSED_ENV = ("MIL_TM_FUSED_A1", "MIL_TM_FUSED_A3")
VALUES = {name: (None, 0, 3) if name == "gemm_pieces" else (None, False, True) for name in SWITCHES}


def _clear(monkeypatch):
    for name in (*ENV.values(), *FUSED_ENV):
        monkeypatch.delenv(name, raising=False)


def _all_switches(names=SWITCHES, **fixed):
    for combo in itertools.product(*(VALUES[n] for n in names)):
        yield SimpleNamespace(**{**dict.fromkeys(SWITCHES), **dict(zip(names, combo)), **fixed})


def _rules(sw, a1, a3, env_cls, n_bags, need):
    """The rules, restated.  a1, a3, env_cls: the environment variables of the three fused switches; fused_cls is the attribute,
    else its variable; the other six switches' variables are unset, so None is off."""
    cls_asked = need is not True and need == "cls"
    fused_cls = sw.fused_cls if sw.fused_cls is not None else env_cls
    packed = n_bags > 1 and bool(sw.packed) and (need is False or (cls_asked and bool(sw.packed_cls)))
    batched = not packed and n_bags > 1 and need is False and bool(sw.batch_bags)
    if packed:
        fused_a1 = fused_a3 = True
        cls = "packed" if cls_asked else None
    elif cls_asked and fused_cls:
        fused_a1 = fused_a3 = True
        cls = "fused"
    else:
        fused_a1, fused_a3 = a1 and need is False, a3 and need is False
        cls = "maps" if cls_asked else None
    return dict(bags="packed" if packed else "batched" if batched else "each", ppeg_packed=packed and bool(sw.packed_ppeg),
                fused_a1=fused_a1, fused_a3=fused_a3, cls=cls, det=bool(sw.deterministic), pieces=sw.gemm_pieces or 0)


def test_truth_table(monkeypatch):
    from mil_amd import ops
    _clear(monkeypatch)
    count = 0
    for a1, a3, env_cls in itertools.product((False, True), repeat=3):
        monkeypatch.setenv("MIL_TM_FUSED_A1", "1" if a1 else "0")
        monkeypatch.setenv("MIL_TM_FUSED_A3", "1" if a3 else "0")
        monkeypatch.setenv("MIL_TM_FUSED_CLS", "1" if env_cls else "0")
        for sw in _all_switches():
            for n_bags, need in itertools.product((1, 2), (False, True, "cls")):
                got = ops.tm_route(sw, n_bags, need)
                assert dataclasses.asdict(got) == _rules(sw, a1, a3, env_cls, n_bags, need), (vars(sw), a1, a3, env_cls, n_bags, need)
                count += 1
    assert count == 8 * 3 ** 7 * 6
    route = ops.tm_route(sw, 2, False)
    assert [f.name for f in dataclasses.fields(route)] == ["bags", "ppeg_packed", "fused_a1", "fused_a3", "cls", "det", "pieces"]
    with pytest.raises(dataclasses.FrozenInstanceError):
        route.bags = "each"
    sw.gemm_pieces = 2
    with pytest.raises(ValueError):
        ops.tm_route(sw, 2, False)


def test_an_attribute_left_none_reads_its_environment_variable(monkeypatch):
    from mil_amd import ops
    _clear(monkeypatch)
    sw = SimpleNamespace(**dict.fromkeys(SWITCHES))
    assert ops.tm_route(sw, 2, "cls") == ops.TmRoute("each", False, False, False, "maps", False, 0)
    monkeypatch.setenv("MIL_TM_FUSED_CLS", "1")
    assert ops.tm_route(sw, 2, "cls") == ops.TmRoute("each", False, True, True, "fused", False, 0)
    for name in ("MIL_TM_PACKED", "MIL_TM_PACKED_PPEG", "MIL_TM_DETERMINISTIC", "MIL_TM_BATCH_BAGS"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setenv("MIL_TM_PIECES", "3")
    assert ops.tm_route(sw, 2, "cls") == ops.TmRoute("each", False, True, True, "fused", True, 3)
    assert ops.tm_route(sw, 2, False) == ops.TmRoute("packed", True, True, True, None, True, 3)
    assert ops.tm_route(sw, 1, False) == ops.TmRoute("each", False, False, False, None, True, 3)
    monkeypatch.setenv("MIL_TM_PACKED_CLS", "1")
    assert ops.tm_route(sw, 2, "cls") == ops.TmRoute("packed", True, True, True, "packed", True, 3)
    sw.packed = False                                                   # the attribute wins over the environment
    assert ops.tm_route(sw, 2, False) == ops.TmRoute("batched", False, False, False, None, True, 3)


# ---- the keys as the steppers built them before ops.tm_route, their expressions copied as they stood
def _image_key_before(self, sides):
    from mil_amd import ops
    m = self.model
    attn = bool(getattr(m, "patch_attn", False))
    det = ops.tm_deterministic(m.extractor_pathology.deterministic)
    pieces = ops.tm_pieces(m.extractor_pathology.gemm_pieces)
    batched = ops.tm_batch_bags(m.extractor_pathology.batch_bags) and len(sides) > 1 and not attn
    cls = attn and ops.tm_packed_cls(getattr(m.extractor_pathology, "packed_cls", None))
    packed = ops.tm_packed(m.extractor_pathology.packed) and len(sides) > 1 and (not attn or cls)
    ppeg = packed and ops.tm_packed_ppeg(getattr(m.extractor_pathology, "packed_ppeg", None))
    route = (("packed",) + (("ppeg",) if ppeg else ()) + (("cls",) if cls else ())) if packed else ("batch_bags",) if batched else ()
    return (("transmil-sides", tuple(sides), bool(m.training), self.backward) + (("patch_attn",) if attn else ())
            + (("deterministic",) if det else ()) + ((("gemm_pieces", pieces),) if pieces else ())
            + route)


def _fusion_key_before(self, cap, lengths):
    from mil_amd import ops
    agg = self.model.aggregator
    det, pieces = ops.tm_deterministic(agg.deterministic), ops.tm_pieces(agg.gemm_pieces)
    batched = ops.tm_batch_bags(agg.batch_bags) and len(lengths) > 1      # the aggregator's batched landmark-side chain
    packed = ops.tm_packed(agg.packed) and len(lengths) > 1               # its packed sequence, which wins over that
    ppeg = packed and ops.tm_packed_ppeg(getattr(agg, "packed_ppeg", None))  # ... with PPEG as one launch set too
    cls = packed and ops.tm_packed_cls(getattr(agg, "packed_cls", None))     # ... and the cls attention on that route
    route = (("packed",) + (("ppeg",) if ppeg else ()) + (("cls",) if cls else ())) if packed else ("batch_bags",) if batched else ()
    return (("fusion-transmil", int(cap), self.sides(lengths), bool(self.model.training), bool(agg.training), self.backward)
            + (("deterministic",) if det else ()) + ((("gemm_pieces", pieces),) if pieces else ())
            + route)


def _steppers(ex, patch_attn, training=False):
    """The SimpleNamespace stand-ins of tests/test_tm_cls_packed_host.py: what the two key methods read of a stepper."""
    ex.training = training
    model = SimpleNamespace(extractor_pathology=ex, aggregator=ex, training=training, patch_attn=patch_attn)
    return (SimpleNamespace(model=model, backward=training),
            SimpleNamespace(model=model, backward=training, sides=lambda lengths: tuple(lengths)))


def test_existing_keys_are_unchanged(monkeypatch):
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.transmil_step import RaggedTransMILStepper
    _clear(monkeypatch)
    count = 0
    for fused_cls in (None, False):                                     # the three fused switches off
        for sw in _all_switches(SWITCHES[:-1], fused_cls=fused_cls):
            for patch_attn, training, sides in itertools.product((False, True), (False, True), ((7,), (7, 16))):
                image, fusion = _steppers(sw, patch_attn, training)
                assert RaggedTransMILStepper.key(image, sides) == _image_key_before(image, sides), (vars(sw), patch_attn, sides)
                assert (RaggedFusionTransMILStepper.key(fusion, 1024, sides) == _fusion_key_before(fusion, 1024, sides)), (vars(sw), sides)
                count += 1
    assert count == 2 * 3 ** 6 * 8
    # and by the environment alone, the attributes None
    sw = SimpleNamespace(**dict.fromkeys(SWITCHES))
    for name in ("MIL_TM_DETERMINISTIC", "MIL_TM_PACKED", "MIL_TM_PACKED_PPEG", "MIL_TM_PACKED_CLS", "MIL_TM_BATCH_BAGS"):
        monkeypatch.setenv(name, "1")
        monkeypatch.setenv("MIL_TM_PIECES", "3")
        for patch_attn in (False, True):
            image, fusion = _steppers(sw, patch_attn)
            assert RaggedTransMILStepper.key(image, (7, 16)) == _image_key_before(image, (7, 16))
            assert RaggedFusionTransMILStepper.key(fusion, 512, (7, 16)) == _fusion_key_before(fusion, 512, (7, 16))
    assert RaggedTransMILStepper.key(image, (7, 16))[4:] == ("patch_attn", "deterministic", ("gemm_pieces", 3), "packed", "ppeg", "cls")


def test_the_fused_switches_are_part_of_the_key_where_they_change_the_launches(monkeypatch):
    """A graph captured with one of them off used to be replayed after it was turned on: no key named them."""
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    from mil_amd.model.dim1 import TransMIL
    from mil_amd.transmil_step import RaggedTransMILStepper
    _clear(monkeypatch)
    ex = TransMIL(2)
    image, fusion = _steppers(ex, patch_attn=True)
    key = lambda sides=(7, 16): RaggedTransMILStepper.key(image, sides)                         # noqa: E731
    fkey = lambda lengths=(49, 256): RaggedFusionTransMILStepper.key(fusion, 1024, lengths)    # noqa: E731
    # fused_cls, a patch_attn model: bag by bag the key changes (one bag, two bags, the attribute, the environment) ...
    off, off_one = key(), key((7,))
    ex.fused_cls = True
    assert key() == off + ("fused_cls",) and key((7,)) == off_one + ("fused_cls",)
    ex.fused_cls = None
    monkeypatch.setenv("MIL_TM_FUSED_CLS", "1")
    assert key() == off + ("fused_cls",)
    monkeypatch.setenv("MIL_TM_FUSED_A1", "1")                          # a1 / a3 are not named beside it: it implies them
    assert key() == off + ("fused_cls",)
    monkeypatch.delenv("MIL_TM_FUSED_A1")
    # ... on the packed route it does not: the cls attention is formed there, whatever fused_cls says
    ex.packed = ex.packed_cls = True
    on = key()
    assert on == off + ("packed", "cls") and key((7,)) == off_one + ("fused_cls",)
    monkeypatch.delenv("MIL_TM_FUSED_CLS")
    assert key() == on and key((7,)) == off_one
    ex.packed = ex.packed_cls = None
    # MIL_TM_FUSED_A1 / _A3 without patch_attn: the same
    image.model.patch_attn = False
    off, f_off = key(), fkey()
    for names, tokens in ((("MIL_TM_FUSED_A1",), ("fused_a1",)), (("MIL_TM_FUSED_A3",), ("fused_a3",)),
                          (("MIL_TM_FUSED_A1", "MIL_TM_FUSED_A3"), ("fused_a1", "fused_a3"))):
        for name in names:
            monkeypatch.setenv(name, "1")
        ex.packed = ex.batch_bags = None
        assert key() == off + tokens and fkey() == f_off + tokens, names
        ex.batch_bags = True                                            # the fused tokens go in front of the route's
        assert key() == off + tokens + ("batch_bags",) and fkey() == f_off + tokens + ("batch_bags",)
        ex.packed = True                                                # both passes run fused there anyway
        assert key() == off + ("packed",) and fkey() == f_off + ("packed",)
        image.model.patch_attn = True                                   # the attention outputs keep the maps: a1 / a3 do not apply
        assert not set(key()) & {"fused_a1", "fused_a3", "packed"}
        image.model.patch_attn = False
        for name in names:
            monkeypatch.delenv(name)
        assert key() == off + ("packed",)


FLAGS = (("deterministic", "deterministic", 1, True), ("tm_gemm_pieces", "gemm_pieces", 3, 3), ("tm_batch_bags", "batch_bags", 1, True),
         ("tm_packed", "packed", 1, True), ("tm_packed_ppeg", "packed_ppeg", 1, True), ("tm_packed_cls", "packed_cls", 1, True))


@pytest.mark.parametrize("flag, attr, given, want", FLAGS)
def test_build_model_sets_the_flag_on_every_transmil_module(flag, attr, given, want):
    from mil_amd.train_ddp import build_model
    others = [a for _, a, _, _ in FLAGS if a != attr] + ["fused_cls"]
    for value, expect in ((given, want), (0, None)):
        image = build_model(argparse.Namespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768,
                                               variant="image_only", **{flag: value}))
        fusion = build_model(SimpleNamespace(modality=["pathology"], model_pathology="TransMIL", model_CI="CLIP", aggregator="TransMIL",
                                             num_classes=2, learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18",
                                             fusion_transmil=1, clip_layers=1, variant="fusion", **{flag: value}))
        for model, n in ((image, 1), (fusion, 2)):
            mods = [m for m in model.modules() if type(m).__name__ == "TransMIL"]
            assert len(mods) == n
            for m in mods:
                assert type(getattr(m, attr)) is type(expect) and getattr(m, attr) == expect, (flag, value)
                assert all(getattr(m, a) is None for a in others), (flag, value)
