"""Host side of the evaluation metrics: the float64 oracle (tests/metrics_ref.py) and the package's own ratio formation
(mil_amd.metrics) against what scikit-learn returned for the cases of tests/golden/metrics_sklearn.json
(tools/gen_metrics_golden.py; scikit-learn itself is never imported here), the --save_best selection rule, and the new flags."""
import json
import os

import numpy as np
import pytest

import metrics_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_sklearn.json")
TOL = 1e-12           # the two sides differ by the float64 rounding of one or two divisions


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


CASES = _cases()
HARD_KEYS = ("acc", "auc_hard", "recall", "precision")
AT_KEYS = ("acc_at", "recall_at", "precision_at")


def _conf(labels, preds, C):
    conf = np.zeros((C, C), np.int64)
    for a, b in zip(labels, preds):
        conf[a, b] += 1
    return conf


def test_golden_covers_the_cases_the_issue_names():
    names = [c["name"] for c in CASES]
    assert len(CASES) >= 24
    assert any("levels4" in n for n in names) and any("only positives" in n for n in names)
    assert any("only negatives" in n for n in names) and any("never predicted" in n for n in names)
    assert any("absent from the labels" in n for n in names)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_matches_sklearn(case):
    exp, C = case["expected"], case["C"]
    got = ref.hard_metrics(case["labels"], case["preds"], C)
    for k in HARD_KEYS:
        assert ref.close(got[k], exp[k], TOL), (k, got[k], exp[k])
    if C == 2:
        s = np.asarray(case["scores"], np.float32)
        at_best = ref.score_metrics(s, case["labels"])
        assert ref.close(at_best["auc"], exp["auc"], TOL), (at_best["auc"], exp["auc"])
        assert at_best["best_thres"] == exp["best_thres"]                 # equal, not close
        at_thres = ref.score_metrics(s, case["labels"], exp["thres"])
        for k in AT_KEYS:
            assert ref.close(at_best[k], exp["at_best"][k], TOL), (k, at_best[k], exp["at_best"][k])
            assert ref.close(at_thres[k], exp["at_thres"][k], TOL), (k, at_thres[k], exp["at_thres"][k])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_package_ratios_match_sklearn(case):
    """mil_amd.metrics forms the same values from the integers the reduce kernel returns (here: the oracle's integers)."""
    from mil_amd import metrics as M
    exp, C = case["expected"], case["C"]
    got = M.hard_metrics(_conf(case["labels"], case["preds"], C))
    for k in HARD_KEYS:
        assert ref.close(got[k], exp[k], TOL), (k, got[k], exp[k])
    if C != 2:
        return
    s, lab = np.asarray(case["scores"], np.float32), np.asarray(case["labels"])
    ints = ref.reduce_ints(s, lab)
    for thres, want in ((None, exp["at_best"]), (exp["thres"], exp["at_thres"])):
        tp = int(((s >= np.float64(thres)) & (lab == 1)).sum()) if thres is not None else 0
        fp = int(((s >= np.float64(thres)) & (lab != 1)).sum()) if thres is not None else 0
        m = M.score_metrics(len(s), ints["P"], ints["S2"], ints["jstar"], ints["sstar"], ints["ge_pos"], ints["ge_neg"], tp, fp,
                            thres)
        assert ref.close(m["auc"], exp["auc"], TOL) and m["best_thres"] == exp["best_thres"]
        for k in AT_KEYS:
            assert ref.close(m[k], want[k], TOL), (k, thres, m[k], want[k])


def test_oracle_losses_follow_torch():
    import torch
    g = torch.Generator().manual_seed(3)
    for B, C in ((1, 2), (3, 2), (8, 5), (3, 5)):
        p = torch.rand((B, C), generator=g)
        p[0, 0], p[0, 1] = 0.0, 1.0                                        # the -100 clamp
        y = torch.eye(C)[torch.randint(0, C, (B,), generator=g)]
        crit = torch.nn.CrossEntropyLoss() if C > 2 else torch.nn.BCELoss()
        want = float(crit(p.double(), y.double()))
        assert ref.close(ref.criterion(p.numpy(), y.numpy()), want, 1e-12)


def test_select_best_history():
    from mil_amd.metrics import select_best
    nan = float("nan")
    best, saved = 0.0, []
    for auc in (0.5, nan, 0.5, 0.4, 0.7, nan, 0.7, 0.69):
        save, best = select_best(auc, best, True)
        saved.append(save)
    assert saved == [True, False, True, False, True, False, True, False] and best == 0.7
    assert select_best(0.0, 0.0, True) == (True, 0.0)                     # the reference's 0 <= 0
    save, best = select_best(nan, 0.0, True)
    assert not save and best == 0.0                                       # nan never beats a number
    for auc in (0.1, nan, 0.0):                                           # --save_best off: every epoch, as before
        assert select_best(auc, 0.9, False) == (True, 0.9)


def test_new_flags_parse_and_default_off():
    from mil_amd.config import create_arg_parser
    from mil_amd.evaluate import parse_args
    a = create_arg_parser([])
    assert a.validate == 0 and a.save_best is False and a.index_json_valid == ""
    b = create_arg_parser(["--validate", "1", "--save_best", "--index_json_valid", "v.json"])
    assert b.validate == 1 and b.save_best is True and b.index_json_valid == "v.json"
    # the reporting flags belong to evaluate.py: its parser takes them next to test_ddp.py's, the shared one refuses them
    e = parse_args(["--best_thres", "0.25"])
    assert e.report_metrics == 0 and e.mode == "test" and e.best_thres == 0.25
    e = parse_args(["--report_metrics", "1", "--num_classes", "2", "--mode", "valid"])
    assert e.report_metrics == 1 and e.mode == "valid" and e.num_classes == 2
    for argv in (["--mode", "train"], ["--report_metrics", "2"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    with pytest.raises(SystemExit):
        create_arg_parser(["--report_metrics", "1"])


def test_checkpoint_files_follow_the_selection(tmp_path):
    """train_ddp.write_checkpoints on a hand-made history: which files exist and which epoch checkpoint_best holds."""
    import torch
    from mil_amd.train_ddp import write_checkpoints
    nan = float("nan")

    def files(d):
        return sorted(f[len("checkpoint_"):-len(".pth.tar")] for f in os.listdir(d))

    def epoch_of(d, name):
        return torch.load(os.path.join(d, f"checkpoint_{name}.pth.tar"), weights_only=True)["epoch"]

    d = str(tmp_path / "best")
    os.makedirs(d)
    best = 0.0
    for epoch, auc in enumerate((0.6, 0.5, nan, 0.6, 0.55)):                # kept: 0 and 3 (equality replaces)
        best = write_checkpoints({"epoch": epoch + 1}, d, epoch, True, auc, best, True)
        assert epoch_of(d, "last") == epoch + 1
    assert files(d) == ["0000", "0003", "best", "last"] and best == 0.6 and epoch_of(d, "best") == 4
    d = str(tmp_path / "every")
    os.makedirs(d)
    for epoch, auc in enumerate((0.6, nan)):                                # --save_best off: every epoch, plus last
        write_checkpoints({"epoch": epoch + 1}, d, epoch, True, auc, 0.0, False)
    assert files(d) == ["0000", "0001", "best", "last"] and epoch_of(d, "best") == 2
    d = str(tmp_path / "plain")
    os.makedirs(d)
    for epoch in range(2):                                                  # no --validate: the parent's file set
        write_checkpoints({"epoch": epoch + 1}, d, epoch, False, None, 0.0, False)
    assert files(d) == ["0000", "0001", "best"]


def test_abi_and_header_carry_the_metrics_entries():
    from mil_amd import _lib
    assert _lib.ABI_VERSION >= 24
    for name in ("mil_eval_push", "mil_eval_rank", "mil_eval_reduce", "mil_eval_out_bytes"):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols()
    from mil_amd.ops import metrics as om
    text = open(_lib.HEADER_PATH).read()
    for macro, val in (("MIL_EVAL_TILE", om.EVAL_TILE), ("MIL_EVAL_MAX_ROWS", om.EVAL_MAX_ROWS), ("MIL_EVAL_OUT_WORDS", om.EVAL_OUT_WORDS),
                       ("MIL_EVAL_OUT_LOSS", om.EVAL_OUT_LOSS), ("MIL_EVAL_OUT_SSTAR", om.EVAL_OUT_SSTAR),
                       ("MIL_EVAL_LOSS_SLOTS", om.EVAL_LOSS_SLOTS)):
        assert f"#define {macro} {val}" in text, macro
