#!/usr/bin/env python3
"""Writes tests/golden/metrics_sklearn.json: small evaluation cases and what scikit-learn returns for them through the calls
the reference makes - valid() on the argmax predictions (train_ddp.py:497-509: roc_auc_score, recall_score, precision_score
with zero_division = nan, one-hot rows above two classes) and test_ddp.py on the scores (:141-162, :286-309: roc_curve +
argmax(tpr - fpr), roc_auc_score, then accuracy / recall / precision of score >= threshold).  A call that raises is recorded
as nan.  The tests read the file and never import scikit-learn.

    python tools/gen_metrics_golden.py            # needs scikit-learn (generated with 1.7.2)"""
import json
import os
import warnings

import numpy as np
from sklearn.metrics import accuracy_score, precision_score, recall_score, roc_auc_score, roc_curve

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "metrics_sklearn.json")


def guarded(fn, *a, **k):
    try:
        return float(fn(*a, **k))
    except ValueError:
        return float("nan")


def hard_expected(labels, preds, C):
    labels, preds = list(labels), list(preds)
    if C > 2:
        return {"acc": float(accuracy_score(labels, preds)),
                "auc_hard": guarded(roc_auc_score, np.eye(C)[labels], np.eye(C)[preds], multi_class="ovo", average="macro"),
                "recall": guarded(recall_score, labels, preds, average="macro", zero_division=np.nan),
                "precision": guarded(precision_score, labels, preds, average="macro", zero_division=np.nan)}
    return {"acc": float(accuracy_score(labels, preds)), "auc_hard": guarded(roc_auc_score, labels, preds),
            "recall": guarded(recall_score, labels, preds, zero_division=np.nan),
            "precision": guarded(precision_score, labels, preds, zero_division=np.nan)}


def at_expected(labels, scores, thres):
    hard = [bool(s >= thres) for s in scores]
    lab = [bool(v) for v in labels]
    return {"acc_at": float(accuracy_score(lab, hard)), "recall_at": guarded(recall_score, lab, hard),
            "precision_at": guarded(precision_score, lab, hard)}


def score_expected(labels, scores, thres):
    fpr, tpr, thresholds = roc_curve(labels, scores)
    best = float(thresholds[int(np.argmax(tpr - fpr))])
    return {"auc": guarded(roc_auc_score, labels, scores), "best_thres": best, "at_best": at_expected(labels, scores, best),
            "thres": thres, "at_thres": at_expected(labels, scores, thres)}


def main():
    rng = np.random.default_rng(20240611)
    cases = []

    def binary(name, labels, scores, preds=None, thres=0.5):
        scores = np.asarray(scores, np.float32)
        labels = [int(v) for v in labels]
        preds = [int(s > 0.5) for s in scores] if preds is None else [int(v) for v in preds]   # argmax of (1 - s, s)
        exp = hard_expected(labels, preds, 2)
        exp.update(score_expected(labels, scores.astype(np.float64), thres))
        cases.append({"name": name, "C": 2, "labels": labels, "preds": preds, "scores": [float(s) for s in scores],
                      "expected": exp})

    def multi(name, labels, preds, C=4):
        labels, preds = [int(v) for v in labels], [int(v) for v in preds]
        cases.append({"name": name, "C": C, "labels": labels, "preds": preds, "expected": hard_expected(labels, preds, C)})

    for k, n in enumerate((2, 3, 7, 16, 33, 64)):
        for levels in (4, 16, 0):
            lab = rng.integers(0, 2, n)
            if lab.min() == lab.max():
                lab[0] = 1 - lab[0]
            raw = rng.random(n) * 0.6 + 0.3 * lab * rng.random(n)
            s = np.round(raw * levels) / levels if levels else raw
            binary(f"binary n{n} levels{levels}", lab, np.clip(s, 0.0, 1.0), thres=(0.5, 0.25, 0.3)[k % 3])
    binary("binary all scores equal", [0, 1, 1, 0, 1], [0.5] * 5)
    binary("binary inverted", [1, 1, 0, 0], [0.1, 0.2, 0.8, 0.9])
    binary("binary separable", [0, 0, 1, 1, 1], [0.1, 0.2, 0.7, 0.8, 0.9])
    binary("binary only positives", [1, 1, 1, 1], [0.2, 0.9, 0.9, 0.4])
    binary("binary only negatives", [0, 0, 0], [0.2, 0.9, 0.4])
    binary("binary only negatives, none predicted", [0, 0, 0], [0.2, 0.1, 0.4])
    binary("binary never predicts positive", [0, 1, 1, 0], [0.1, 0.2, 0.3, 0.4])
    for n in (9, 40):
        lab, prd = rng.integers(0, 4, n), rng.integers(0, 4, n)
        lab[:4] = prd[:4] = np.arange(4)
        multi(f"C4 n{n} all classes", lab, prd)
        prd2 = np.where(prd == 2, 0, prd)
        multi(f"C4 n{n} class 2 never predicted", lab, prd2)
        lab2 = np.where(lab == 3, 1, lab)
        multi(f"C4 n{n} class 3 absent from the labels", lab2, prd)
        multi(f"C4 n{n} class 3 absent from labels and predictions", lab2, np.where(prd == 3, 0, prd))
    multi("C4 one label class only", [1, 1, 1], [1, 0, 1])
    multi("C5 n17", rng.integers(0, 5, 12).tolist() + [0, 1, 2, 3, 4], rng.integers(0, 5, 17), C=5)
    # one case per line; nan and +inf are written as Python's json writes and reads them (NaN, Infinity)
    with open(OUT, "w") as f:
        f.write('{"sklearn": %s, "cases": [\n' % json.dumps(__import__("sklearn").__version__))
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")
    print(f"{len(cases)} cases -> {OUT}")


if __name__ == "__main__":
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        main()
