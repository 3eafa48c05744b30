"""One synthetic validation epoch, timed twice in one process: the per-bag host read against the device-side log.

Per model (image-only ABMIL; image-only TransMIL with --transmil_graph 1, its eval forward replayed per grid side), --bags ragged
bags resident on the device, eval mode, no grad, one bag per forward:
  baseline  the loop test_ddp.py runs for these models, written here: float(out[0, 1]) per bag (one device -> host sync per
            bag) and the label from the host copy of the batch (no launch, no sync), then accuracy, AUC and the Youden
            threshold with numpy on the host (sorted scores and cumulative counts: no Python loop over the bags)
  log       metrics.EvalLog: one push launch behind each forward, nothing read inside the loop, finish() at the end
The two alternate region by region (baseline, log, baseline, ..), --reps regions each after one untimed epoch of either (which
also captures the TransMIL graphs); a region is one whole epoch, wall clock between two synchronizes.  Prints one JSON line per
model with the median (min - max) of both in ms, per epoch and per bag."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import mil_amd  # noqa: E402,F401
from mil_amd import train_ddp  # noqa: E402
from mil_amd.config import create_arg_parser  # noqa: E402
from mil_amd.metrics import EvalLog  # noqa: E402


def host_metrics(preds, labels):
    """What a host-side loop computes from the per-bag reads: accuracy at 0.5, AUC (pairs, ties half), Youden threshold."""
    s, lab = np.asarray(preds, np.float64), np.asarray(labels)
    pos, neg = s[lab == 1], s[lab == 0]
    auc = float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / max(1, len(pos) * len(neg)))
    best_t = np.inf
    if len(pos) and len(neg):
        order = np.argsort(-s, kind="stable")
        last = np.r_[np.diff(s[order]) != 0, True]          # the last sample of each distinct score, scores decreasing
        j = np.cumsum(lab[order] == 1)[last] / len(pos) - np.cumsum(lab[order] == 0)[last] / len(neg)
        if j.max() > 0:
            best_t = float(s[order][last][int(np.argmax(j))])
    return {"acc": float(((s >= 0.5) == (lab == 1)).mean()), "auc": auc, "best_thres": best_t}


def bench(name, argv, bags, nmin, nmax, F, reps, dev):
    args = create_arg_parser(["--variant", "image_only", "--synthetic", f"[{nmax}, {F}, {bags}]", *argv])
    torch.manual_seed(1)
    model = train_ddp.build_model(args).to(dev).eval()
    g = torch.Generator().manual_seed(2)
    lens = [int(v) for v in torch.randint(nmin, nmax + 1, (bags,), generator=g)]
    xs = [torch.randn((1, n, F), generator=g).to(dev) for n in lens]
    cls = torch.randint(0, 2, (bags,), generator=g)
    ys_host = [torch.eye(2)[int(c)].reshape(1, 2) for c in cls]         # the batch's label as the data loader hands it over
    ys = [y.to(dev) for y in ys_host]
    log = EvalLog(bags, 2, 1, dev)

    def baseline():
        preds, labels = [], []
        for x, y in zip(xs, ys_host):
            _, out = model([x])
            preds.append(float(out[0, 1]))                  # the sync per bag
            labels.append(int(y[0].argmax()))               # host tensor, as test_ddp.py's b["label"][0].argmax()
        return host_metrics(preds, labels)

    def logged():
        log.reset()
        for x, y in zip(xs, ys):
            _, out = model([x])
            log.push(out, y)
        return log.finish()

    t = {"baseline": [], "log": []}
    with torch.no_grad():
        a, b = baseline(), logged()                         # untimed: graph captures, first launches
        for _ in range(reps):
            for key, fn in (("baseline", baseline), ("log", logged)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[key].append(1e3 * (time.perf_counter() - t0))
    row = {"model": name, "bags": bags, "patches": [min(lens), max(lens)], "auc_baseline": a["auc"], "auc_log": b["auc"],
           "best_thres_equal": a["best_thres"] == b["best_thres"]}
    for key, v in t.items():
        v = sorted(v)
        row[f"{key}_ms"] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3),
                            "per_bag_median": round(v[len(v) // 2] / bags, 4)}
    row["log_over_baseline"] = round(row["log_ms"]["median"] / row["baseline_ms"]["median"], 4)
    print(json.dumps(row), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bags", type=int, default=200)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--models", nargs="*", default=["ABMIL", "TransMIL"])
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if "ABMIL" in a.models:
        bench("ABMIL", [], a.bags, 256, 1024, 768, a.reps, dev)
    if "TransMIL" in a.models:
        bench("TransMIL --transmil_graph 1", ["--model_pathology", "TransMIL", "--transmil_graph", "1"], a.bags, 1000, 2000, 768,
              a.reps, dev)


if __name__ == "__main__":
    main()
