#!/usr/bin/env python3
"""Evaluation with metrics: the entry point `python evaluate.py ... --report_metrics 1 [--mode valid]` and the per-bag loop
it shares with train_ddp.py's validation (reference: test_ddp.py:214-253, batch 1, eval mode, no grad): every bag one forward
with its true length, through the replayed forward where the flags select one (model.graph_eval,
fusion_step.RaggedFusionInference) and the eager one otherwise, fed from an HBM-resident cohort (cohort.DeviceCohort,
augment=False) when it fits.  The loop is test_ddp.py's own, bag for bag (tests/test_gpu_metrics.py holds the two to the same
predictions, bit for bit); test_ddp.py itself stays as it was, and its parser refuses the two flags of this entry point.

As an entry point it takes test_ddp.py's flags, loads `checkpoint_best.pth.tar` strictly and prints test_ddp.py's line; with
`--report_metrics 1` the predictions go through a metrics.EvalLog instead of a host read per bag and the run closes with the
reference's `Result : Loss .. AUC .. Accuracy .. Precision .. Recall .. | Threshold ..` line (test_ddp.py:160), at
`--best_thres` or, with `--mode valid`, at the Youden threshold found on this set.  The ROC plot and the Excel sheet stay out
of scope.

The reference's valid() pads a batch of bags with zero rows to a common length (dataset.py:386-391) and lets the model see the
padding, which changes the result; here a bag is never padded.

With a metrics.EvalLog every forward is followed by one push on the same stream - outside any graph, so no graph key or stepper
changes - and nothing is read on the host inside the loop; without one, the loop reads each bag's probability as before."""
import os
import sys
import time

import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import mil_amd  # noqa: F401
    __package__ = "mil_amd"

from .dataset import collate_bags, load_cohort  # noqa: E402

CT_SHAPE = (512, 160, 2, 2)              # synthetic stand-in for the CT encoder's feature map (aggregator.py:139-140)


class BagEvaluator:
    """Built once per cohort (the inference graphs and the resident cohort are kept between passes), run once per pass."""

    def __init__(self, args, model, data, dev, prompts: int):
        self.args, self.model, self.data, self.dev, self.prompts = args, model, data, dev, prompts
        self.with_ct = args.variant != "image_only" and "CT" in args.modality
        self.three_terms = (args.loss_point == "CT-Pth-Last" and "CT" in args.modality and "pathology" in args.modality)
        self.inf = None
        if (getattr(args, "hip_graph", 0) and args.variant != "image_only" and not args.learnablePrompt and prompts <= 12
                and list(args.modality) in (["pathology"], ["CT", "pathology"])):
            # one forward is ~70 short launches: replay it from a hipGraph per capacity bucket (fusion_step.RaggedFusionInference)
            from .fusion_step import RaggedFusionInference
            self.inf = RaggedFusionInference(model, B=1, P=prompts, in_dim=args.patch_dim,
                                             ct_shape=CT_SHAPE if self.with_ct else None)
        self.cohort = None
        if self.inf is not None and getattr(args, "resident_cohort", 1):
            # the evaluation cohort resident in HBM too (cohort.DeviceCohort, no patch drop at test time: dataset.py:374 is
            # train-only): one feed launch per bag instead of np.load + pageable copy
            from .cohort import DeviceCohort
            lens_all = ([int(v) for v in data.lengths] if hasattr(data, "lengths") else None)
            if lens_all is None:
                import numpy as _np
                lens_all = [int(_np.load(os.path.join(data.root, k + ".npy"), mmap_mode="r").shape[0]) for k in data.keys]
            if DeviceCohort.fits(DeviceCohort.bytes_needed(lens_all, args.patch_dim), dev):
                self.cohort = DeviceCohort.from_dataset(data, dev, seed=args.seed, augmentation=False)
                self.cohort.draw_epoch(0, augment=False)

    @property
    def nterm(self) -> int:
        return 3 if self.three_terms else 1

    def _push(self, log, out, heads, toks, y):
        """One launch behind the forward: the Last head (and the CT / Pth heads under 'CT-Pth-Last': one head here, so the same
        term three times, as train_ddp.py's total_loss), the cosine term when both text-aligned tokens came back."""
        extra = None
        if "textCosSim" in self.args.loss and len(toks) == 2:
            from . import ops
            extra = ops.cosine_embedding_loss(toks[0].squeeze(1), toks[1].squeeze(1)).reshape(1)
        if self.three_terms:
            terms = (heads + [out, out])[:3] if heads else [out, out, out]
            log.push(terms, y, extra)
        else:
            log.push(out, y, extra)

    def run(self, log=None, timed: bool = True, read: bool = True):
        """(preds, labels, times).  log None: preds = float(out[0, 1]) per bag, read on the spot (a sync per bag).  With a log:
        one push per forward, preds and labels read from the log ONCE at the end (read=False: not at all); timed=False drops
        the per-bag synchronize, so that the loop holds no host read."""
        args, model, data, dev, inf, cohort, with_ct = self.args, self.model, self.data, self.dev, self.inf, self.cohort, self.with_ct
        preds, labels, times = [], [], []
        with torch.no_grad():
            for i in range(len(data)):                                     # batch_size = 1 (test_ddp.py:73)
                if cohort is not None and not with_ct:
                    n = cohort.n[i]
                    slot = inf.slot(n)
                    if slot.bucket.fits([n]):
                        if timed:
                            torch.cuda.synchronize()
                            t0 = time.time()
                        ks = cohort.feed([i], slot.x, slot.bucket.len_dev, ids_dst=slot.ids)
                        out = inf.forward(slot, ks, on_device=True)
                        if timed:
                            torch.cuda.synchronize()
                            times.append(time.time() - t0)
                        if log is not None:
                            self._push(log, out, [], [], cohort.labels[i:i + 1])
                        else:
                            preds.append(float(out[0, 1]))
                            labels.append(int(cohort.labels[i].argmax()))
                        continue
                b = collate_bags([data[i]])
                x = b["pathology"].to(dev)
                ct = None
                if with_ct:
                    from . import synthetic as syn
                    ct = syn.make_ct_map(args.seed + 104729 + i, 1, CT_SHAPE[1], CT_SHAPE[2]).to(dev)
                y = b["label"].to(dev) if log is not None else None
                if timed:
                    torch.cuda.synchronize()
                    t0 = time.time()
                heads, toks = [], []
                if args.variant == "image_only":
                    _, out = model([x])
                elif inf is not None:
                    n = int(b["lengths"][0])
                    slot = inf.slot(n)
                    slot.x[:n].copy_(x[0, :n], non_blocking=True)
                    if ct is not None:
                        slot.ct.copy_(ct, non_blocking=True)
                    slot.ids.copy_(b["CI"], non_blocking=True)                 # the text tower is part of the replayed forward
                    out = inf.forward(slot, [n])
                else:
                    xs = [x] if ct is None else ([ct, x] if "pathology" in args.modality else [ct])
                    out = model(xs, b["CI"].to(dev))
                    if isinstance(out, tuple) and isinstance(out[0], list):
                        heads, toks = list(out[0]), [t_ for t_ in out[1] if t_ is not None]
                    elif isinstance(out, tuple):
                        toks = [t_ for t_ in out[1:] if torch.is_tensor(t_)]
                    out = out[0][0] if isinstance(out[0], list) else (out[0] if isinstance(out, tuple) else out)
                if timed:
                    torch.cuda.synchronize()
                    times.append(time.time() - t0)
                if log is not None:
                    self._push(log, out, heads, toks, y.to(torch.float32))
                else:
                    preds.append(float(out[0, 1]))
                    labels.append(int(b["label"][0].argmax()))
        if log is not None and read:
            probs, cls = log.read()                                        # the one read of the pass
            preds, labels = [float(p) for p in probs[:, 1]], [int(c) for c in cls[:, 0]]
        return preds, labels, times


def parse_args(argv=None):
    """test_ddp.py's flags (config.create_arg_parser) and the two of this entry point: --report_metrics {0,1} (default 0) and
    --mode {valid,test} (default test).  They are parsed here, not in config.py, so that train_ddp.py and test_ddp.py, which
    have no use for them, refuse them as unknown arguments."""
    import argparse
    from .config import create_arg_parser
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--report_metrics", type=int, default=0, choices=[0, 1])
    p.add_argument("--mode", type=str, default="test", choices=["valid", "test"])
    own, rest = p.parse_known_args(argv)
    args = create_arg_parser(rest)
    args.report_metrics, args.mode = own.report_metrics, own.mode
    return args


def evaluate(args):
    """test_ddp.py's test(args) over the shared loop: returns (preds, labels); with --report_metrics 1 both are read from the
    log once at the end."""
    from .train_ddp import build_model
    if not torch.cuda.is_available():
        raise NotImplementedError("the MIL hot path runs on MI355X only: no GPU is visible")
    dev = torch.device("cuda", int(args.gpu.split(",")[0]))
    torch.cuda.set_device(dev)
    prompts = 10 if args.CI_prompt_version == "devided" else 1
    if args.learnablePrompt:
        prompts = len(args.clinical_features) + 1
    data, args.patch_dim = load_cohort(args, "test", prompts)
    model = build_model(args).to(dev)
    if args.test_pth:
        ck = torch.load(os.path.join(args.test_pth, "checkpoint_best.pth.tar"), map_location=dev, weights_only=True)
        model.load_state_dict(ck["state_dict"])                       # strict, as test_ddp.py:99
    model.eval()
    ev = BagEvaluator(args, model, data, dev, prompts)
    log = None
    if getattr(args, "report_metrics", 0):
        from .metrics import EvalLog
        log = EvalLog(len(data), args.num_classes, ev.nterm, dev)
    preds, labels, times = ev.run(log)
    hard = [1 if p >= args.best_thres else 0 for p in preds]
    acc = sum(int(a == b) for a, b in zip(hard, labels)) / len(labels)
    print(f"bags {len(labels)}  ACC@{args.best_thres:.4f} {acc:.4f}  Time for inference {1e3 * sum(times[1:]) / max(1, len(times) - 1):.3f} ms/bag")
    if log is not None:
        # --mode valid: the Youden threshold found on this set; --mode test: the one typed in (test_ddp.py:141-162)
        m = log.finish(None if args.mode == "valid" else args.best_thres)
        print("Result : Loss %.4e   AUC %.4f   Accuracy %.4f   Precision %.4f   Recall %.4f | Threshold %.4f" % (
            m["loss"], m.get("auc", m["auc_hard"]), m.get("acc_at", m["acc"]), m.get("precision_at", m["precision"]),
            m.get("recall_at", m["recall"]), m.get("thres", float("nan"))))
    return preds, labels


if __name__ == "__main__":
    evaluate(parse_args())
