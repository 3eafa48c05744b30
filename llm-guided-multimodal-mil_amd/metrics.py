"""Validation / test metrics from a device-side evaluation log (csrc/metrics.hip, ops/metrics.py).

`EvalLog` keeps what the reference's valid() (train_ddp.py:382-513) and test_ddp.py (:141-162, :286-309) gather on the host -
per-bag probabilities, label and predicted classes, per-step criterion values - in device buffers: one small launch per step
(`push`), nothing read on the host until `finish()`, which launches the all-pairs rank pass and one reduce and copies a few
hundred bytes back.  Every count is an integer, so the results are exact and the same from run to run; the final ratios are
formed here on the host in float64 (`derive`).  `select_best` is the reference's `--save_best` rule (train_ddp.py:214-227)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

NAN = float("nan")


def _div(a: float, b: float, zero: float = NAN) -> float:
    return float(a) / float(b) if b else zero


def _nanmean(vals) -> float:
    kept = [v for v in vals if not math.isnan(v)]
    return sum(kept) / len(kept) if kept else NAN


def hard_metrics(conf: np.ndarray) -> Dict[str, float]:
    """acc, auc_hard, recall, precision of the argmax predictions from the confusion matrix conf[label][pred] - what valid()
    gets from sklearn (train_ddp.py:497-509).  C <= 2: roc_auc_score(labels, preds) = (TPR + TNR) / 2 and the positive class's
    recall / precision with zero_division = nan.  C > 2: roc_auc_score on one-hot rows (np.eye(C); the reference hard-codes 5),
    i.e. the macro mean of the per-class (TPR_c + TNR_c) / 2, and macro recall / precision over the classes present among the
    labels or the predictions, a 0 / 0 class left out of the mean (zero_division = nan).  A class absent from the labels makes
    the AUC nan (sklearn raises)."""
    conf = np.asarray(conf, dtype=np.int64)
    C, n = conf.shape[0], int(conf.sum())
    out = {"acc": _div(int(np.trace(conf)), n)}
    lab, prd, tp = conf.sum(1), conf.sum(0), np.diag(conf)
    if C <= 2:
        P = int(lab[1]) if C == 2 else 0
        N = n - P
        TP = int(tp[1]) if C == 2 else 0
        TN = int(tp[0])
        out["auc_hard"] = (TP / P + TN / N) / 2.0 if P and N else NAN
        out["recall"] = _div(TP, P)
        out["precision"] = _div(TP, int(prd[1]) if C == 2 else 0)
        return out
    aucs, rec, pre = [], [], []
    for c in range(C):
        Pc, Nc = int(lab[c]), n - int(lab[c])
        tn = n - int(lab[c]) - int(prd[c]) + int(tp[c])
        aucs.append((int(tp[c]) / Pc + tn / Nc) / 2.0 if Pc and Nc else NAN)
        if lab[c] or prd[c]:
            rec.append(_div(int(tp[c]), Pc))
            pre.append(_div(int(tp[c]), int(prd[c])))
    out["auc_hard"] = NAN if any(math.isnan(a) for a in aucs) else sum(aucs) / C
    out["recall"], out["precision"] = _nanmean(rec), _nanmean(pre)
    return out


def score_metrics(n: int, P: int, S2: int, jstar: int, sstar: float, ge_pos: int, ge_neg: int, tp_at: int, fp_at: int,
                  thres: Optional[float]) -> Dict[str, float]:
    """The binary score metrics of test_ddp.py:141-162,286-309 from the integers of the reduce: auc = S2 / (2 P N) is
    roc_auc_score(labels, score) (ties count half), best_thres = roc_curve + argmax(tpr - fpr) = the score of the Youden index
    when J* > 0 and +inf (roc_curve's first threshold) otherwise.  recall_at / precision_at / acc_at classify score >= thres as
    positive, at the given threshold or, with thres None, at best_thres; as sklearn's default zero_division they are 0 on 0 / 0."""
    N = n - P
    best = float(sstar) if jstar > 0 else math.inf
    if thres is None:
        thres, tp_at, fp_at = best, (ge_pos if jstar > 0 else 0), (ge_neg if jstar > 0 else 0)
    return {"auc": _div(S2, 2 * P * N), "best_thres": best, "thres": float(thres), "recall_at": _div(tp_at, P, 0.0),
            "precision_at": _div(tp_at, tp_at + fp_at, 0.0), "acc_at": _div(tp_at + (N - fp_at), n)}


def derive(counts: Dict[str, object], thres: Optional[float] = None) -> Dict[str, float]:
    """Every reported value from the integers and the double loss sums of one reduce (EvalLog.finish's `counts`)."""
    sums, nb = counts["loss_sums"], counts["loss_weight"]
    out = {k: _div(sums[i], nb) for i, k in enumerate(("loss_last", "loss_ct", "loss_pth", "loss_cossim"))}
    out["loss"] = _div(sum(sums), nb)
    out.update(hard_metrics(counts["conf"]))
    if counts["conf"].shape[0] == 2:
        out.update(score_metrics(counts["n"], counts["P"], counts["S2"], counts["jstar"], counts["sstar"], counts["ge_pos"],
                                 counts["ge_neg"], counts["tp_at"], counts["fp_at"], thres))
    return out


def select_best(auc_hard: float, best: float, save_best: bool) -> Tuple[bool, float]:
    """(write checkpoint_{epoch:04d} + checkpoint_best this epoch?, the best validation AUC afterwards).  Without --save_best
    every epoch is written; with it only an epoch whose AUC is >= the best so far - equality replaces, as the reference's
    `valid_auc_best <= valid_auc` (train_ddp.py:216); the best starts at 0 there.  nan never beats a number."""
    if not save_best:
        return True, best
    if auc_hard is not None and not math.isnan(auc_hard) and best <= auc_hard:
        return True, float(auc_hard)
    return False, best


class EvalLog:
    """Device-side log of an evaluation pass over at most `capacity` bags of a `C`-class model whose loss has `nterm` criterion
    terms (1: 'Last'; 3: 'CT-Pth-Last').  push() is one launch on the current stream and reads nothing on the host, and it is
    capture-safe: the row index lives in a device counter.  finish() is the only host read."""

    def __init__(self, capacity: int, C: int, nterm: int = 1, device=None):
        import torch
        from .ops import metrics as om
        if not 1 <= int(capacity) <= om.EVAL_MAX_ROWS:
            raise ValueError(f"EvalLog: capacity {capacity} is outside 1..{om.EVAL_MAX_ROWS}")
        if not 1 <= int(nterm) <= om.EVAL_MAX_TERMS:
            raise ValueError(f"EvalLog: nterm {nterm} is outside 1..{om.EVAL_MAX_TERMS}")
        self._torch, self._om = torch, om
        self.capacity, self.C, self.nterm = int(capacity), int(C), int(nterm)
        self.ce = self.C > 2                                           # train_ddp.py:95-98
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = dev
        self.log_prob = torch.zeros((self.capacity, self.C), device=dev, dtype=torch.float32)
        self.log_cls = torch.zeros((self.capacity, 2), device=dev, dtype=torch.int32)
        self.step_b = torch.zeros((self.capacity,), device=dev, dtype=torch.int32)
        self.step_loss = torch.zeros((self.capacity, om.EVAL_LOSS_SLOTS), device=dev, dtype=torch.float64)
        self.ctr = torch.zeros((4,), device=dev, dtype=torch.int32)
        self.rank = torch.zeros((self.capacity, 3), device=dev, dtype=torch.int32) if self.C == 2 else None
        self.out = torch.zeros((om.eval_out_bytes(self.C) // 8,), device=dev, dtype=torch.int64)

    def reset(self) -> None:
        self.ctr.zero_()

    def push(self, probs, y, extra=None) -> None:
        """probs: the Last head's [B, C] probabilities, or a sequence (Last, CT, Pth) of `nterm` of them; y [B, C] one-hot
        fp32; extra: a device scalar added to the total loss (the textCosSim term)."""
        if self._torch.is_tensor(probs):
            probs = (probs,)
        if len(probs) != self.nterm:
            raise ValueError(f"EvalLog.push: {len(probs)} terms given, the log was built for {self.nterm}")
        if probs[0].shape[-1] != self.C:
            raise ValueError(f"EvalLog.push: {probs[0].shape[-1]} classes given, the log was built for {self.C}")
        self._om.eval_push(probs, y, extra, self.ce, self.capacity, self.log_prob, self.log_cls, self.step_b, self.step_loss,
                           self.ctr)

    def _reduce(self, thres: Optional[float]) -> Dict[str, object]:
        om = self._om
        if self.rank is not None:
            om.eval_rank(self.log_prob, self.log_cls, self.ctr, self.capacity, self.rank)
        om.eval_reduce(self.log_prob, self.log_cls, self.step_b, self.step_loss, self.ctr, self.rank, self.capacity, self.C,
                       math.inf if thres is None else float(thres), self.out)
        raw = self.out.cpu().numpy()                                   # the one device -> host copy
        w = raw[:om.EVAL_OUT_WORDS]
        d = w.view(np.float64)
        conf = raw[om.EVAL_OUT_WORDS:].view(np.int32)[:self.C * self.C].reshape(self.C, self.C).astype(np.int64)
        return {"n": int(w[om.EVAL_OUT_N]), "steps": int(w[om.EVAL_OUT_STEPS]), "flag": int(w[om.EVAL_OUT_FLAG]),
                "P": int(w[om.EVAL_OUT_P]), "N": int(w[om.EVAL_OUT_NEG]), "S2": int(w[om.EVAL_OUT_S2]),
                "tp_at": int(w[om.EVAL_OUT_TP_AT]), "fp_at": int(w[om.EVAL_OUT_FP_AT]), "jstar": int(w[om.EVAL_OUT_JSTAR]),
                "istar": int(w[om.EVAL_OUT_ISTAR]), "ge_pos": int(w[om.EVAL_OUT_GE_POS]), "ge_neg": int(w[om.EVAL_OUT_GE_NEG]),
                "sstar": float(d[om.EVAL_OUT_SSTAR]),
                "loss_sums": [float(v) for v in d[om.EVAL_OUT_LOSS:om.EVAL_OUT_LOSS + om.EVAL_LOSS_SLOTS]],
                "loss_weight": float(d[om.EVAL_OUT_LOSS + om.EVAL_LOSS_SLOTS]), "conf": conf}

    def finish(self, thres: Optional[float] = None) -> Dict[str, object]:
        """Rank + reduce, one copy back, the ratios in float64.  thres: the threshold of recall_at / precision_at / acc_at
        (None: the Youden threshold found on this log).  Raises RuntimeError when a push was dropped or a probability was NaN.
        The integers themselves are under "counts"."""
        counts = self._reduce(thres)
        if counts["flag"] & self._om.EVAL_FLAG_OVERFLOW:
            raise RuntimeError(f"EvalLog: a push went beyond the capacity of {self.capacity} bags and was dropped")
        if counts["flag"] & self._om.EVAL_FLAG_NAN:
            raise RuntimeError("EvalLog: a pushed probability was NaN")
        out = derive(counts, thres)
        out["counts"] = counts
        return out

    def read(self) -> Tuple[np.ndarray, np.ndarray]:
        """(probabilities float32 [n, C], classes int32 [n, 2] = {label, predicted}) of the logged bags: a host read."""
        n = min(int(self.ctr[0]), self.capacity)
        return self.log_prob[:n].cpu().numpy(), self.log_cls[:n].cpu().numpy()


def format_valid(epoch: int, m: Dict[str, object], keys: Sequence[str] = ("loss", "loss_last", "loss_ct", "loss_pth",
                                                                        "loss_cossim", "acc", "auc_hard", "recall", "precision",
                                                                        "auc", "best_thres")) -> str:
    return f"Valid Epoch: [{epoch}]\t" + "\t".join(f"{k} {m[k]:.6g}" for k in keys if k in m)
