"""numpy float64 oracle of the evaluation metrics (mil_amd.metrics / csrc/metrics.hip), written from the definitions: what the
reference's valid() gets from sklearn on the argmax predictions (train_ddp.py:497-509) and its test_ddp.py from the scores
(:141-162, :286-309).  Nothing here looks at a confusion matrix or at the kernels' intermediate counts except `rank_counts` /
`reduce_ints`, which restate the integer definitions of the issue so that the device integers can be compared exactly."""
import math

import numpy as np

NAN = float("nan")


# ---- per-step criterion (train_ddp.py:95-98), float64 on the given fp32 probabilities
def bce(p, y):
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    with np.errstate(divide="ignore"):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
    return float(np.mean(-(y * lp + (1.0 - y) * l1p)))


def cross_entropy(p, y):
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    mx = p.max(1, keepdims=True)
    logsm = p - (mx + np.log(np.exp(p - mx).sum(1, keepdims=True)))
    return float(np.mean(-(y * logsm).sum(1)))


def criterion(p, y):
    return cross_entropy(p, y) if np.asarray(p).shape[1] > 2 else bce(p, y)


def argmax_first(a):
    """Row-wise argmax, the first maximal index winning (torch.argmax, np.argmax)."""
    return np.argmax(np.asarray(a), axis=1).astype(np.int64)


def step_losses(steps):
    """steps: [(probs_terms, y, extra)] -> (per-step [last, ct, pth, extra] float64, per-step B)."""
    rows, bs = [], []
    for terms, y, extra in steps:
        vals = [criterion(t, y) for t in terms] + [0.0] * (3 - len(terms))
        rows.append(vals + [0.0 if extra is None else float(extra)])
        bs.append(np.asarray(y).shape[0])
    return np.asarray(rows, np.float64).reshape(-1, 4), np.asarray(bs, np.int64)


def weighted_losses(steps):
    """AverageMeter: sum(loss_step * B_step) / sum(B_step) per term, and the total."""
    rows, bs = step_losses(steps)
    per = (rows * bs[:, None]).sum(0) / bs.sum()
    return {"loss_last": per[0], "loss_ct": per[1], "loss_pth": per[2], "loss_cossim": per[3],
            "loss": float((rows.sum(1) * bs).sum() / bs.sum())}


# ---- the argmax-prediction metrics
def _nanmean(v):
    v = [x for x in v if not math.isnan(x)]
    return sum(v) / len(v) if v else NAN


def _ratio(a, b, zero=NAN):
    return a / b if b else zero


def _binary_hard_auc(lab, prd):
    """roc_auc_score of a 0/1 label vector against a 0/1 prediction: (TPR + TNR) / 2; nan when a class is absent."""
    P, N = int((lab == 1).sum()), int((lab == 0).sum())
    if not P or not N:
        return NAN
    return (int(((lab == 1) & (prd == 1)).sum()) / P + int(((lab == 0) & (prd == 0)).sum()) / N) / 2.0


def hard_metrics(labels, preds, C):
    lab, prd = np.asarray(labels, np.int64), np.asarray(preds, np.int64)
    out = {"acc": float((lab == prd).mean())}
    if C <= 2:
        tp = int(((lab == 1) & (prd == 1)).sum())
        out["auc_hard"] = _binary_hard_auc(lab, prd)
        out["recall"] = _ratio(tp, int((lab == 1).sum()))
        out["precision"] = _ratio(tp, int((prd == 1).sum()))
        return out
    aucs = [_binary_hard_auc((lab == c).astype(np.int64), (prd == c).astype(np.int64)) for c in range(C)]
    out["auc_hard"] = NAN if any(math.isnan(a) for a in aucs) else sum(aucs) / C
    present = [c for c in range(C) if (lab == c).any() or (prd == c).any()]
    out["recall"] = _nanmean([_ratio(int(((lab == c) & (prd == c)).sum()), int((lab == c).sum())) for c in present])
    out["precision"] = _nanmean([_ratio(int(((lab == c) & (prd == c)).sum()), int((prd == c).sum())) for c in present])
    return out


# ---- the score metrics of a binary model
def rank_counts(scores, labels):
    s, pos = np.asarray(scores, np.float32), np.asarray(labels) == 1
    ge, eq = s[None, :] >= s[:, None], s[None, :] == s[:, None]          # [i, j]: s_j >= s_i
    return (ge & pos[None, :]).sum(1), (ge & ~pos[None, :]).sum(1), (eq & ~pos[None, :]).sum(1)


def reduce_ints(scores, labels):
    s, pos = np.asarray(scores, np.float32), np.asarray(labels) == 1
    gp, gn, en = (v.astype(object) for v in rank_counts(s, labels))       # Python ints: no overflow anywhere
    P, N = int(pos.sum()), int((~pos).sum())
    S2 = int(sum(2 * (N - gn[i]) + en[i] for i in range(len(s)) if pos[i]))
    best = None
    for i in range(len(s)):
        key = (int(gp[i]) * N - int(gn[i]) * P, float(s[i]), -i)
        if best is None or key > best:
            best, istar = key, i
    if best is None:
        return {"P": P, "N": N, "S2": S2, "jstar": 0, "ge_pos": 0, "ge_neg": 0, "sstar": 0.0}
    return {"P": P, "N": N, "S2": S2, "jstar": best[0], "ge_pos": int(gp[istar]), "ge_neg": int(gn[istar]),
            "sstar": float(s[istar])}


def auc_pairs(scores, labels):
    """P(score of a positive > score of a negative) + half the ties: roc_auc_score(labels, scores)."""
    s, lab = np.asarray(scores, np.float64), np.asarray(labels)
    sp, sn = s[lab == 1], s[lab != 1]
    if not len(sp) or not len(sn):
        return NAN
    gt = int((sp[:, None] > sn[None, :]).sum())
    eq = int((sp[:, None] == sn[None, :]).sum())
    return (gt + 0.5 * eq) / (len(sp) * len(sn))


def youden_threshold(scores, labels):
    """roc_curve + argmax(tpr - fpr): the thresholds are +inf and then the distinct scores in decreasing order, the first
    maximum wins; tpr - fpr is compared exactly (cross-multiplied integers)."""
    s, lab = np.asarray(scores, np.float32), np.asarray(labels)
    P, N = int((lab == 1).sum()), int((lab != 1).sum())
    best_t, best_j = math.inf, 0
    for t in sorted(set(float(v) for v in s), reverse=True):
        j = int(((s >= t) & (lab == 1)).sum()) * N - int(((s >= t) & (lab != 1)).sum()) * P
        if j > best_j:
            best_t, best_j = t, j
    return best_t


def at_threshold(scores, labels, thres):
    """recall / precision / accuracy of (score >= thres) as test_ddp.py:147-150 (sklearn's default zero_division: 0)."""
    s, lab = np.asarray(scores, np.float32), np.asarray(labels)
    hard = s >= np.float64(thres)
    tp, P, pp = int((hard & (lab == 1)).sum()), int((lab == 1).sum()), int(hard.sum())
    return {"recall_at": _ratio(tp, P, 0.0), "precision_at": _ratio(tp, pp, 0.0), "acc_at": float((hard == (lab == 1)).mean())}


def score_metrics(scores, labels, thres=None):
    best = youden_threshold(scores, labels)
    out = {"auc": auc_pairs(scores, labels), "best_thres": best}
    out.update(at_threshold(scores, labels, best if thres is None else thres))
    return out


def all_metrics(steps, thres=None):
    """The whole dict of EvalLog.finish for steps = [(probs_terms, y, extra)], probs_terms[0] the Last head."""
    probs = np.concatenate([np.asarray(t[0][0], np.float32) for t in steps], 0)
    y = np.concatenate([np.asarray(t[1], np.float32) for t in steps], 0)
    C = probs.shape[1]
    labels, preds = argmax_first(y), argmax_first(probs)
    out = weighted_losses(steps)
    out.update(hard_metrics(labels, preds, C))
    if C == 2:
        out.update(score_metrics(probs[:, 1], labels, thres))
    return out


def close(a, b, tol=1e-12):
    """Equal within tol relative (absolute below 1), nan == nan, inf == inf."""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol * max(1.0, abs(a), abs(b))


def rel_close(a, b, tol=1e-12):
    """Equal within tol RELATIVE, whatever the magnitude; 0 only equals 0.  For the loss values."""
    a, b = float(a), float(b)
    return a == b or abs(a - b) <= tol * max(abs(a), abs(b))
