"""GPU: the evaluation log's kernels (csrc/metrics.hip) and metrics.EvalLog against the float64 oracle tests/metrics_ref.py.
Integers are compared exactly.  The losses are held to 1e-12 RELATIVE whatever their size (ref.rel_close; 0 only equals 0):
both sides are double on the same fp32 probabilities and differ by the device's log / exp and the order of a sum of at most 64
terms.  The final ratios (values in [0, 1], formed by one or two float64 divisions of the same integers) are held to 1e-12 with
ref.close, which also treats nan and inf."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_ref as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "llm-guided-multimodal-mil_amd")
TOL = 1e-12


def _same(k, got, want):
    """A reported value against the oracle's: losses relative, the threshold equal, the ratios within TOL."""
    if k == "best_thres":
        return got == want
    return ref.rel_close(got, want, TOL) if k.startswith("loss") else ref.close(got, want, TOL)
T = 64                      # MIL_EVAL_TILE: the rank kernel's tile edge (asserted against the binding below)
DEV = "cuda:0"


def _log(capacity, C, nterm=1):
    from mil_amd.metrics import EvalLog
    return EvalLog(capacity, C, nterm, DEV)


def _onehot(cls, C):
    return torch.eye(C, dtype=torch.float32)[torch.as_tensor(cls)]


def _steps(B, C, nterm, with_extra, seed):
    """Two steps: the first holds a probability of exactly 0 and one of exactly 1 (the -100 clamp on either log), the second an
    argmax tie (the first maximal index wins)."""
    g = torch.Generator().manual_seed(seed)
    steps = []
    for k in range(2):
        terms = [torch.rand((B, C), generator=g) for _ in range(nterm)]
        if k == 0:
            for t in terms:
                t[0, 0], t[0, C - 1] = 0.0, 1.0
        else:
            terms[0][B - 1, :] = 0.25
            terms[0][B - 1, 1:3] = 0.75             # columns 1 and 2 tie (C = 2: column 1 alone, columns 0 / 1 differ)
            if C == 2:
                terms[0][B - 1, :] = 0.5            # columns 0 and 1 tie
        cls = torch.randint(0, C, (B,), generator=g)
        if k == 0:
            cls[0] = 0                              # label 1 on the probability 0, label 0 on the probability 1: both clamps show
        y = _onehot(cls, C)
        extra = torch.rand((1,), generator=g) if with_extra else None
        steps.append((terms, y, extra))
    return steps


@pytest.mark.parametrize("with_extra", [False, True], ids=["plain", "extra"])
@pytest.mark.parametrize("nterm", [1, 3])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_push_logs_scores_classes_and_losses(B, C, nterm, with_extra):
    steps = _steps(B, C, nterm, with_extra, 100 * B + 10 * C + nterm)
    log = _log(2 * B, C, nterm)
    for terms, y, extra in steps:
        log.push([t.to(DEV) for t in terms], y.to(DEV), None if extra is None else extra.to(DEV))
    probs, cls = log.read()
    want_p = torch.cat([s[0][0] for s in steps]).numpy()
    want_y = torch.cat([s[1] for s in steps]).numpy()
    assert probs.tobytes() == want_p.tobytes()                                      # bit for bit
    assert np.array_equal(cls[:, 0], ref.argmax_first(want_y)) and np.array_equal(cls[:, 1], ref.argmax_first(want_p))
    assert cls[2 * B - 1, 1] == (0 if C == 2 else 1)                                # the tie went to the first maximal index
    np_steps = [([t.numpy() for t in terms], y.numpy(), None if e is None else float(e)) for terms, y, e in steps]
    want_rows, want_b = ref.step_losses(np_steps)
    got_rows = log.step_loss[:2].cpu().numpy()
    print("step losses", got_rows.tolist(), want_rows.tolist())
    assert np.array_equal(log.step_b[:2].cpu().numpy(), want_b)
    if C == 2:
        assert float(want_rows[0, 0]) >= 200.0 / (B * C)                            # both clamps were hit
    for a, b in zip(got_rows.ravel(), want_rows.ravel()):
        assert ref.rel_close(a, b, TOL), (a, b)
    m, want = log.finish(), ref.all_metrics(np_steps)
    assert m["counts"]["n"] == 2 * B and m["counts"]["steps"] == 2
    for k, v in want.items():
        assert _same(k, m[k], v), (k, m[k], v)


def test_overflow_and_nan_raise_at_finish():
    log = _log(4, 2)
    p, y = torch.rand((3, 2)).to(DEV), _onehot([0, 1, 1], 2).to(DEV)
    log.push(p, y)
    log.push(p, y)                                                                  # rows 3..5 of 4: dropped
    with pytest.raises(RuntimeError, match="capacity"):
        log.finish()
    probs, _ = log.read()
    assert probs.shape[0] == 3                                                      # the dropped push wrote nothing
    log.reset()
    log.push(p, y)
    assert log.finish()["counts"]["n"] == 3                                         # reset clears the flag too
    log.reset()
    p[1, 0] = float("nan")
    log.push(p, y)
    with pytest.raises(RuntimeError, match="NaN"):
        log.finish()


def _fill(log, scores, labels):
    """A log of n samples written directly (the pushes are covered above): scores as prob[:, 1]."""
    n = len(scores)
    s = torch.as_tensor(np.asarray(scores, np.float32))
    log.reset()
    log.log_prob[:n, 1] = s.to(DEV)
    log.log_prob[:n, 0] = (1.0 - s).to(DEV)
    log.log_cls[:n, 0] = torch.as_tensor(np.asarray(labels, np.int32)).to(DEV)
    log.log_cls[:n, 1] = (s > 0.5).to(torch.int32).to(DEV)
    log.ctr[0] = n


def _rank_case(n, kind, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 2, n)
    if kind == "pos":
        lab[:] = 1
    elif kind == "neg":
        lab[:] = 0
    if kind == "distinct":
        s = (rng.permutation(n).astype(np.float32) + 0.5) / n                       # no two equal
    else:
        s = rng.integers(0, 4, n).astype(np.float32) / 4.0 + 0.125                  # four levels: heavy ties
    return s.astype(np.float32), lab


@pytest.mark.parametrize("kind", ["levels4", "distinct", "pos", "neg"])
@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1, 1000])
def test_rank_and_reduce_integers_are_exact(n, kind):
    from mil_amd.ops import metrics as om
    assert om.EVAL_TILE == T
    s, lab = _rank_case(n, kind, 7 * n + len(kind))
    log = _log(max(n, 3) + 5, 2)                                                     # capacity beyond n: the grid's idle tail
    _fill(log, s, lab)
    for thres in (None, 0.375, 0.3):
        m = log.finish(thres)
        c = m["counts"]
        gp, gn, en = ref.rank_counts(s, lab)
        got = log.rank[:n].cpu().numpy()
        assert np.array_equal(got[:, 0], gp) and np.array_equal(got[:, 1], gn) and np.array_equal(got[:, 2], en)
        ints = ref.reduce_ints(s, lab)
        for k, v in ints.items():
            assert c[k] == v, (k, c[k], v)
        hard = s >= np.float64(np.inf if thres is None else thres)
        assert c["tp_at"] == int((hard & (lab == 1)).sum()) and c["fp_at"] == int((hard & (lab == 0)).sum())
        conf = np.zeros((2, 2), np.int64)
        np.add.at(conf, (lab, (s > 0.5).astype(np.int64)), 1)
        assert np.array_equal(c["conf"], conf) and c["n"] == n
        want = ref.score_metrics(s, lab, thres)
        want.update(ref.hard_metrics(lab, (s > 0.5).astype(np.int64), 2))
        assert m["best_thres"] == want.pop("best_thres")
        for k, v in want.items():
            assert ref.close(m[k], v, TOL), (k, thres, m[k], v)


def test_push_replays_from_a_captured_graph():
    """One push captured on one stream (no parallel branches); replayed three times with the static inputs changed in between,
    the log holds three steps with the three inputs: the row index is read on the device."""
    B, C = 3, 2
    g = torch.Generator().manual_seed(5)
    inputs = [(torch.rand((B, C), generator=g), _onehot(torch.randint(0, C, (B,), generator=g), C)) for _ in range(3)]
    log = _log(3 * B, C)
    sp, sy = inputs[0][0].to(DEV), inputs[0][1].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        log.push(sp, sy)                                                            # warm-up outside the capture
        log.reset()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        log.push(sp, sy)
    for p, y in inputs:
        sp.copy_(p)
        sy.copy_(y)
        graph.replay()
    torch.cuda.synchronize()
    probs, cls = log.read()
    assert probs.tobytes() == torch.cat([p for p, _ in inputs]).numpy().tobytes()
    assert np.array_equal(cls[:, 0], ref.argmax_first(torch.cat([y for _, y in inputs]).numpy()))
    m = log.finish()
    assert m["counts"]["steps"] == 3 and m["counts"]["n"] == 3 * B
    want = ref.weighted_losses([([p.numpy()], y.numpy(), None) for p, y in inputs])
    assert ref.rel_close(m["loss"], want["loss"], TOL), (m["loss"], want["loss"])


@pytest.mark.parametrize("model_pathology", ["ABMIL", "TransMIL"])
def test_eval_log_behind_twelve_eval_forwards(model_pathology):
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    F = 512
    args = create_arg_parser(["--variant", "image_only", "--model_pathology", model_pathology, "--synthetic", f"[130, {F}, 12]"])
    torch.manual_seed(11)
    model = train_ddp.build_model(args).to(DEV).eval()
    g = torch.Generator().manual_seed(12)
    log = _log(12, 2)
    outs, ys = [], []
    with torch.no_grad():
        for i in range(12):
            n = (7, 50, 130)[i % 3]
            x = torch.randn((1, n, F), generator=g).to(DEV)
            y = _onehot([int(torch.randint(0, 2, (1,), generator=g))], 2).to(DEV)
            _, out = model([x])
            log.push(out, y)
            outs.append(out)
            ys.append(y)
    m = log.finish()
    steps = [([o.cpu().numpy()], y.cpu().numpy(), None) for o, y in zip(outs, ys)]      # read back afterwards
    probs = np.concatenate([s[0][0] for s in steps])
    labels = ref.argmax_first(np.concatenate([s[1] for s in steps]))
    c = m["counts"]
    for k, v in ref.reduce_ints(probs[:, 1], labels).items():
        assert c[k] == v, (k, c[k], v)
    conf = np.zeros((2, 2), np.int64)
    np.add.at(conf, (labels, ref.argmax_first(probs)), 1)
    assert np.array_equal(c["conf"], conf) and c["n"] == 12 and c["steps"] == 12
    for k, v in ref.all_metrics(steps).items():
        assert _same(k, m[k], v), (k, m[k], v)


def _run(script, *argv):
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *argv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


TRAIN = ["--synthetic", "[64, 768, 12]", "--clip_layers", "1", "--batch_size", "2", "--n_epochs", "2", "--iter_per_epoch", "4"]


def test_train_ddp_validates_and_keeps_the_best_checkpoint(tmp_path):
    out = _run("train_ddp.py", *TRAIN, "--validate", "1", "--save_best", "--save_dir", str(tmp_path))
    lines = [ln for ln in out.splitlines() if ln.startswith("Valid Epoch:")]
    assert len(lines) == 2 and lines[0].startswith("Valid Epoch: [0]") and lines[1].startswith("Valid Epoch: [1]")
    assert all(k in lines[0] for k in ("loss ", "acc ", "auc_hard ", "recall ", "precision ", "auc ", "best_thres "))
    files = set(os.listdir(tmp_path))
    assert "checkpoint_last.pth.tar" in files and "checkpoint_best.pth.tar" in files
    last = torch.load(tmp_path / "checkpoint_last.pth.tar", weights_only=True)
    assert last["epoch"] == 2
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    args = create_arg_parser(TRAIN)
    args.patch_dim = 768
    model = train_ddp.build_model(args)
    best = torch.load(tmp_path / "checkpoint_best.pth.tar", weights_only=True)
    model.load_state_dict(best["state_dict"])                                       # strict
    numbered = sorted(f for f in files if f[11:15].isdigit())
    assert numbered and best["epoch"] == int(numbered[-1][11:15]) + 1               # best = the last epoch that was kept


ROUTES = {
    # the fused trainer owns the weights: the pass loads them into the module first; its dropout counter lives on the host
    "fused_step": ["--variant", "image_only", "--synthetic", "[128, 512, 8]", "--batch_size", "4", "--fused_step"],
    # the replayed TransMIL step: device-side dropout pass counter, the validation forward replayed per grid side
    "transmil_graph": ["--variant", "image_only", "--model_pathology", "TransMIL", "--transmil_graph", "1", "--synthetic",
                       "[300, 768, 6]", "--ragged", "--batch_size", "1"],
    # the bucketed fusion step: validation through the replayed forward, fed from a resident cohort
    "hip_graph": ["--synthetic", "[700, 768, 8]", "--ragged", "--clip_layers", "1", "--batch_size", "1", "--hip_graph", "1"],
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_validation_runs_behind_every_training_route(tmp_path, route):
    """Two epochs, so that training goes on after a validation pass (train mode restored, dropout counters untouched: the pass
    asserts it) and the second pass reuses the evaluator."""
    out = _run("train_ddp.py", *ROUTES[route], "--n_epochs", "2", "--iter_per_epoch", "3", "--validate", "1", "--save_dir",
               str(tmp_path))
    lines = [ln for ln in out.splitlines() if ln.startswith("Valid Epoch:")]
    assert len(lines) == 2 and "auc_hard " in lines[1]
    assert {"checkpoint_0000.pth.tar", "checkpoint_0001.pth.tar", "checkpoint_best.pth.tar",
            "checkpoint_last.pth.tar"} == set(os.listdir(tmp_path))                  # --save_best off: every epoch, plus last


@pytest.mark.parametrize("route", ["hip_graph", "transmil_graph"])
def test_a_kept_evaluator_sees_the_weights_of_the_day(route):
    """train_ddp.py builds its evaluator once - captured inference graphs, resident cohort - and runs it every epoch while the
    optimizer updates the parameters in place.  Here: a pass, an in-place change of every trainable parameter, a second pass of
    the SAME evaluator, and a pass of a fresh one.  The second pass must follow the weights (it moves by more than 1e-4) and
    agree with the fresh evaluator within 1e-6: fp32 probabilities out of the same kernels, apart at most by the order of a
    few float atomics of the forward (some ulp of 6e-8)."""
    from mil_amd import train_ddp
    from mil_amd.config import create_arg_parser
    from mil_amd.dataset import load_cohort
    from mil_amd.evaluate import BagEvaluator
    args = create_arg_parser(ROUTES[route])
    data, args.patch_dim = load_cohort(args, "valid", 1)
    torch.manual_seed(5)
    model = train_ddp.build_model(args).to(DEV).eval()

    def one_pass(ev):
        log = _log(len(data), 2, ev.nterm)
        ev.run(log, timed=False, read=False)
        log.finish()                                                                # raises on overflow / NaN
        return log.read()[0]

    kept = BagEvaluator(args, model, data, torch.device(DEV), 1)
    p1 = one_pass(kept)
    g = torch.Generator(device=DEV).manual_seed(6)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.mul_(1.0 + 0.2 * torch.randn(p.shape, generator=g, device=DEV))
    p2 = one_pass(kept)
    p3 = one_pass(BagEvaluator(args, model, data, torch.device(DEV), 1))
    print("moved by", float(np.abs(p2 - p1).max()), "kept vs fresh", float(np.abs(p2 - p3).max()))
    assert float(np.abs(p2 - p1).max()) > 1e-4
    assert float(np.abs(p2 - p3).max()) <= 1e-6


def test_train_ddp_without_validate_writes_the_same_files_as_before(tmp_path):
    out = _run("train_ddp.py", *TRAIN, "--save_dir", str(tmp_path))
    assert "Valid Epoch" not in out
    assert set(os.listdir(tmp_path)) == {"checkpoint_0000.pth.tar", "checkpoint_0001.pth.tar", "checkpoint_best.pth.tar"}


@pytest.mark.parametrize("route", [[], ["--hip_graph", "1"]], ids=["eager", "resident_replay"])
def test_evaluate_reports_metrics_and_returns_test_ddps_preds(capsys, route):
    """evaluate.py --report_metrics 1 --mode valid against test_ddp.py, which this change leaves as it was."""
    from mil_amd import evaluate, test_ddp
    from mil_amd.config import create_arg_parser
    from mil_amd.evaluate import parse_args
    argv = ["--synthetic", "[64, 768, 12]", "--clip_layers", "1", "--ragged", *route]
    torch.manual_seed(3)
    plain = test_ddp.test(create_arg_parser(argv))
    assert "Result :" not in capsys.readouterr().out
    torch.manual_seed(3)
    rep = evaluate.evaluate(parse_args([*argv, "--report_metrics", "1", "--mode", "valid"]))
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("Result : Loss")]
    assert len(line) == 1 and all(k in line[0] for k in ("AUC", "Accuracy", "Precision", "Recall", "| Threshold"))
    assert np.asarray(plain[0], np.float64).tobytes() == np.asarray(rep[0], np.float64).tobytes()   # bit for bit
    assert list(plain[1]) == list(rep[1])


def test_evaluate_entry_point_prints_the_result_line_and_test_ddp_refuses_its_flags():
    argv = ["--synthetic", "[64, 768, 12]", "--clip_layers", "1", "--ragged", "--report_metrics", "1", "--mode", "valid"]
    out = _run("evaluate.py", *argv)
    line = [ln for ln in out.splitlines() if ln.startswith("Result : Loss")]
    assert len(line) == 1 and "| Threshold" in line[0] and "Time for inference" in out
    for flags, why in ((["--report_metrics", "1"], "unrecognized arguments: --report_metrics 1"),
                       (["--mode", "valid"], "--mode")):         # argparse reads --mode as an ambiguous prefix of --model_*
        r = subprocess.run([sys.executable, os.path.join(PKG, "test_ddp.py"), *argv[:5], *flags], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 2 and why in r.stderr, r.stderr[-300:]               # refused by the parser, not silently ignored
