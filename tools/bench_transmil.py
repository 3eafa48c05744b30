"""TransMIL image-only extractor (--model_pathology TransMIL): one bag of N patches, eval forward and forward + backward (BCE
through the aggregator_clip head), HIP path against the torch restatement (tests/transmil_ref.py, fp32) on the same GPU in the
same process.  Median of --reps timed regions; GF per step from the shapes (transmil_flops below); fraction of the 157.3 TF
fp32 MFMA peak.  Prints one JSON line per N."""
import argparse, json, os, sys
from types import SimpleNamespace
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import mil_amd  # noqa: E402,F401
from mil_amd import synthetic as syn  # noqa: E402
from mil_amd.model.utils_clip import get_model  # noqa: E402
from mil_amd.model.dim1.TransMIL import geometry  # noqa: E402
import transmil_ref as R  # noqa: E402

PEAK_TF = 157.3


def transmil_flops(N: int, L: int = 768) -> float:
    """Forward FLOPs of one bag (multiply-add = 2): _fc1, and per layer to_qkv, the Nystrom products (A1, A2, A3, A3 v, 6 x 4
    pseudo-inverse products, Z W, A1 U), the 33-tap conv, to_out; PPEG 49 taps.  Backward counted as twice the forward."""
    g = geometry(N)
    n, seq, m, d, D = g["n_pad"], g["seq"], 256, 64, 512
    per_head = 2 * (n * m * d + m * m * d + m * n * d + m * n * d + 24 * m ** 3 + m * m * d + n * m * d) + 2 * 33 * n * d
    layer = 2 * n * D * 3 * D + 8 * per_head + 2 * seq * D * D
    return 2 * N * L * D + 2 * layer + 2 * 49 * seq * D


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[2000, 7600, 15592])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_torch", action="store_true", help="skip the torch restatement")
    a = ap.parse_args()
    dev = torch.device("cuda")
    args = SimpleNamespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    torch.manual_seed(1234)
    model = get_model(args).to(dev).eval()        # eval: dropout off, gradients still flow
    p = {k.replace("extractor_pathology.", ""): v.detach() for k, v in model.state_dict().items()}
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    y = syn.make_labels(3, 1).to(dev)
    bce = torch.nn.BCELoss()
    for N in a.N:
        x = syn.make_bags(N, 1, N, 768)[0].to(dev)

        def fwd():
            with torch.no_grad():
                model([x], [N])

        def step():
            model.zero_grad(set_to_none=True)
            _, prob = model([x], [N])
            bce(prob, y).backward()

        def t_fwd():
            with torch.no_grad():
                R.transmil(x, p)

        def t_step():
            for v in pr.values():
                v.grad = None
            h, _ = R.transmil(x, pr)
            bce(torch.sigmoid(h @ pr["fc.1.weight"].t() + pr["fc.1.bias"]).unsqueeze(0), y).backward()

        gf = transmil_flops(N) / 1e9
        res = dict(N=N, n_pad=geometry(N)["n_pad"], gf_fwd=round(gf, 2), gf_step=round(3 * gf, 2),
                   fwd_ms=round(timed(fwd, a.reps, a.warmup), 3), step_ms=round(timed(step, a.reps, a.warmup), 3))
        res["step_frac_peak"] = round(3 * gf / (res["step_ms"] * 1e-3) / (PEAK_TF * 1e3), 4)
        if not a.no_torch:
            res["torch_fwd_ms"] = round(timed(t_fwd, a.reps, a.warmup), 3)
            res["torch_step_ms"] = round(timed(t_step, a.reps, a.warmup), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
