"""Fusion model with the TransMIL aggregator (--aggregator TransMIL --fusion_transmil 1): the train-mode eager step of the
authors' shape - modality ['CT', 'pathology'], 160 CT tokens, one note, one bag of N patches, BCE x 3 (loss_point CT-Pth-Last),
backward, FlatAdam - next to the same model with the ABMIL aggregator in the same process.  Median of --reps timed regions
with their spread.  Prints one JSON line per N.

--index: per N, the HOST time per step of the two ways to the sequence index of the multi-modal bag: the Python list of
1 + s^2 ints uploaded (what the image-only eager path does) and the [B, 9] table + one launch of ops.tm_seq_index_segs;
wall-clock of the host thread, the device idle at the start of every region, plus the device time of the launch.

--graph: per N, the same eager TransMIL-aggregator step next to the step replayed from its hipGraph
(fusion_step.RaggedFusionTransMILStepper, counted FlatAdam inside the graph; --fusion_transmil_graph 1), one region = one
step, and the bytes the graph keeps resident in the stepper's memory pool.

--graph_eval: per N, the replayed EVALUATION forward (RaggedFusionTransMILStepper, backward=False; test_ddp.py
--fusion_transmil_graph 1) with the note-attention export off and with model.note_attn = "all" (the export's launches inside the
graph, the per-bag slicing behind the replay); one region = --inner forwards, reported per forward."""
import argparse, json, os, sys, time
from types import SimpleNamespace
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import mil_amd  # noqa: E402,F401
from mil_amd import ops, synthetic as syn  # noqa: E402
from mil_amd.model.utils import get_model  # noqa: E402
from mil_amd.model.dim1.TransMIL import segment_table, seq_index_segments  # noqa: E402
from mil_amd.optim import FlatAdam  # noqa: E402

D_CT, P = 160, 1
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731


def region_times(fn, reps, warm):
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
    return ts


def make_args(aggregator, clip_layers):
    return SimpleNamespace(modality=["CT", "pathology"], model_pathology=aggregator, model_CI="CLIP", aggregator=aggregator,
                           num_classes=2, learnablePrompt=0, alignment_base="CI", model_CT="resnetMC3_18",
                           fusion_transmil=int(aggregator == "TransMIL"), clip_layers=clip_layers)


def step_rows(a, dev):
    y = syn.make_labels(3, 1).to(dev)
    ids = syn.make_token_ids(4, 1, P).to(dev)
    ct = torch.randn((1, D_CT, 512), generator=torch.Generator().manual_seed(5)).to(dev)
    for N in a.N:
        x = syn.make_bags(N, 1, N, 768).to(dev)
        res = dict(N=N, rows=N + 2 * P + D_CT)
        for agg in ("TransMIL", "ABMIL"):
            torch.manual_seed(1234)
            model = get_model(make_args(agg, a.clip_layers)).to(dev).train()
            opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=1e-5)
            with torch.no_grad():
                t = model.clinic_extractor(ids)              # the frozen tower: outside the region, as with --cache_text 1

            def step():
                opt.zero_grad()
                model([ct, x], None, text_features=t, labels=y, loss_scale=3.0 / 2)
                ops.backward(model.last_loss)
                opt.step()

            ts = region_times(step, a.reps, a.warmup)
            res.update({agg + "_ms": round(med(ts), 3), agg + "_min_ms": round(min(ts), 3), agg + "_max_ms": round(max(ts), 3)})
            del model, opt
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def graph_rows(a, dev):
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    y = syn.make_labels(3, 1).to(dev)
    ids = syn.make_token_ids(4, 1, P).to(dev)
    ct = torch.randn((1, D_CT, 512), generator=torch.Generator().manual_seed(5)).to(dev)
    for N in a.N:
        x = syn.make_bags(N, 1, N, 768).to(dev)
        res = dict(N=N, rows=N + 2 * P + D_CT)
        for tag in ("eager", "replayed"):
            torch.manual_seed(1234)
            model = get_model(make_args("TransMIL", a.clip_layers)).to(dev).train()
            opt = FlatAdam([p for p in model.parameters() if p.requires_grad], lr=1e-5, counted=(tag == "replayed"))
            with torch.no_grad():
                t = model.clinic_extractor(ids)              # the frozen tower: outside the region, as with --cache_text 1
            if tag == "eager":
                def step():
                    opt.zero_grad()
                    model([ct, x], None, text_features=t, labels=y, loss_scale=3.0 / 2)
                    ops.backward(model.last_loss)
                    opt.step()
            else:
                st = RaggedFusionTransMILStepper(model, opt, B=1, P=P, ct_shape=(D_CT, 512), loss_mult=3.0, drop_seed=1234)
                slot = st.slot(N)
                slot.x[:N].copy_(x[0])
                slot.ct.copy_(ct)
                slot.text.copy_(t)
                slot.y.copy_(y)

                def step():
                    st.step(slot, [N])
            ts = region_times(step, a.reps, max(a.warmup, 3))   # eager visit, capture, first replay: before the regions
            res.update({tag + "_ms": round(med(ts), 3), tag + "_min_ms": round(min(ts), 3), tag + "_max_ms": round(max(ts), 3)})
            if tag == "replayed":
                assert st.n_graphs == 1 and st.replays >= a.reps, (st.n_graphs, st.replays)
                assert int(st.flag.item()) == 0              # no length on the device left its key
                res.update(cap=slot.cap, side=st.sides([N])[0], graph_MiB=round(st.pool_bytes() / 2 ** 20, 1))
                del st, slot
            del model, opt
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def graph_eval_rows(a, dev):
    from mil_amd.fusion_step import RaggedFusionTransMILStepper
    ct = torch.randn((1, D_CT, 512), generator=torch.Generator().manual_seed(5)).to(dev)
    t = torch.randn((1, P, 512), generator=torch.Generator().manual_seed(6)).to(dev)
    for N in a.N:
        x = syn.make_bags(N, 1, N, 768).to(dev)
        res = dict(N=N, rows=N + 2 * P + D_CT, inner=a.inner)
        for tag, scope in (("off", False), ("all", "all")):
            torch.manual_seed(1234)
            model = get_model(make_args("TransMIL", a.clip_layers)).to(dev).eval()
            model.note_attn = scope
            st = RaggedFusionTransMILStepper(model, None, B=1, P=P, ct_shape=(D_CT, 512), backward=False)
            slot = st.slot(N)
            slot.x[:N].copy_(x[0])
            slot.ct.copy_(ct)
            slot.text.copy_(t)

            def region():
                for _ in range(a.inner):
                    st.step(slot, [N])
            st.step(slot, [N])                               # eager visit; the capture and the first replays are the warm-up
            ts = [v / a.inner for v in region_times(region, a.reps, max(a.warmup, 2))]
            assert st.n_graphs == 1 and st.replays >= a.reps * a.inner and int(st.flag.item()) == 0
            assert (model.last_bag_attn is not None) == (scope == "all")
            res.update({tag + "_ms": round(med(ts), 4), tag + "_min_ms": round(min(ts), 4), tag + "_max_ms": round(max(ts), 4)})
            del st, slot, model
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


def index_rows(a, dev):
    for N in a.N:
        R = N + 2 * P + D_CT
        segs = [[(N, P), (N + P, D_CT), (N + P + D_CT, P), (0, N)]]

        def host_list():
            return torch.tensor(seq_index_segments(segs), dtype=torch.int32).to(dev, non_blocking=True)

        def device_table():
            rows, total = segment_table(segs)
            return ops.tm_seq_index_segs(torch.tensor(rows, dtype=torch.int32).to(dev, non_blocking=True), total, R)

        assert torch.equal(host_list(), device_table())
        res = dict(N=N, entries=int(host_list().numel()))
        for tag, fn in (("host_list", host_list), ("device_table", device_table)):
            ts = []
            for i in range(a.warmup + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    ts.append(1e3 * (t1 - t0))
            res.update({tag + "_host_ms": round(med(ts), 4), tag + "_host_min_ms": round(min(ts), 4),
                        tag + "_host_max_ms": round(max(ts), 4)})
        rows, total = segment_table(segs)
        tab = torch.tensor(rows, dtype=torch.int32).to(dev)
        out = torch.empty(total, dtype=torch.int32, device=dev)
        res["launch_device_ms"] = round(med(region_times(lambda: ops.tm_seq_index_segs(tab, total, R, idx_out=out), a.reps, a.warmup)), 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[2000, 7600, 15592])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clip_layers", type=int, default=1, help="the frozen text tower runs outside the timed region")
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--graph", action="store_true", help="the eager step next to the step replayed from its hipGraph")
    ap.add_argument("--graph_eval", action="store_true", help="the replayed evaluation forward, note-attention export off / all")
    ap.add_argument("--inner", type=int, default=20, help="--graph_eval: forwards per timed region")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    (graph_eval_rows if a.graph_eval else graph_rows if a.graph else index_rows if a.index else step_rows)(a, dev)


if __name__ == "__main__":
    main()
