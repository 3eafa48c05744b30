"""TransMIL image-only extractor (--model_pathology TransMIL): one bag of N patches, eval forward and forward + backward (BCE
through the aggregator_clip head), HIP path against the torch restatement (tests/transmil_ref.py, fp32) on the same GPU in the
same process.  Median of --reps timed regions; GF per step from the shapes (transmil_flops below); fraction of the 157.3 TF
fp32 MFMA peak.  Prints one JSON line per N.

--graph: per N, the TRAINING step (model.train(), BCE, backward, counted FlatAdam) eager - the module called with host
lengths, as train_ddp.py's autograd path runs it - next to the same step replayed from the side's hipGraph
(transmil_step.RaggedTransMILStepper): same bag, same region count, same process; the spread of the eager regions and the
memory of the graph's pool are reported with it.
--ragged K: K bags drawn from U[2000, 15592] in turn through the stepper: ms/step, replay / eager counts, eager steps after a
key's second visit (must be 0), graphs, the memory of their shared pool and the free memory the whole run took.
--attn cls: per N, the eval forward without attention and with the per-patch cls attention (need_attn="cls"), and the peak
allocated bytes of both, in one process; then the same forward with the attention on the fused passes (fused_cls, the route of
MIL_TM_FUSED_CLS=1), and a train-mode forward + backward of the extractor with the attention on either route (ms and peak).
--fused-a3: per N, the eager TRAINING step (model.train(), BCE, backward, counted FlatAdam) with the landmark-query pass
materialised (MIL_TM_FUSED_A3=0: the A3 map, its softmax and their products), fused (=1: csrc/landmark_attn.hip), and
materialised again - same model, same bag, same process, the switch read per call; median (min - max) of --reps regions each
and the peak allocated bytes of one step per route.
--fused-a1: the same three columns for the token-query pass (MIL_TM_FUSED_A1=0: the A1 map, its softmax and their products;
=1: csrc/token_attn.hip).  MIL_TM_FUSED_A3 is left as the environment has it and reported: run it once with 0 and once with 1.
--deterministic: per N, the eager TRAINING step with the fixed-order sums off and on (TransMIL.deterministic, the switch of
MIL_TM_DETERMINISTIC / --deterministic 1) in ALTERNATING regions - off, on, off, on .. - of one process, same model, same bag;
median (min - max) of --reps regions each; a region is one untimed step behind the flip and one timed step.  With --graph the replayed step as well: the stepper keeps one graph per setting
(the flag is part of its key) and the regions alternate between the two.
--pieces 3: the default rows (eval forward, forward + backward) with the Nystrom core's K >= 256 products on three-piece
split-bf16 MFMA (TransMIL.gemm_pieces, the switch of MIL_TM_PIECES / --tm_gemm_pieces); --pieces 0 pins the fp32 products.  The
rows carry the value and the min - max of the regions next to the median: run 0 and 3 one after the other on one machine.
--bags B (B > 1): per N, the TRAINING step over B bags of N patches each - eager (the module called with host lengths) and
replayed (RaggedTransMILStepper, B bags per slot) - with the landmark-side chain bag by bag (TransMIL.batch_bags = False: the
route of MIL_TM_BATCH_BAGS=0), batched over the bags (= True: ops.nystrom_core_bags), and bag by bag again, in one process, same
model, same bags; median (min - max) of --reps regions each and the peak allocated bytes of one eager step per route.  The
first and third columns are the yardstick.  B = 1 (the default) leaves every other row as it is.  --packed adds the column of
TransMIL.packed (ops.nystrom_core_packed: every token-side stage one launch set over all bags' rows) and, behind it, the column
of TransMIL.packed + TransMIL.packed_ppeg (ops.tm_ppeg_packed: PPEG too one launch set), read against the packed column
(`*_packed_ppeg_over_packed`); --mix makes the bags ragged.
--packed-cls: the eval forward WITH the per-patch cls attention (patch_attn; need_attn="cls") for 2, 4 and 8 ragged bags of up to
N patches, eager and replayed - the best route without the packed cls attention (bag by bag with MIL_TM_FUSED_CLS=1: no A1 / A3
map) next to packed + packed_cls and packed + packed_ppeg + packed_cls, the routes alternating region by region."""
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


def graph_rows(a, dev, args):
    from mil_amd import ops
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    bce = torch.nn.BCELoss()
    y = syn.make_labels(3, 1).to(dev)
    for N in a.N:
        torch.manual_seed(1234)
        m_e = get_model(args).to(dev).train()
        torch.manual_seed(1234)
        m_r = get_model(args).to(dev).train()
        o_e = FlatAdam(list(m_e.parameters()), lr=1e-5, counted=True)
        o_r = FlatAdam(list(m_r.parameters()), lr=1e-5, counted=True)
        st = RaggedTransMILStepper(m_r, o_r, B=1, drop_seed=1)
        x = syn.make_bags(N, 1, N, 768)[0].to(dev)
        slot = st.slot([N])
        slot.x[:N].copy_(x)
        slot.y.copy_(y)

        def eager():
            o_e.zero_grad()
            _, prob = m_e([x], [N])
            ops.backward(bce(prob, y))
            o_e.step()

        def replay():
            st.step(slot, [N])

        for _ in range(3):                        # eager visit, capture, first replay
            replay()
        assert st.n_graphs == 1
        ts = region_times(eager, a.reps, a.warmup)
        tr = region_times(replay, a.reps, a.warmup)
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        print(json.dumps(dict(N=N, side=slot.sides[0], eager_ms=round(med(ts), 3), eager_min_ms=round(min(ts), 3),
                              eager_max_ms=round(max(ts), 3), replay_ms=round(med(tr), 3), replay_min_ms=round(min(tr), 3),
                              replay_max_ms=round(max(tr), 3), graph_mib=round(list(st.graph_bytes.values())[0] / 2 ** 20, 1),
                              replays=st.replays, eager_steps=st.eager_steps)), flush=True)
        del st, slot, m_e, m_r, o_e, o_r
        torch.cuda.empty_cache()


def ragged_run(a, dev, args):
    import time
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    torch.manual_seed(1234)
    model = get_model(args).to(dev).train()
    opt = FlatAdam(list(model.parameters()), lr=1e-5, counted=True)
    st = RaggedTransMILStepper(model, opt, B=1, drop_seed=1, max_graphs=a.max_graphs or None)
    lens = [int(v) for v in torch.randint(2000, 15593, (a.ragged,), generator=torch.Generator().manual_seed(a.seed))]
    pool = torch.randn((15592, 768), generator=torch.Generator().manual_seed(2)).to(dev)
    y = syn.make_labels(3, 1).to(dev)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    visits, late_eager, t_replay, n_replay = {}, 0, 0.0, 0
    t0 = time.perf_counter()
    for n in lens:
        slot = st.slot([n])
        slot.x[:n].copy_(pool[:n], non_blocking=True)
        slot.y.copy_(y, non_blocking=True)
        v = visits[slot.sides] = visits.get(slot.sides, 0) + 1
        e0, g0 = st.eager_steps, st.n_graphs
        if v > 2:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        st.step(slot, [n])
        if v > 2:
            torch.cuda.synchronize()
            t_replay += time.perf_counter() - t1
            n_replay += 1
            late_eager += st.eager_steps - e0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    held = free0 - torch.cuda.mem_get_info(dev)[0]
    slots = sum(s.x.numel() * 4 for s in st.slots.values())
    print(json.dumps(dict(ragged=a.ragged, sides=len(visits), graphs=st.n_graphs, replays=st.replays, eager_steps=st.eager_steps,
                          eager_after_second_visit=late_eager, ms_per_step_all=round(1e3 * wall / a.ragged, 3),
                          ms_per_replayed_step=round(1e3 * t_replay / max(1, n_replay), 3), replayed_timed=n_replay,
                          held_gib=round(held / 2 ** 30, 3), slot_inputs_gib=round(slots / 2 ** 30, 3),
                          graph_pool_gib=round(st.pool_bytes() / 2 ** 30, 3),
                          largest_capture_mib=round(max(st.graph_bytes.values(), default=0) / 2 ** 20, 1))), flush=True)


def attn_rows(a, dev, args):
    """Per N, in one process: the eval forward (no grad) of the extractor without attention and with need_attn="cls", the
    median of --reps regions each with the spread of the plain one, and the peak allocated bytes of one forward of each."""
    torch.manual_seed(1234)
    net = get_model(args).to(dev).eval().extractor_pathology
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731

    def measure(res, fn, tag, times=True):
        """tag_ms / _min_ms / _max_ms of --reps regions of fn (times), tag_peak_mib of one more call."""
        if times:
            ts = region_times(fn, a.reps, a.warmup)
            res.update({tag + "_ms": round(med(ts), 3), tag + "_min_ms": round(min(ts), 3), tag + "_max_ms": round(max(ts), 3)})
        else:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            res[tag + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 3)
            del out

    for N in a.N:
        x = syn.make_bags(N, 1, N, 768)[0].to(dev)
        gw = torch.randn(512, generator=torch.Generator().manual_seed(3)).to(dev)

        def fwd(want, fused=None):
            net.fused_cls = fused
            return net(x, [N], need_attn=want)

        def train_step(fused):
            net.zero_grad(set_to_none=True)
            h, attn = fwd("cls", fused)
            (h[0] * gw).sum().backward()
            return attn

        run = {"fwd": lambda: fwd(False), "fwd_cls": lambda: fwd("cls", False), "fwd_again": lambda: fwd(False),
               "fwd_cls_fused": lambda: fwd("cls", True)}
        res = dict(N=N, n_pad=geometry(N)["n_pad"])
        net.eval()
        with torch.no_grad():
            for tag in ("fwd", "fwd_cls", "fwd_again", "fwd_cls_fused"):
                measure(res, run[tag], tag)
            for tag in ("fwd", "fwd_cls", "fwd_cls_fused"):
                measure(res, run[tag], tag, times=False)
        net.train()                                  # forward + backward of the extractor, the attention asked for
        for fused, tag in ((False, "train_cls"), (True, "train_cls_fused")):
            measure(res, lambda: train_step(fused), tag)
            measure(res, lambda: train_step(fused), tag, times=False)
        net.zero_grad(set_to_none=True)
        net.fused_cls = None
        res["cls_cost_pct"] = round(100.0 * (res["fwd_cls_ms"] - res["fwd_ms"]) / res["fwd_ms"], 2)
        res["cls_fused_cost_pct"] = round(100.0 * (res["fwd_cls_fused_ms"] - res["fwd_ms"]) / res["fwd_ms"], 2)
        res["full_map_mib_per_layer"] = round(8 * res["n_pad"] ** 2 * 4 / 2 ** 20, 1)
        print(json.dumps(res), flush=True)
        del x
        torch.cuda.empty_cache()


def fused_rows(a, dev, args, env="MIL_TM_FUSED_A3", name="a3"):
    """The three columns of --fused-a3 / --fused-a1: `env` is the switch that moves, `name` tags the map's size in the result."""
    from mil_amd import ops
    from mil_amd.optim import FlatAdam
    bce = torch.nn.BCELoss()
    y = syn.make_labels(3, 1).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    for N in a.N:
        torch.manual_seed(1234)
        model = get_model(args).to(dev).train()
        opt = FlatAdam(list(model.parameters()), lr=1e-5, counted=True)
        x = syn.make_bags(N, 1, N, 768)[0].to(dev)

        def step():
            opt.zero_grad()
            _, prob = model([x], [N])
            ops.backward(bce(prob, y))
            opt.step()

        res = dict(N=N, n_pad=geometry(N)["n_pad"], switch=env)
        if name == "a1":
            res["fused_a3"] = os.environ.get("MIL_TM_FUSED_A3", "0")
        before = os.environ.get(env)
        for switch, tag in (("0", "materialised"), ("1", "fused"), ("0", "materialised_again")):
            os.environ[env] = switch
            ts = region_times(step, a.reps, a.warmup)
            res.update({tag + "_ms": round(med(ts), 3), tag + "_min_ms": round(min(ts), 3), tag + "_max_ms": round(max(ts), 3)})
        for switch, tag in (("0", "materialised"), ("1", "fused")):
            os.environ[env] = switch
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            step()
            torch.cuda.synchronize()
            res[tag + "_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        os.environ.pop(env, None)
        if before is not None:
            os.environ[env] = before
        res[name + "_map_mib"] = round(8 * 256 * res["n_pad"] * 4 / 2 ** 20, 1)
        res["fused_over_materialised"] = round(res["fused_ms"] / min(res["materialised_ms"], res["materialised_again_ms"]), 4)
        print(json.dumps(res), flush=True)
        del model, opt, x
        torch.cuda.empty_cache()


def det_rows(a, dev, args):
    from mil_amd import ops
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    bce = torch.nn.BCELoss()
    y = syn.make_labels(3, 1).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731

    def alternate(fn, ext, res, tag):
        for on in (False, True, False, True):     # both settings warm (with a stepper: eager visit, capture) before any is timed
            ext.deterministic = on
            for _ in range(max(a.warmup, 2)):
                fn()
        ts = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):            # a region: one untimed step behind the flip (it runs on what the other
                ext.deterministic = on          # setting left in the caches; a training run never alternates), one timed
                ts[on] += region_times(fn, 1, 1)
        for on, name in ((False, "off"), (True, "on")):
            res.update({f"{tag}_{name}_ms": round(med(ts[on]), 3), f"{tag}_{name}_min_ms": round(min(ts[on]), 3),
                        f"{tag}_{name}_max_ms": round(max(ts[on]), 3)})
        res[f"{tag}_on_minus_off_us"] = round(1e3 * (med(ts[True]) - med(ts[False])), 1)

    for N in a.N:
        torch.manual_seed(1234)
        model = get_model(args).to(dev).train()
        opt = FlatAdam(list(model.parameters()), lr=1e-5, counted=True)
        x = syn.make_bags(N, 1, N, 768)[0].to(dev)

        def eager():
            opt.zero_grad()
            _, prob = model([x], [N])
            ops.backward(bce(prob, y))
            opt.step()

        res = dict(N=N, n_pad=geometry(N)["n_pad"], regions=a.reps)
        alternate(eager, model.extractor_pathology, res, "eager")
        if a.graph:
            torch.manual_seed(1234)
            m_r = get_model(args).to(dev).train()
            o_r = FlatAdam(list(m_r.parameters()), lr=1e-5, counted=True)
            st = RaggedTransMILStepper(m_r, o_r, B=1, drop_seed=1)
            slot = st.slot([N])
            slot.x[:N].copy_(x)
            slot.y.copy_(y)
            alternate(lambda: st.step(slot, [N]), m_r.extractor_pathology, res, "replay")
            assert st.n_graphs == 2, st.n_graphs
            res["graphs"] = st.n_graphs
            del st, slot, m_r, o_r
        print(json.dumps(res), flush=True)
        del model, opt, x
        torch.cuda.empty_cache()


def bags_rows(a, dev, args):
    from mil_amd import ops
    from mil_amd.optim import FlatAdam
    from mil_amd.transmil_step import RaggedTransMILStepper
    B = a.bags
    bce = torch.nn.BCELoss()
    y = syn.make_labels(3, B).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    for N in a.N:
        torch.manual_seed(1234)
        m_e = get_model(args).to(dev).train()
        torch.manual_seed(1234)
        m_r = get_model(args).to(dev).train()
        o_e = FlatAdam(list(m_e.parameters()), lr=1e-5, counted=True)
        o_r = FlatAdam(list(m_r.parameters()), lr=1e-5, counted=True)
        st = RaggedTransMILStepper(m_r, o_r, B=B, drop_seed=1)
        lengths = [max(1, N * (4 - b % 4) // 4) for b in range(B)] if a.mix else [N] * B       # --mix: N, 3N/4, N/2, N/4, N, ..
        x = torch.cat([syn.make_bags(N + b, 1, n, 768)[0] for b, n in enumerate(lengths)], 0).to(dev)
        slot = st.slot(lengths)
        slot.x[:sum(lengths)].copy_(x)
        slot.y.copy_(y)

        def eager():
            o_e.zero_grad()
            _, prob = m_e([x], lengths)
            ops.backward(bce(prob, y))
            o_e.step()

        def replay():
            st.step(slot, lengths)

        res = dict(N=N, bags=B, lengths=lengths, n_pad=geometry(N)["n_pad"], regions=a.reps,
                   fused_env=[os.environ.get(k, "0") for k in ("MIL_TM_FUSED_A1", "MIL_TM_FUSED_A3")])
        routes = (((False, False, False, "off"), (True, False, False, "on"))
                  + (((False, True, False, "packed"), (False, True, True, "packed_ppeg")) if a.packed else ())
                  + ((False, False, False, "off_again"),))
        for on, pk, pp, tag in routes:
            for m in (m_e, m_r):
                ex = m.extractor_pathology
                ex.batch_bags, ex.packed, ex.packed_ppeg = on, pk, pp
            for _ in range(3):                        # the stepper: eager visit, capture, first replay of this route's key
                replay()
            for name, fn in (("eager", eager), ("replay", replay)):
                ts = region_times(fn, a.reps, a.warmup)
                res.update({f"{name}_{tag}_ms": round(med(ts), 3), f"{name}_{tag}_min_ms": round(min(ts), 3),
                            f"{name}_{tag}_max_ms": round(max(ts), 3)})
        for on, pk, pp, tag in routes[:-1]:
            ex = m_e.extractor_pathology
            ex.batch_bags, ex.packed, ex.packed_ppeg = on, pk, pp
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            eager()
            torch.cuda.synchronize()
            res[f"eager_{tag}_peak_mib"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        assert st.n_graphs == len(routes) - 1, st.n_graphs          # one graph per route: the switches are part of the key
        for name in ("eager", "replay"):
            off = min(res[f"{name}_off_ms"], res[f"{name}_off_again_ms"])
            res[f"{name}_on_over_off"] = round(res[f"{name}_on_ms"] / off, 4)
            if a.packed:
                res[f"{name}_packed_over_off"] = round(res[f"{name}_packed_ms"] / off, 4)
                res[f"{name}_packed_over_on"] = round(res[f"{name}_packed_ms"] / res[f"{name}_on_ms"], 4)
                res[f"{name}_packed_ppeg_over_packed"] = round(res[f"{name}_packed_ppeg_ms"] / res[f"{name}_packed_ms"], 4)
        res["graph_mib"] = {("packed_ppeg" if "ppeg" in k else "packed" if "packed" in k else "on" if "batch_bags" in k else "off"): round(v / 2 ** 20, 1)
                            for k, v in st.graph_bytes.items()}
        print(json.dumps(res), flush=True)
        del st, slot, m_e, m_r, o_e, o_r, x
        torch.cuda.empty_cache()


def cls_packed_rows(a, dev, args):
    """Per bag count one JSON line: medians (and min / max) over a.reps regions of a.calls eval forwards each, in ms per forward.
    The routes take turns inside every repetition, so a drift of the machine lands on all of them alike."""
    from mil_amd.transmil_step import RaggedTransMILStepper
    routes = (("bag_fused_cls", dict(packed=False, packed_ppeg=False, packed_cls=False)),
              ("packed_cls", dict(packed=True, packed_ppeg=False, packed_cls=True)),
              ("packed_ppeg_cls", dict(packed=True, packed_ppeg=True, packed_cls=True)))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    for N in a.N:
        for B in (2, 4, 8):
            torch.manual_seed(1234)
            model = get_model(args).to(dev).eval()
            model.patch_attn = True
            ex = model.extractor_pathology
            ex.fused_cls = True                         # the bag-by-bag route at its best; the packed route is fused anyway
            st = RaggedTransMILStepper(model, None, B=B, backward=False)
            lengths = [max(1, N * (4 - b % 4) // 4) for b in range(B)]                  # N, 3N/4, N/2, N/4, N, ..
            x = torch.cat([syn.make_bags(N + b, 1, n, 768)[0] for b, n in enumerate(lengths)], 0).to(dev)
            slot = st.slot(lengths)
            slot.x[:sum(lengths)].copy_(x)

            def eager():
                with torch.no_grad():
                    for _ in range(a.calls):
                        ex(x, lengths, need_attn="cls")

            def replay():
                for _ in range(a.calls):
                    st.step(slot, lengths)

            def route(kw):
                for k, v in kw.items():
                    setattr(ex, k, v)

            for _, kw in routes:                        # every route: eager visit, capture, first replays; and a warm eager pass
                route(kw)
                for _ in range(3):
                    st.step(slot, lengths)
                eager()
            ts = {(name, tag): [] for name in ("eager", "replay") for tag, _ in routes}
            for _ in range(a.reps):
                for name, fn in (("eager", eager), ("replay", replay)):
                    for tag, kw in routes:
                        route(kw)
                        ts[name, tag] += [t / a.calls for t in region_times(fn, 1, 0)]
            res = dict(N=N, bags=B, lengths=lengths, regions=a.reps, calls_per_region=a.calls)
            for (name, tag), v in ts.items():
                res.update({f"{name}_{tag}_ms": round(med(v), 3), f"{name}_{tag}_min_ms": round(min(v), 3),
                            f"{name}_{tag}_max_ms": round(max(v), 3)})
            for name in ("eager", "replay"):
                for tag, _ in routes[1:]:
                    res[f"{name}_{tag}_over_bag_fused_cls"] = round(res[f"{name}_{tag}_ms"] / res[f"{name}_bag_fused_cls_ms"], 4)
            assert st.n_graphs == len(routes), st.n_graphs                  # one graph per route: the switches are part of the key
            print(json.dumps(res), flush=True)
            del st, slot, model, x
            torch.cuda.empty_cache()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[2000, 7600, 15592])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_torch", action="store_true", help="skip the torch restatement")
    ap.add_argument("--graph", action="store_true", help="training step per N: eager next to the replayed hipGraph")
    ap.add_argument("--ragged", type=int, default=0, help="K bags from U[2000, 15592] in turn through the graph stepper")
    ap.add_argument("--max_graphs", type=int, default=0, help="--ragged: the stepper's graph cap (0 = its default)")
    ap.add_argument("--attn", choices=["cls"], default=None, help="eval forward per N with and without the per-patch cls "
                    "attention (need_attn='cls'): ms and peak allocated bytes of both")
    ap.add_argument("--fused-a3", dest="fused_a3", action="store_true", help="eager training step per N with the landmark-query "
                    "pass materialised, fused (MIL_TM_FUSED_A3=1), materialised again: ms and peak allocated bytes")
    ap.add_argument("--fused-a1", dest="fused_a1", action="store_true", help="the same for the token-query pass "
                    "(MIL_TM_FUSED_A1); MIL_TM_FUSED_A3 stays as the environment has it")
    ap.add_argument("--deterministic", action="store_true", help="eager training step per N with the fixed-order sums off and "
                    "on in alternating regions; with --graph the replayed step too")
    ap.add_argument("--pieces", type=int, choices=[0, 3], default=None, help="the default rows with TransMIL.gemm_pieces set: 3 = "
                    "split-bf16 products in the Nystrom core, 0 = fp32 products; unset: MIL_TM_PIECES decides")
    ap.add_argument("--bags", type=int, default=1, help="B > 1: the training step over B bags of N patches, eager and "
                    "replayed, with TransMIL.batch_bags off, on, off again: ms and peak allocated bytes")
    ap.add_argument("--packed", action="store_true", help="--bags B: one more column, the step with TransMIL.packed set (a step's "
                    "bags as one packed sequence) and the one with TransMIL.packed_ppeg on top (PPEG as one launch set), between `on` and `off_again`.  It always runs both attention passes fused: "
                    "set MIL_TM_FUSED_A1=1 MIL_TM_FUSED_A3=1 so that the other two columns do too")
    ap.add_argument("--mix", action="store_true", help="--bags B: a ragged mix, bag b of N (4 - b mod 4) / 4 patches")
    ap.add_argument("--packed-cls", dest="packed_cls", action="store_true", help="the eval forward with patch_attn for 2 / 4 / 8 "
                    "ragged bags of up to N patches (give --N 2000): bag by bag with MIL_TM_FUSED_CLS next to the packed route with "
                    "TransMIL.packed_cls, eager and replayed, alternating regions of --calls forwards")
    ap.add_argument("--calls", type=int, default=10, help="--packed-cls: forwards per timed region")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda")
    args = SimpleNamespace(modality=["pathology"], model_pathology="TransMIL", num_classes=2, patch_dim=768, variant="image_only")
    if a.packed_cls:
        cls_packed_rows(a, dev, args)
        return
    if a.bags > 1:
        bags_rows(a, dev, args)
        return
    if a.attn:
        attn_rows(a, dev, args)
        return
    if a.fused_a3:
        fused_rows(a, dev, args)
        return
    if a.fused_a1:
        fused_rows(a, dev, args, "MIL_TM_FUSED_A1", "a1")
        return
    if a.deterministic:
        det_rows(a, dev, args)
        return
    if a.graph or a.ragged:
        if a.graph:
            graph_rows(a, dev, args)
        if a.ragged:
            ragged_run(a, dev, args)
        return
    torch.manual_seed(1234)
    model = get_model(args).to(dev).eval()        # eval: dropout off, gradients still flow
    if a.pieces is not None:
        model.extractor_pathology.gemm_pieces = a.pieces
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
        res = dict(N=N, n_pad=geometry(N)["n_pad"], gf_fwd=round(gf, 2), gf_step=round(3 * gf, 2))
        for tag, fn in (("fwd", fwd), ("step", step)):
            ts = region_times(fn, a.reps, a.warmup)
            res[tag + "_ms"] = round(sorted(ts)[len(ts) // 2], 3)
            if a.pieces is not None:
                res.update({tag + "_min_ms": round(min(ts), 3), tag + "_max_ms": round(max(ts), 3)})
        if a.pieces is not None:
            res["pieces"] = a.pieces
        res["step_frac_peak"] = round(3 * gf / (res["step_ms"] * 1e-3) / (PEAK_TF * 1e3), 4)
        if not a.no_torch:
            res["torch_fwd_ms"] = round(timed(t_fwd, a.reps, a.warmup), 3)
            res["torch_step_ms"] = round(timed(t_step, a.reps, a.warmup), 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
