"""Flag system of the entry points.  Flag names and defaults follow the reference's config.py:10-142 for
everything the hot path reads (modality / model_* / aggregator / num_classes / learnablePrompt / n_ctx /
clinical_features / lr / b1 / b2 / batch_size / seed / dist_* ...), list flags are parsed with
ast.literal_eval as upstream (config.py:4-8).  Hospital-data flags are dropped; synthetic-data flags are new."""
import argparse
import ast


def arg_as_list(s):
    v = ast.literal_eval(s)
    if not isinstance(v, list):
        raise argparse.ArgumentTypeError(f'Argument "{s}" is not a list')
    return v


def create_arg_parser(argv=None):
    p = argparse.ArgumentParser(description="MI355X-native LLM-guided multi-modal MIL (hot path)")
    # ---- model (reference names; defaults chosen so the built path runs: upstream defaults select CT + TransMIL)
    p.add_argument("--modality", default=["pathology"], type=arg_as_list, help="subset of ['CT', 'pathology', 'CI'] ('CT': the encoder's feature map is a synthetic input)")
    p.add_argument("--alignment_base", default="CI", type=str)
    p.add_argument("--model_CT", default="resnetMC3_18", type=str)
    p.add_argument("--model_pathology", default="ABMIL", type=str,
                   help="image_only: ABMIL or TransMIL (Nystrom attention + PPEG; autograd path, replayed from hipGraphs with "
                        "--transmil_graph 1); fusion: ABMIL")
    p.add_argument("--model_CI", default="CLIP", type=str)
    p.add_argument("--aggregator", default="ABMIL", type=str)
    p.add_argument("--CI_prompt_version", default="single", type=str, help="single (1 note) | devided (10 prompts)")
    p.add_argument("--clinical_features", type=arg_as_list,
                   default=["sex", "age", "sm", "locationcancer", "cancerimaging", "cancerimagingT", "cancerimagingN",
                            "cancerimagingM", "classification_cancer"])
    p.add_argument("--learnablePrompt", default=0, type=int)
    p.add_argument("--n_ctx", default=8, type=int)
    p.add_argument("--prompt_len", default=0, type=int)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--variant", default="fusion", choices=["fusion", "image_only"],
                   help="fusion: model/aggregator.py path; image_only: model/aggregator_clip.py path")
    # ---- optimisation (train_ddp.py:104-118 forces lr 1e-5 for Adam with 2 classes)
    p.add_argument("--start_epoch", type=int, default=0)
    p.add_argument("--n_epochs", type=int, default=2)
    p.add_argument("--resume", default="", type=str)
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--loss", type=str, default="BCE", help="'BCE'; a name containing 'textCosSim' adds "
                   "CosineEmbeddingLoss(x_CT2CI, x_Pth2CI, 1) when both tokens exist (train_ddp.py:102,325-329)")
    p.add_argument("--cache_text", type=int, default=0, help="1: frozen text tower (learnablePrompt 0) - keep every note's "
                   "embedding after its first encode_text instead of recomputing it each step as model/dim1/CLIP.py:71-75 does "
                   "(same values: the tower is frozen)")
    p.add_argument("--train_contract", type=int, default=0, help="1: the module returns the tuple the reference's training "
                   "loop unpacks, ([out, out, out], [CT2CI, Pth2CI], None) (train_ddp.py:300), instead of the shipped "
                   "module's (aggregator.py:202-209)")
    p.add_argument("--loss_point", type=str, default="Last")
    p.add_argument("--schedule", default=[500], nargs="*", type=int)
    p.add_argument("--cos", action="store_true")
    p.add_argument("--b1", type=float, default=0.9)
    p.add_argument("--b2", type=float, default=0.999)
    p.add_argument("--seed", default=1234, type=int)
    p.add_argument("--batch_size", default=8, type=int, help="global mini-batch (divided by the number of GPUs)")
    p.add_argument("--iter_per_epoch", type=int, default=20)
    p.add_argument("--save_dir", type=str, default="")
    p.add_argument("--test_pth", type=str, default=None)
    p.add_argument("--best_thres", type=float, default=0.5)
    # ---- distributed (one process per GPU; torchrun env or mp.spawn as upstream train_ddp.py:622-624)
    p.add_argument("--gpu", default="0", type=str, help="comma-separated GPU ids when spawning")
    p.add_argument("--multiprocessing_distributed", action="store_true")
    p.add_argument("--dist_url", type=str, default="tcp://127.0.0.1:4444")
    p.add_argument("--dist_backend", type=str, default="nccl")
    p.add_argument("--world_size", type=int, default=1)
    p.add_argument("--rank", type=int, default=0)
    # ---- on-disk cohort (reference: --path_data_pathology, config.py; dataset.py:366-393).  A directory of
    # <patientid>.npy patch-feature bags [n, F] fp32 plus a JSON index {"id": {"label", "kind", "ids"}} in place of the
    # private Excel sheets; unset = synthetic bags.
    p.add_argument("--path_data_pathology", type=str, default="", help="directory of <patientid>.npy bags (dataset.py:367)")
    p.add_argument("--index_json", type=str, default="", help="cohort index; default <path_data_pathology>/index.json")
    p.add_argument("--augmentation", type=int, default=1, help="train-time patch drop (dataset.py:374-381)")
    p.add_argument("--resident_cohort", type=int, default=1,
                   help="with --hip_graph 1: load every bag ONCE into HBM (cohort.DeviceCohort), draw the per-epoch patch drop "
                        "on the device and feed each step by one gather launch; 0 = the host pipeline per step (np.load, "
                        "random.sample drop, zero-pad, pageable copy).  Falls back to 0 by itself when the cohort does not fit")
    p.add_argument("--patch_keep", type=float, default=1.0, help="synthetic cohorts: keep fraction of the per-epoch patch drop "
                   "(on-disk cohorts use the reference's 0.9 / 0.8 per bag kind)")
    # ---- synthetic data (no hospital data offline)
    p.add_argument("--synthetic", default=[1024, 768, 64], type=arg_as_list,
                   help="[patches per bag, patch feature dim, bags in the synthetic cohort]")
    p.add_argument("--ragged", action="store_true", help="draw a different patch count per bag")
    p.add_argument("--clip_layers", type=int, default=12)
    p.add_argument("--fused_step", action="store_true", help="image_only: fused trainer instead of autograd + DDP")
    p.add_argument("--no_dropout", action="store_true", help="--fused_step: eval-mode arithmetic (no dropout) while training; "
                   "the default is a true model.train() step with in-kernel dropout masks")
    p.add_argument("--clip_gemm_pieces", type=int, default=0, choices=[0, 2, 3],
                   help="frozen CLIP text tower: 0 = fp32 MFMA GEMMs (parity path); 2 / 3 = split-bf16 products "
                        "(3 / 6 cross terms: ~3e-6 / fp32-level relative error, 2.3x / 1.45x the fp32 GEMM rate)")
    p.add_argument("--hip_graph", type=int, default=0, help="autograd path: capture forward + backward of a repeating "
                   "batch shape in a hipGraph and replay it (graph_step.py); meant for the one-bag-per-GPU regime")
    p.add_argument("--transmil_graph", type=int, default=0, help="image_only + --model_pathology TransMIL: replay the step "
                   "from one hipGraph per grid side s = ceil(sqrt(N)), bag lengths and the gather index on the device "
                   "(transmil_step.RaggedTransMILStepper); feeds from the HBM-resident cohort when --resident_cohort 1 fits.  "
                   "test_ddp.py: its per-bag eval forward is replayed the same way (the model built by build_model does it)")
    p.add_argument("--transmil_max_graphs", type=int, default=0, help="--transmil_graph 1: most graphs kept (0 = the "
                   "stepper's default); a grid side beyond the cap runs eagerly")
    p.add_argument("--save_patch_attn", type=str, default="", help="test_ddp.py, image_only + --model_pathology TransMIL: write "
                   "DIR/<bag key or index>.npy per bag, float32 [2, 8, N] = layers x heads x patches, the cls token's attention "
                   "to each patch (a repeated patch's two keys summed; not renormalised), bags in the order test_ddp.py runs "
                   "them.  Works with and without --transmil_graph 1; the files are written when the run ends")
    p.add_argument("--save_note_attn", type=str, default="", help="test_ddp.py, --variant fusion --modality \"['pathology']\": "
                   "write DIR/<bag key or index>.npz per bag with float32 note [3, P, 8, N] = attention sites (block 0, block 1, "
                   "final) x text tokens x heads x patches, the softmax weights of the note's token(s) over the patches, and bag "
                   "[N + P], the final gated-attention aggregator's weights, patches first (with --aggregator TransMIL "
                   "--fusion_transmil 1: bag [2, 8, N + P] = layers x heads x rows, the cls token's attention to each row of the "
                   "multi-modal bag, a repeated row's two keys summed, patches first).  The flag switches --hip_graph off: "
                   "with --hip_graph 1 the evaluation runs the eager forward, not the replayed one.  The files are written when "
                   "the run ends.  With --note_attn_scope all also --modality \"['CT']\" and \"['CT','pathology']\", and "
                   "--hip_graph 1 (stays on) or --fusion_transmil_graph 1: the weights come out of the replayed forward.  With CT "
                   "the file gains note_ct [3, P, 8, D], the note's weights over the D CT tokens at the three sites of the "
                   "transformer's CT pass; note is there only with pathology; bag covers the whole multi-modal bag in memory "
                   "order: [D + P] (CT tokens, text tokens) or [N + P + D + P] (patches, CT-side text tokens, CT tokens, "
                   "pathology-side text tokens), [2, 8, that] with the TransMIL aggregator")
    p.add_argument("--note_attn_scope", type=str, default="pathology", choices=["pathology", "all"],
                   help="what --save_note_attn covers.  pathology: --modality \"['pathology']\" on the eager forward (model.note_attn "
                        "= True).  all: wherever the token->image sites run on the absorbed pools - CT in the modality, the "
                        "capacity-bucket forwards and the replayed evaluation (model.note_attn = 'all'); --modality \"['CI']\" and "
                        "--variant image_only stay refused")
    p.add_argument("--flat_adam", type=int, default=1, help="autograd path: parameters in one flat buffer, one gradient "
                   "all-reduce and one Adam launch per step (optim.FlatAdam); 0 = torch DDP + torch.optim.Adam")
    p.add_argument("--fusion_transmil", type=int, default=0, help="--variant fusion: 1 = build --aggregator TransMIL (and "
                   "--model_pathology TransMIL's unused extractor) over the multi-modal bag, rows in upstream's sequence "
                   "order, bags one after another; eager autograd path (refused with --hip_graph 1; its graph path is "
                   "--fusion_transmil_graph 1).  0: both "
                   "values raise NotImplementedError as before")
    p.add_argument("--fusion_transmil_graph", type=int, default=0, help="--variant fusion --aggregator TransMIL "
                   "--fusion_transmil 1 --flat_adam 1, modality ['pathology'] or ['CT','pathology']: replay the step from one "
                   "hipGraph per (row capacity, grid sides of the multi-modal bags), bag lengths and TransMIL's gather index on "
                   "the device (fusion_step.RaggedFusionTransMILStepper); Adam inside the graph at world size 1; the training "
                   "step runs on TransMIL's fixed-order sums (--deterministic 1 implied).  test_ddp.py "
                   "replays its per-bag eval forward from the same graphs.  Refused with --hip_graph 1 and --learnablePrompt 1")
    p.add_argument("--deterministic", type=int, default=0, help="train_ddp.py and test_ddp.py: 1 = every sum of the TransMIL "
                   "forward and backward that crosses workgroups (split-K products, the gather's backward, the res_conv and "
                   "PPEG weight gradients) is taken in an order fixed by the shapes, without float atomics, so that two runs "
                   "from one seed on one GPU give the same bits; set on every TransMIL module of the model (--model_pathology "
                   "TransMIL, --aggregator TransMIL --fusion_transmil 1), eager or replayed (--transmil_graph 1).  Models "
                   "without a TransMIL module accept the flag and do nothing: their steps hold no float atomic.  0: the "
                   "environment variable MIL_TM_DETERMINISTIC decides (default off)")
    p.add_argument("--tm_gemm_pieces", type=int, default=0, choices=[0, 3],
                   help="train_ddp.py and test_ddp.py: 3 = the Nystrom core's products with K >= 256 (the pseudo-inverse chain, "
                        "W, U, O and their gradients) as three-piece split-bf16 products on bf16 MFMA, six cross terms, "
                        "fp32-level error; set on every TransMIL module of the model.  Models without a TransMIL module accept "
                        "the flag and ignore it.  0: the environment variable MIL_TM_PIECES decides (default 0 = fp32 MFMA)")
    p.add_argument("--tm_batch_bags", type=int, default=0, choices=[0, 1],
                   help="train_ddp.py and test_ddp.py: 1 = a TransMIL step of several bags (--batch_size > 1, several bags per "
                        "slot, the fusion model's TransMIL aggregator) runs the landmark-side chain of its bags - A2, the "
                        "pseudo-inverse, U and their gradients - as one set of launches at batch 8 x bags instead of once per "
                        "bag; each bag keeps its own pseudo-inverse scale.  Which steps take this route: ops.tm_route (DESIGN 4.6, "
                        "Route of a step).  Set on every TransMIL module of the model.  Models without a TransMIL "
                        "module accept the flag and ignore it.  0: the environment variable MIL_TM_BATCH_BAGS decides (default 0)")
    p.add_argument("--tm_packed", type=int, default=0, choices=[0, 1],
                   help="train_ddp.py and test_ddp.py: 1 = a TransMIL step of several bags runs every layer over ONE packed "
                        "sequence of all bags' rows - LayerNorm, the pad gather, to_qkv, the landmarks, both fused attention "
                        "passes, the residual conv, to_out, the dropout and the residual one launch set each, whatever the "
                        "number of bags; PPEG stays per bag (--tm_packed_ppeg).  Which steps take this route: ops.tm_route (DESIGN 4.6, Route of a "
                        "step).  Set on every TransMIL module of the model.  Models "
                        "without a TransMIL module accept the flag and ignore it.  0: the environment variable MIL_TM_PACKED "
                        "decides (default 0)")
    p.add_argument("--tm_packed_ppeg", type=int, default=0, choices=[0, 1],
                   help="train_ddp.py and test_ddp.py: 1 = where --tm_packed 1 runs a TransMIL step over one packed sequence, "
                        "PPEG too is one launch set over all bags' sequence rows (a table of per-bag row offsets and sides), "
                        "with no per-bag slice or concatenation between the two layers; per bag the same values, the PPEG "
                        "weight and bias gradients one sum over all bags.  When it applies: ops.tm_route (DESIGN 4.6).  Set "
                        "on every TransMIL module of the model, as --tm_packed is.  0: the environment variable "
                        "MIL_TM_PACKED_PPEG decides (default 0)")
    p.add_argument("--tm_packed_cls", type=int, default=0, choices=[0, 1],
                   help="train_ddp.py and test_ddp.py: 1 = with --tm_packed 1, a TransMIL step of several bags that asks for the "
                        "per-patch cls attention (--save_patch_attn, the fusion model's note attention over a TransMIL "
                        "aggregator) stays on the packed route: each layer's cls attention of all bags is one launch set, "
                        "bit-equal per bag to the fused single-bag kernels.  When it applies: ops.tm_route (DESIGN 4.6).  "
                        "Set on every TransMIL module of the model, as --tm_packed is.  0: the "
                        "environment variable MIL_TM_PACKED_CLS decides (default 0)")
    # ---- validation and metrics (metrics.EvalLog: a device-side log, one small launch per forward, one host read per pass)
    p.add_argument("--validate", type=int, default=0, choices=[0, 1],
                   help="train_ddp.py: 1 = after every epoch run the validation bags one per forward (eval mode, true lengths, "
                        "no zero padding) and print one 'Valid Epoch' line - loss, accuracy and the AUC / recall / precision of "
                        "the argmax predictions as the reference's valid(), for two classes also the score AUC and the Youden "
                        "threshold; writes checkpoint_last.pth.tar every epoch.  0: no validation, checkpoints as before")
    p.add_argument("--index_json_valid", type=str, default="", help="--validate 1 with an on-disk cohort: the validation "
                   "cohort's index (bags under --path_data_pathology); synthetic cohorts draw their own validation bags")
    p.add_argument("--save_best", action="store_true", help="--validate 1: write checkpoint_{epoch:04d} and checkpoint_best only "
                   "when the validation AUC is >= the best so far (the reference's flag); off: every epoch")
    args = p.parse_args(argv)
    if args.fusion_transmil and args.hip_graph:
        # refused here, before an entry point touches the GPU: the bucketed steppers key their graphs by row capacity,
        # TransMIL's shapes follow the grid side of each bag
        raise ValueError("--fusion_transmil 1 runs on the eager autograd path only: drop --hip_graph 1")
    if args.fusion_transmil_graph:
        # refused here too: the stepper replays the fusion model's TransMIL-aggregator step with a counted FlatAdam inside
        if (args.variant != "fusion" or args.aggregator != "TransMIL" or not args.fusion_transmil or not args.flat_adam):
            raise ValueError("--fusion_transmil_graph 1 needs --variant fusion --aggregator TransMIL --fusion_transmil 1 "
                             "--flat_adam 1")
        if list(args.modality) not in (["pathology"], ["CT", "pathology"]):
            raise ValueError("--fusion_transmil_graph 1 is built for --modality \"['pathology']\" and \"['CT','pathology']\"")
        if args.learnablePrompt:
            raise ValueError("--fusion_transmil_graph 1: learnable prompts (their SGD inside the graph) are not built, "
                             "drop --learnablePrompt 1")
        if args.save_note_attn and args.note_attn_scope != "all":
            raise ValueError("--fusion_transmil_graph 1 keeps no attention weights: drop --save_note_attn "
                             "(or ask for them from the replayed forward: --note_attn_scope all)")
    if args.save_patch_attn and (args.variant != "image_only" or args.model_pathology != "TransMIL"):
        # refused here, before an entry point touches the GPU
        raise ValueError("--save_patch_attn writes TransMIL's cls-token attention: it needs --variant image_only "
                         "--model_pathology TransMIL (ABMIL keeps its scores in extractor_pathology.last_scores)")
    wide = args.note_attn_scope == "all" and list(args.modality) in (["CT"], ["CT", "pathology"])
    if args.save_note_attn and (args.variant != "fusion" or (list(args.modality) != ["pathology"] and not wide)):
        raise ValueError("--save_note_attn writes the note's attention over the patches: it needs --variant fusion "
                         "--modality \"['pathology']\"")
    if args.save_note_attn and args.hip_graph and args.note_attn_scope != "all":
        # the weights come out of the eager forward (model.note_attn), not the replayed one: test_ddp.py then takes its
        # op-by-op evaluation loop
        args.hip_graph = 0
    return args
