"""What the explanation tools (backbone_saliency, backbone_cam / attr / faith, mlc_cam / attr / faith) share: their parsers'
common flags, the two subjects they explain -- a linear probe (backbone_eval's Baseline) and the multi-label model (inference.py
`Model`) -- with every refusal before the device is touched, the batches of a real split or of the synthetic stream, and the
loop that explains them batch by batch and writes the collected outputs.  Imported by the tools, which are run as scripts and have
put this directory on sys.path."""
import os
import time

import torch

import backbone_eval
import eval_cli
from sm3hip.attr import METHODS as ATTR_METHODS
from sm3hip.cam import STAGES, TARGETS
from sm3hip.faith import MODALITIES, MODES
from sm3hip.metrics import CLASSES_NAME
from sm3hip.rise import MAX_CELLS, MAX_MASKS, threshold
from src.models.baseline import Baseline

ATTR_TOOL_METHODS = ATTR_METHODS + ("rise",)  # the attribution tools also make the black-box maps of sm3hip/rise.py
FAITH_METHODS = ("cam", "ig", "smoothgrad", "random", "rise")


# ---- parsers ----------------------------------------------------------------------------------------------------------------
def backbone_parser(description):
    """backbone_eval's command line plus --linear-path."""
    p = backbone_eval.get_parser(tta_flags=False)
    p.description = description
    p.add_argument("--linear-path", type=str, default=None,
                   help="backbone_eval's best_linear.pth (a Baseline state_dict); required with real data")
    return p


def mlc_parser(description, log_path):
    """mlc_eval's command line plus --checkpoint, with the tool's own --log-path default."""
    import mlc_eval
    p = mlc_eval.get_parser(tta_flags=False)
    p.description = description
    p.add_argument("--checkpoint", type=str, default=None,
                   help="a checkpoint inference.py loads (best_linear.pth / best_finetune.pth); required with real data")
    p.set_defaults(log_path=log_path)
    return p


def add_target_arg(p):
    p.add_argument("--target", default="pred", choices=TARGETS,
                   help="logit per label: pred = the argmax class, cls = the class AUC_AVG scores (CLS_WEIGHTS)")
    return p


def add_cases_args(p, verb="map"):
    p.add_argument("--split", default="test", choices=("test", "valid"))
    p.add_argument("--max-cases", default=64, type=int, help=f"cases of the split (or synthetic images) to {verb}")
    return p


def add_attr_args(p, method_help="ig (Integrated Gradients), smoothgrad or rise (black-box: random masks, forward only)",
                  chunk_help="path points / samples / masks per encoder forward (default: from the free device memory); any value "
                             "gives the same bits"):
    """The flags the two attribution tools share (the place --cam-layer takes in the Grad-CAM tools)."""
    add_target_arg(p)
    p.add_argument("--method", default="ig", help=method_help)
    p.add_argument("--steps", default=32, type=int, help="ig: points of the midpoint rule on the path from the baseline")
    p.add_argument("--samples", default=16, type=int, help="smoothgrad: noisy copies per image")
    p.add_argument("--sigma", default=0.15, type=float, help="smoothgrad: noise level relative to each image's max - min")
    p.add_argument("--squared", action="store_true", help="smoothgrad: average the squared gradients")
    p.add_argument("--attr-seed", default=0, type=int, help="smoothgrad: seed of the noise; rise: seed of the masks")
    p.add_argument("--rise-masks", default=4000, type=int, help="rise: random masks per image pair")
    p.add_argument("--rise-cells", default=7, type=int, help="rise: cells of the binary grid a mask is upsampled from, per side")
    p.add_argument("--rise-p", default=0.5, type=float, help="rise: probability that a grid corner keeps the image")
    p.add_argument("--chunk", default=None, type=int, help=chunk_help)
    return add_cases_args(p, "attribute")


def check_rise_args(args, tool, size):
    """The refusals of --method rise that need no device.  size: (H, W) of the images."""
    if not 1 <= args.rise_masks <= MAX_MASKS:
        raise SystemExit(f"{tool}: --rise-masks must be between 1 and {MAX_MASKS}")
    if not 1 <= args.rise_cells <= min(MAX_CELLS, *size):
        raise SystemExit(f"{tool}: --rise-cells must be between 1 and min(H, W, {MAX_CELLS}) = {min(MAX_CELLS, *size)}")
    if not 0 < args.rise_p < 1 or threshold(args.rise_p) == 0:
        raise SystemExit(f"{tool}: --rise-p must lie strictly between 0 and 1")
    if (size[0] * size[1]) % 4:
        raise SystemExit(f"{tool}: the image's H * W ({size[0]} x {size[1]}) must be a multiple of 4")


def check_attr_args(args, tool, size):
    """Refusals that need no device.  size: (H, W) of the images (what --method rise asks of them)."""
    if args.method not in ATTR_TOOL_METHODS:
        raise SystemExit(f"{tool}: --method {args.method} is not available (one of {', '.join(ATTR_TOOL_METHODS)})")
    if args.max_cases < 1:
        raise SystemExit(f"{tool}: --max-cases must be at least 1")
    n, name = {"ig": (args.steps, "--steps"), "smoothgrad": (args.samples, "--samples"),
               "rise": (args.rise_masks, "--rise-masks")}[args.method]
    if args.method == "rise":
        check_rise_args(args, tool, size)
    if n < 1:
        raise SystemExit(f"{tool}: {name} must be at least 1")
    if args.chunk is not None and not 1 <= args.chunk <= n:
        raise SystemExit(f"{tool}: --chunk must be between 1 and {name} ({n})")
    if args.sigma < 0:
        raise SystemExit(f"{tool}: --sigma must be non-negative")
    if not 0 <= args.attr_seed < 2 ** 64:
        raise SystemExit(f"{tool}: --attr-seed must be non-negative and below 2^64")


def add_faith_args(p):
    """The flags the two faithfulness tools share: those of the attribution tools, --cam-layer and the curve's own."""
    add_attr_args(p, method_help="how the maps are made: " + ", ".join(FAITH_METHODS),
                  chunk_help="curve steps per encoder forward (default: from the free device memory); any value gives the same "
                             "bits")
    p.set_defaults(method="cam")
    p.add_argument("--cam-layer", default="layer4", help="cam: encoder stage whose output the maps weight (layer1 .. layer4)")
    p.add_argument("--curve-steps", default=32, type=int, help="steps of the deletion / insertion curves (at most H * W)")
    p.add_argument("--curve-mode", default="both", help="both, deletion or insertion")
    p.add_argument("--modality", default="joint", help="joint (both images perturbed, each by its own map), derm or clinic")
    return p


def check_faith_args(args, tool, size):
    """Refusals that need no device.  size: (H, W) of the images."""
    if args.method not in FAITH_METHODS:
        raise SystemExit(f"{tool}: --method {args.method} is not available (one of {', '.join(FAITH_METHODS)})")
    if args.max_cases < 1:
        raise SystemExit(f"{tool}: --max-cases must be at least 1")
    hw = size[0] * size[1]
    if hw % 4:
        raise SystemExit(f"{tool}: the image's H * W ({size[0]} x {size[1]}) must be a multiple of 4")
    if not 1 <= args.curve_steps <= hw:
        raise SystemExit(f"{tool}: --curve-steps must be between 1 and H * W ({hw})")
    if args.chunk is not None and not 1 <= args.chunk <= args.curve_steps:
        raise SystemExit(f"{tool}: --chunk must be between 1 and --curve-steps ({args.curve_steps})")
    if args.curve_mode not in MODES:
        raise SystemExit(f"{tool}: --curve-mode {args.curve_mode} is not available (one of {', '.join(MODES)})")
    if args.modality not in MODALITIES:
        raise SystemExit(f"{tool}: --modality {args.modality} is not available (one of {', '.join(MODALITIES)})")
    if args.method == "cam" and args.cam_layer not in STAGES:
        raise SystemExit(f"{tool}: --cam-layer {args.cam_layer} is not available (one of {', '.join(STAGES)})")
    if args.method == "ig" and args.steps < 1:
        raise SystemExit(f"{tool}: --steps must be at least 1")
    if args.method == "smoothgrad" and args.samples < 1:
        raise SystemExit(f"{tool}: --samples must be at least 1")
    if args.method == "smoothgrad" and args.sigma < 0:
        raise SystemExit(f"{tool}: --sigma must be non-negative")
    if args.method == "rise":
        check_rise_args(args, tool, size)
    if not 0 <= args.attr_seed < 2 ** 64:
        raise SystemExit(f"{tool}: --attr-seed must be non-negative and below 2^64")


# ---- the two subjects -------------------------------------------------------------------------------------------------------
def load_linear(model, path):
    """backbone_eval's best_linear.pth ({"state_dict": ...}) or a bare state_dict; a "module." prefix is dropped."""
    state = torch.load(path, map_location="cpu")
    state = state.get("state_dict", state)
    model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in state.items()})


def build(args):
    """inference.py's Model with the --mlc-proj label projectors (build_model's layout for v4)."""
    import inference
    from src.models.projector import build_mlc_projectors
    extractor = inference.Extractor(args.arch)
    feat_dim = extractor.derm_feat_dim + extractor.clinic_feat_dim
    return inference.Model(extractor, build_mlc_projectors(args.mlc_proj, feat_dim, args.mlc_proj_dim, args.num_labels),
                           args.mlc_proj_dim, args.l2_norm, args.num_heads, args.sa_dim_ff, args.sa_dropout)


def load_checkpoint(model, path):
    """As inference.py's __main__: {"state_dict": ...} (or a bare state_dict), "encoder." dropped from the keys, strict."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    state = dict(state.get("state_dict", state))
    for k in list(state):
        if "encoder." in k:
            state[k.replace("encoder.", "")] = state.pop(k)
    model.load_state_dict(state, strict=True)


def image_size(args, mlc):
    return (args.test_sz, args.test_sz) if mlc else tuple(args.img_sz)


def subject(args, parser, tool, mlc, check=None, freeze=False):
    """(model on the device in eval mode, device, its generator, whether the data is real) of a linear probe or, mlc=True, of the
    multi-label model.  Every refusal comes first (check(args, tool): the tool's own, after the architecture's); then the
    seeds -- torch's, then the device generator's -- the model, its weights and the encoders' arithmetic mode."""
    from src.utils import misc
    if mlc:
        misc.require_mlc_arch(args.arch, tool)
        misc.require_mlc_proj(args, tool)
        flag, path, what = "--checkpoint", args.checkpoint, "a best_linear.pth / best_finetune.pth"
    else:
        misc.require_baseline_arch(args.arch, tool)
        flag, path, what = "--linear-path", args.linear_path, "backbone_eval's best_linear.pth"
    if check is not None:
        check(args, tool)
    real = misc.require_data(args, tool)
    if path is not None and not os.path.isfile(path):
        raise SystemExit(f"{tool}: {flag} {path} does not exist")
    if real and path is None:
        raise SystemExit(f"{tool}: {flag} ({what}) is required with real data")
    if args.max_cases < 1:
        raise SystemExit(f"{tool}: --max-cases must be at least 1")
    if not mlc:
        eval_cli.ignored_notice(args, parser, real)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    model = build(args) if mlc else Baseline(args.arch, args.arch_weights)
    if path is not None:
        (load_checkpoint if mlc else load_linear)(model, path)
        print(f"loaded model weights from '{path}'" if mlc else f"loaded linear probe from '{path}'")
    if freeze:
        for p in model.parameters():
            p.requires_grad_(False)
    owner = model.extractor if mlc else model
    for m in (owner.derm_backbone, owner.clinic_backbone):
        m.sm3_dtype = misc.amp_dtype(args)
    return model.to(dev).eval(), dev, gen, real


def batches(args, mlc, dev, gen, real):
    """(batches of (derm, clinic, labels), their positions in the split or the generated stream, the split's name): the first
    --max-cases cases of --split through the validation chain, or synthetic images."""
    size = image_size(args, mlc)
    if real:
        from src.utils.data.sampler import eval_batches
        store, aug = eval_cli.image_store(args, [args.split], dev, size, "mlc_eval" if mlc else "backbone_eval")
        split = store.splits[args.split]
        n = min(args.max_cases, len(split))
        sels = [s[s < n] for s in eval_batches(len(split), args.batch_size)]
        sels = [s for s in sels if s.numel()]
        return eval_cli.split_batches(args, store, split, aug, sels), torch.cat(sels), args.split
    n = args.max_cases
    sizes = [min(args.batch_size, n - s) for s in range(0, n, args.batch_size)]
    return eval_cli.synthetic_batches(sizes, size, dev, gen), torch.arange(n), "synthetic"


# ---- the loop ---------------------------------------------------------------------------------------------------------------
def collect(data, per_batch):
    """per_batch(derm, clinic, labels) -> {key: tensor or list of tensors} for every batch of `data`; the outputs moved to the
    CPU and concatenated over the batches, and the seconds it took."""
    got = {}
    torch.cuda.synchronize()
    t0 = time.time()
    for batch in data:
        for k, v in per_batch(*batch).items():
            if isinstance(v, list):
                for held, o in zip(got.setdefault(k, [[] for _ in v]), v):
                    held.append(o.cpu())
            else:
                got.setdefault(k, []).append(v.cpu())
    torch.cuda.synchronize()
    saved = {k: [torch.cat(l) for l in v] if isinstance(v[0], list) else torch.cat(v) for k, v in got.items()}
    return saved, time.time() - t0


def explain(args, parser, tool, mlc, per_batch, file, check=None, freeze=False, **keys):
    """The whole of a tool after its parser: the subject, its batches, per_batch(model, derm, clinic, labels, args) over
    them, and <--log-path>/<file> with the collected outputs, the positions, `keys`, the label names and the split.  Returns
    (what was saved, {"cases", "images_per_s", "seconds"})."""
    model, dev, gen, real = subject(args, parser, tool, mlc, check, freeze)
    data, indices, split = batches(args, mlc, dev, gen, real)
    saved, seconds = collect(data, lambda derm, clinic, lab: per_batch(model, derm, clinic, lab, args))
    saved.update(indices=indices, **keys, labels=list(CLASSES_NAME), split=split)
    if mlc:
        saved["mlc_proj"] = args.mlc_proj
    os.makedirs(args.log_path, exist_ok=True)
    torch.save(saved, os.path.join(args.log_path, file))
    n = saved["target_class"].shape[0]
    return saved, {"cases": n, "images_per_s": 2 * n / seconds, "seconds": seconds}  # derm + clinic
