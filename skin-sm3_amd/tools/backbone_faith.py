"""Deletion / insertion faithfulness curves of a linear probe's attribution maps on MI355X: does each of the 8 derm7pt label
predictions fall when the pixels a map calls important are taken away, and rise when only they are shown (sm3hip/faith.py)?

    python tools/backbone_faith.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 8 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/faith --method ig --steps 32 --curve-steps 32 --max-cases 64

Takes tools/backbone_cam.py's and tools/backbone_attr.py's command lines with --method cam|ig|smoothgrad|random (and that
method's own flags: --cam-layer; --steps / --samples / --sigma / --squared / --attr-seed), --curve-steps, --curve-mode
both|deletion|insertion, --modality joint|derm|clinic and --chunk (curve steps per encoder forward).  random ranks a uniform
random map seeded by --attr-seed: the control a faithfulness table needs.  The maps are computed with the chosen method on the
engine, then ranked and scored; the baseline is zero in normalised space (the dataset-mean image).  faith.pt goes to --log-path:
deletion / insertion [n, 8, curve-steps + 1] fp64, deletion_auc / insertion_auc [n, 8] fp64, logits and baseline_logits (8
tensors [n, classes]), targets [n, 8], target_class [n, 8], indices [n], method, labels.  A low deletion AUC and a high insertion
AUC say that the map is faithful.
"""
import os
import sys
import time

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import torch  # noqa: E402

import backbone_attr  # noqa: E402
import backbone_eval  # noqa: E402
from backbone_saliency import load_linear  # noqa: E402
from sm3hip.cam import STAGES  # noqa: E402
from sm3hip.faith import MODALITIES, MODES  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES  # noqa: E402

METHODS = ("cam", "ig", "smoothgrad", "random")


def add_faith_args(p):
    """The flags the two faithfulness tools share: those of the attribution tools, --cam-layer and the curve's own."""
    backbone_attr.add_attr_args(p, method_help="how the maps are made: " + ", ".join(METHODS),
                                chunk_help="curve steps per encoder forward (default: from the free device memory); any value "
                                           "gives the same bits")
    p.set_defaults(method="cam")
    p.add_argument("--cam-layer", default="layer4", help="cam: encoder stage whose output the maps weight (layer1 .. layer4)")
    p.add_argument("--curve-steps", default=32, type=int, help="steps of the deletion / insertion curves (at most H * W)")
    p.add_argument("--curve-mode", default="both", help="both, deletion or insertion")
    p.add_argument("--modality", default="joint", help="joint (both images perturbed, each by its own map), derm or clinic")
    return p


def check_faith_args(args, tool, size):
    """Refusals that need no device.  size: (H, W) of the images."""
    if args.method not in METHODS:
        raise SystemExit(f"{tool}: --method {args.method} is not available (one of {', '.join(METHODS)})")
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
    if args.attr_seed < 0:
        raise SystemExit(f"{tool}: --attr-seed must be non-negative")


def get_parser():
    p = backbone_eval.get_parser()
    p.description = "SM3 deletion / insertion faithfulness curves of a linear probe's attribution maps (MI355X)"
    p.add_argument("--linear-path", type=str, default=None,
                   help="backbone_eval's best_linear.pth (a Baseline state_dict); required with real data")
    return add_faith_args(p)


def make_maps(model, derm, clinic, args, gen):
    """(maps [N, 8, 2, H, W] fp32 on the images' device, target for the curves) by --method; gen: the CPU generator of random."""
    from sm3hip import attr, cam
    if args.method == "random":
        N, _, H, W = derm.shape
        return torch.rand(N, len(NUM_CLASSES), 2, H, W, generator=gen).to(derm.device), args.target
    if args.method == "cam":
        out = cam.grad_cam(model, derm, clinic, layer=args.cam_layer, target=args.target)
    elif args.method == "ig":
        out = attr.integrated_gradients(model, derm, clinic, target=args.target, steps=args.steps)
    else:
        out = attr.smooth_grad(model, derm, clinic, target=args.target, samples=args.samples, sigma=args.sigma,
                               squared=args.squared, seed=args.attr_seed)
    return out["maps"], out["target_class"]  # the curves follow the classes the maps explain


def run(model, data, args):
    """Maps, then curves, over the batches of `data`; the collected outputs (CPU) and the seconds it took."""
    from sm3hip import faith
    gen = torch.Generator().manual_seed(args.attr_seed)
    curves = [n for n in ("deletion", "insertion") if args.curve_mode in ("both", n)]
    keys = curves + [n + "_auc" for n in curves]
    got = {k: [] for k in keys + ["targets", "target_class"]}
    logits, base_logits = [[] for _ in NUM_CLASSES], [[] for _ in NUM_CLASSES]
    torch.cuda.synchronize()
    t0 = time.time()
    for derm, clinic, lab in data:
        maps, target = make_maps(model, derm, clinic, args, gen)
        out = faith.deletion_insertion(model, derm, clinic, maps, target=target, steps=args.curve_steps, modality=args.modality,
                                       mode=args.curve_mode, chunk=args.chunk)
        for k in keys:
            got[k].append(out[k].cpu())
        for i in range(len(NUM_CLASSES)):
            logits[i].append(out["logits"][i].cpu())
            base_logits[i].append(out["baseline_logits"][i].cpu())
        got["targets"].append(lab.cpu())
        got["target_class"].append(out["target_class"].cpu())
    torch.cuda.synchronize()
    saved = {k: torch.cat(v) for k, v in got.items()}
    saved.update(logits=[torch.cat(l) for l in logits], baseline_logits=[torch.cat(l) for l in base_logits])
    return saved, time.time() - t0


def save(saved, args, seconds, tool):
    os.makedirs(args.log_path, exist_ok=True)
    torch.save(saved, os.path.join(args.log_path, "faith.pt"))
    n = saved["target_class"].shape[0]
    stat = {"cases": n, "images_per_s": 2 * n / seconds, "seconds": seconds}  # derm + clinic
    print(f"{tool} ({args.method}, {args.target}, {args.modality}, {args.curve_steps} curve steps): {n} cases x "
          f"{len(NUM_CLASSES)} labels | {stat['images_per_s']:.2f} images/s", flush=True)
    for name in ("deletion", "insertion"):
        if name + "_auc" in saved:
            per = saved[name + "_auc"].mean(dim=0)
            stat[name + "_auc"] = float(per.mean())
            print(f"{tool}: mean {name} AUC " + "  ".join(f"{c} {float(v):.4f}" for c, v in zip(CLASSES_NAME, per)) +
                  f"  | average {stat[name + '_auc']:.4f}", flush=True)
    return stat


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, ignored_line, require_baseline_arch, require_data
    require_baseline_arch(args.arch, "backbone_faith")
    check_faith_args(args, "backbone_faith", tuple(args.img_sz))
    real = require_data(args, "backbone_faith")
    if args.linear_path is not None and not os.path.isfile(args.linear_path):
        raise SystemExit(f"backbone_faith: --linear-path {args.linear_path} does not exist")
    if real and args.linear_path is None:
        raise SystemExit("backbone_faith: --linear-path (backbone_eval's best_linear.pth) is required with real data")
    if ignored_line(args, parser, real):
        print("accepted for compatibility, without effect in this build:", " ".join(ignored_line(args, parser, real)), flush=True)
    from src.models.baseline import Baseline
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    model = Baseline(args.arch, args.arch_weights)
    if args.linear_path is not None:
        load_linear(model, args.linear_path)
        print(f"loaded linear probe from '{args.linear_path}'")
    for m in (model.derm_backbone, model.clinic_backbone):
        m.sm3_dtype = amp_dtype(args)
    model.to(dev).eval()
    if real:
        from sm3hip.augment import chain
        from sm3hip.imagestore import build_for
        from src.utils.data.sampler import eval_batches
        store = build_for(args, [args.split], dev)
        split = store.splits[args.split]
        n = min(args.max_cases, len(split))
        aug = chain("backbone_eval", tuple(args.img_sz), args.mean, args.std)
        sels = [s[s < n] for s in eval_batches(len(split), args.batch_size)]
        sels = [s for s in sels if s.numel()]
        data = backbone_eval.real_batches(store, split, aug, sels, None, True)
        indices = torch.cat(sels)
    else:
        n = args.max_cases
        sizes = [min(args.batch_size, n - s) for s in range(0, n, args.batch_size)]
        data = (backbone_eval.synthetic(b, args.img_sz, dev, gen) for b in sizes)
        indices = torch.arange(n)
    saved, seconds = run(model, data, args)
    saved.update(indices=indices, target=args.target, method=args.method, modality=args.modality, curve_steps=args.curve_steps,
                 labels=list(CLASSES_NAME), split=args.split if real else "synthetic")
    return save(saved, args, seconds, "backbone_faith")


if __name__ == "__main__":
    main()
