"""Grad-CAM class activation maps of a linear probe on MI355X: which region of the dermoscopic and the clinical image drives
each of the 8 derm7pt label predictions (sm3hip/cam.py).

    python tools/backbone_cam.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 32 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/cam --cam-layer layer4 --split test --max-cases 64

Takes backbone_eval's command line (and the data helpers backbone_saliency reuses) plus --linear-path (backbone_eval's
best_linear.pth, a Baseline state_dict), --target, --cam-layer, --split and --max-cases.  The model runs in eval mode on the
validation chain (Resize -> Normalize).  For label i the target is the logit of the argmax class (--target pred) or of the
class AUC_AVG scores (--target cls, sm3hip.metrics.CLS_WEIGHTS).  cam.pt goes to --log-path: maps [n, 8, 2, H, W] fp16 in
[0, 1] (derm, clinic), low_res [n, 8, 2, h, w] fp32 (the stage-resolution maps before upsampling and normalisation), logits
(8 tensors [n, classes]), targets [n, 8], target_class [n, 8], indices [n] (positions in the split; with --data-name
synthetic, in the generated stream), layer.
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

import backbone_eval  # noqa: E402
from backbone_saliency import load_linear  # noqa: E402
from sm3hip.cam import STAGES, TARGETS  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES  # noqa: E402


def get_parser():
    p = backbone_eval.get_parser()
    p.description = "SM3 Grad-CAM maps of a linear probe (MI355X)"
    p.add_argument("--linear-path", type=str, default=None,
                   help="backbone_eval's best_linear.pth (a Baseline state_dict); required with real data")
    p.add_argument("--target", default="pred", choices=TARGETS,
                   help="logit per label: pred = the argmax class, cls = the class AUC_AVG scores (CLS_WEIGHTS)")
    p.add_argument("--cam-layer", default="layer4", choices=STAGES, help="encoder stage whose output the maps weight")
    p.add_argument("--split", default="test", choices=("test", "valid"))
    p.add_argument("--max-cases", default=64, type=int, help="cases of the split (or synthetic images) to map")
    return p


def run(model, data, target, layer):
    """grad_cam over the batches of `data`; the collected outputs (CPU) and the seconds it took."""
    from sm3hip.cam import grad_cam
    maps, low, logits, targets, tcls = [], [], [[] for _ in NUM_CLASSES], [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for derm, clinic, lab in data:
        out = grad_cam(model, derm, clinic, layer=layer, target=target)
        maps.append(out["maps"].half().cpu())
        low.append(out["low_res"].cpu())
        for i, o in enumerate(out["logits"]):
            logits[i].append(o.cpu())
        targets.append(lab.cpu())
        tcls.append(out["target_class"].cpu())
    torch.cuda.synchronize()
    return {"maps": torch.cat(maps), "low_res": torch.cat(low), "logits": [torch.cat(l) for l in logits],
            "targets": torch.cat(targets), "target_class": torch.cat(tcls)}, time.time() - t0


def save(saved, args, seconds, tool):
    os.makedirs(args.log_path, exist_ok=True)
    torch.save(saved, os.path.join(args.log_path, "cam.pt"))
    n = saved["maps"].shape[0]
    stat = {"cases": n, "images_per_s": 2 * n / seconds, "seconds": seconds}  # derm + clinic
    print(f"{tool} ({args.target}, {args.cam_layer}): {n} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(saved['maps'].shape)} | {stat['images_per_s']:.1f} images/s", flush=True)
    return stat


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, ignored_line, require_baseline_arch, require_data
    require_baseline_arch(args.arch, "backbone_cam")
    real = require_data(args, "backbone_cam")
    if args.linear_path is not None and not os.path.isfile(args.linear_path):
        raise SystemExit(f"backbone_cam: --linear-path {args.linear_path} does not exist")
    if real and args.linear_path is None:
        raise SystemExit("backbone_cam: --linear-path (backbone_eval's best_linear.pth) is required with real data")
    if args.max_cases < 1:
        raise SystemExit("backbone_cam: --max-cases must be at least 1")
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
    saved, seconds = run(model, data, args.target, args.cam_layer)
    saved.update(indices=indices, target=args.target, layer=args.cam_layer, labels=list(CLASSES_NAME),
                 split=args.split if real else "synthetic")
    return save(saved, args, seconds, "backbone_cam")


if __name__ == "__main__":
    main()
