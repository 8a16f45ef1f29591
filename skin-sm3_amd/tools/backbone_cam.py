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

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import explain_cli as cli  # noqa: E402
from sm3hip import cam  # noqa: E402
from sm3hip.cam import STAGES  # noqa: E402
from sm3hip.metrics import NUM_CLASSES  # noqa: E402


def add_cam_args(p):
    cli.add_target_arg(p)
    p.add_argument("--cam-layer", default="layer4", choices=STAGES, help="encoder stage whose output the maps weight")
    return cli.add_cases_args(p)


def get_parser():
    return add_cam_args(cli.backbone_parser("SM3 Grad-CAM maps of a linear probe (MI355X)"))


def per_batch(model, derm, clinic, lab, args):
    out = cam.grad_cam(model, derm, clinic, layer=args.cam_layer, target=args.target)
    return {"maps": out["maps"].half(), "low_res": out["low_res"], "logits": out["logits"], "targets": lab,
            "target_class": out["target_class"]}


def run(args, parser, tool, mlc):
    saved, stat = cli.explain(args, parser, tool, mlc, per_batch, "cam.pt", target=args.target, layer=args.cam_layer)
    print(f"{tool} ({args.target}, {args.cam_layer}): {stat['cases']} cases x {len(NUM_CLASSES)} labels, maps "
          f"{tuple(saved['maps'].shape)} | {stat['images_per_s']:.1f} images/s", flush=True)
    return stat


def main(argv=None):
    parser = get_parser()
    return run(parser.parse_args(argv), parser, "backbone_cam", False)


if __name__ == "__main__":
    main()
