"""Integrated Gradients, SmoothGrad and RISE attributions of the SM3 multi-label model (inference.py `Model`) on MI355X: which
pixels of the dermoscopic and the clinical image drive each of the 8 derm7pt label predictions (sm3hip/attr.py, sm3hip/rise.py).

    python tools/mlc_attr.py --data-name SevenPCBaseDataset --data-path ./data/7PC -a resnet50 -b 8 --mlc-proj v4 \
        --mlc-proj-dim 512 --num-heads 1 --sa-dim-ff 128 --checkpoint logs/mlc_eval/best_finetune.pth \
        --log-path logs/mlc_eval/attr --method smoothgrad --samples 16 --sigma 0.15 --split test --max-cases 64

Takes tools/mlc_cam.py's command line (mlc_eval's model and data flags, --checkpoint, --target, --split, --max-cases) with the
attribution flags of tools/backbone_attr.py (--method, --steps, --samples, --sigma, --squared, --attr-seed, --rise-masks,
--rise-cells, --rise-p, --chunk) in the place of --cam-layer.  The heads run in eval semantics.  attr.pt goes to --log-path with the fields backbone_attr writes.
"""
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import backbone_attr  # noqa: E402
import explain_cli as cli  # noqa: E402


def get_parser():
    return cli.add_attr_args(cli.mlc_parser(
        "SM3 Integrated Gradients / SmoothGrad / RISE attributions of the multi-label model (MI355X)", "./logs/mlc_attr"))


def main(argv=None):
    parser = get_parser()
    return backbone_attr.run(parser.parse_args(argv), parser, "mlc_attr", True)


if __name__ == "__main__":
    main()
