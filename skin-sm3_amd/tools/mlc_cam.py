"""Grad-CAM class activation maps of the SM3 multi-label model (inference.py `Model`) on MI355X: which region of the
dermoscopic and the clinical image drives each of the 8 derm7pt label predictions (sm3hip/cam.py).

    python tools/mlc_cam.py --data-name SevenPCBaseDataset --data-path ./data/7PC -a resnet50 -b 32 --mlc-proj v4 \
        --mlc-proj-dim 512 --num-heads 1 --sa-dim-ff 128 --checkpoint logs/mlc_eval/best_finetune.pth \
        --log-path logs/mlc_eval/cam --cam-layer layer4 --split test --max-cases 64

Takes mlc_eval's command line (the model flags: -a, --mlc-proj, --mlc-proj-dim, --num-heads, --sa-dim-ff, --l2-norm; the
data flags: --data-name, --data-path, --mean, --std, --test-sz) plus --checkpoint, a best_linear.pth / best_finetune.pth
that inference.py loads ({"state_dict": ...}, "encoder." stripped from the keys, strict), and --target, --cam-layer, --split
and --max-cases as tools/backbone_cam.py.  The heads run in eval semantics (dropout off, the label projectors' BatchNorm1d
on running statistics).  Images: the validation chain (Resize(test_sz) -> Normalize) of the split, or random images at
--test-sz with --data-name synthetic.  cam.pt goes to --log-path with the fields backbone_cam writes.
"""
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import backbone_cam  # noqa: E402
import explain_cli as cli  # noqa: E402


def get_parser():
    return backbone_cam.add_cam_args(cli.mlc_parser("SM3 Grad-CAM maps of the multi-label model (MI355X)", "./logs/mlc_cam"))


def main(argv=None):
    parser = get_parser()
    return backbone_cam.run(parser.parse_args(argv), parser, "mlc_cam", True)


if __name__ == "__main__":
    main()
