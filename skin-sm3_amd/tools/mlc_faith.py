"""Deletion / insertion faithfulness curves of the attribution maps of the SM3 multi-label model (inference.py `Model`) on
MI355X (sm3hip/faith.py).

    python tools/mlc_faith.py --data-name SevenPCBaseDataset --data-path ./data/7PC -a resnet50 -b 8 --mlc-proj v4 \
        --mlc-proj-dim 512 --num-heads 1 --sa-dim-ff 128 --checkpoint logs/mlc_eval/best_finetune.pth \
        --log-path logs/mlc_eval/faith --method cam --cam-layer layer4 --curve-steps 32 --split test --max-cases 64

Takes tools/mlc_cam.py's and tools/mlc_attr.py's command lines (mlc_eval's model and data flags, --checkpoint, --target, --split,
--max-cases) with the flags of tools/backbone_faith.py (--method cam|ig|smoothgrad|random|rise and that method's own flags,
--curve-steps, --curve-mode, --modality, --chunk).  The heads run in eval semantics.  faith.pt goes to --log-path with the fields
backbone_faith writes.
"""
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import backbone_faith  # noqa: E402
import explain_cli as cli  # noqa: E402


def get_parser():
    return cli.add_faith_args(cli.mlc_parser(
        "SM3 deletion / insertion faithfulness curves of the multi-label model's attribution maps (MI355X)", "./logs/mlc_faith"))


def main(argv=None):
    parser = get_parser()
    return backbone_faith.run(parser.parse_args(argv), parser, "mlc_faith", True)


if __name__ == "__main__":
    main()
