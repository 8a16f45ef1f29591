"""Deletion / insertion faithfulness curves of the attribution maps of the SM3 multi-label model (inference.py `Model`) on
MI355X (sm3hip/faith.py).

    python tools/mlc_faith.py --data-name SevenPCBaseDataset --data-path ./data/7PC -a resnet50 -b 8 --mlc-proj v4 \
        --mlc-proj-dim 512 --num-heads 1 --sa-dim-ff 128 --checkpoint logs/mlc_eval/best_finetune.pth \
        --log-path logs/mlc_eval/faith --method cam --cam-layer layer4 --curve-steps 32 --split test --max-cases 64

Takes tools/mlc_cam.py's and tools/mlc_attr.py's command lines (mlc_eval's model and data flags, --checkpoint, --target, --split,
--max-cases) with the flags of tools/backbone_faith.py (--method cam|ig|smoothgrad|random and that method's own flags,
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

import torch  # noqa: E402

import backbone_eval  # noqa: E402
import backbone_faith  # noqa: E402
import mlc_cam  # noqa: E402
import mlc_eval  # noqa: E402
from sm3hip.metrics import CLASSES_NAME  # noqa: E402


def get_parser():
    p = mlc_eval.get_parser()
    p.description = "SM3 deletion / insertion faithfulness curves of the multi-label model's attribution maps (MI355X)"
    p.add_argument("--checkpoint", type=str, default=None,
                   help="a checkpoint inference.py loads (best_linear.pth / best_finetune.pth); required with real data")
    p.set_defaults(log_path="./logs/mlc_faith")
    return backbone_faith.add_faith_args(p)


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, require_data, require_mlc_arch, require_mlc_proj
    require_mlc_arch(args.arch, "mlc_faith")
    require_mlc_proj(args, "mlc_faith")
    size = (args.test_sz, args.test_sz)
    backbone_faith.check_faith_args(args, "mlc_faith", size)
    real = require_data(args, "mlc_faith")
    if args.checkpoint is not None and not os.path.isfile(args.checkpoint):
        raise SystemExit(f"mlc_faith: --checkpoint {args.checkpoint} does not exist")
    if real and args.checkpoint is None:
        raise SystemExit("mlc_faith: --checkpoint (a best_linear.pth / best_finetune.pth) is required with real data")
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    model = mlc_cam.build(args)
    if args.checkpoint is not None:
        mlc_cam.load_checkpoint(model, args.checkpoint)
        print(f"loaded model weights from '{args.checkpoint}'")
    for m in (model.extractor.derm_backbone, model.extractor.clinic_backbone):
        m.sm3_dtype = amp_dtype(args)
    model.to(dev).eval()
    if real:
        from sm3hip.augment import chain
        from sm3hip.imagestore import build_for
        from src.utils.data.sampler import eval_batches
        store = build_for(args, [args.split], dev)
        split = store.splits[args.split]
        n = min(args.max_cases, len(split))
        aug = chain("mlc_eval", size, args.mean, args.std)
        sels = [s[s < n] for s in eval_batches(len(split), args.batch_size)]
        sels = [s for s in sels if s.numel()]
        data = backbone_eval.real_batches(store, split, aug, sels, None, True)
        indices = torch.cat(sels)
    else:
        n = args.max_cases
        sizes = [min(args.batch_size, n - s) for s in range(0, n, args.batch_size)]
        data = (mlc_eval.synthetic(b, size, dev, gen) for b in sizes)
        indices = torch.arange(n)
    saved, seconds = backbone_faith.run(model, data, args)
    saved.update(indices=indices, target=args.target, method=args.method, modality=args.modality, curve_steps=args.curve_steps,
                 labels=list(CLASSES_NAME), split=args.split if real else "synthetic", mlc_proj=args.mlc_proj)
    return backbone_faith.save(saved, args, seconds, "mlc_faith")


if __name__ == "__main__":
    main()
