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

import torch  # noqa: E402

import backbone_cam  # noqa: E402
import backbone_eval  # noqa: E402
import mlc_eval  # noqa: E402
from sm3hip.cam import STAGES, TARGETS  # noqa: E402
from sm3hip.metrics import CLASSES_NAME  # noqa: E402


def get_parser():
    p = mlc_eval.get_parser()
    p.description = "SM3 Grad-CAM maps of the multi-label model (MI355X)"
    p.add_argument("--checkpoint", type=str, default=None,
                   help="a checkpoint inference.py loads (best_linear.pth / best_finetune.pth); required with real data")
    p.add_argument("--target", default="pred", choices=TARGETS,
                   help="logit per label: pred = the argmax class, cls = the class AUC_AVG scores (CLS_WEIGHTS)")
    p.add_argument("--cam-layer", default="layer4", choices=STAGES, help="encoder stage whose output the maps weight")
    p.add_argument("--split", default="test", choices=("test", "valid"))
    p.add_argument("--max-cases", default=64, type=int, help="cases of the split (or synthetic images) to map")
    p.set_defaults(log_path="./logs/mlc_cam")
    return p


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


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import amp_dtype, require_data, require_mlc_arch, require_mlc_proj
    require_mlc_arch(args.arch, "mlc_cam")
    require_mlc_proj(args, "mlc_cam")
    real = require_data(args, "mlc_cam")
    if args.checkpoint is not None and not os.path.isfile(args.checkpoint):
        raise SystemExit(f"mlc_cam: --checkpoint {args.checkpoint} does not exist")
    if real and args.checkpoint is None:
        raise SystemExit("mlc_cam: --checkpoint (a best_linear.pth / best_finetune.pth) is required with real data")
    if args.max_cases < 1:
        raise SystemExit("mlc_cam: --max-cases must be at least 1")
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    model = build(args)
    if args.checkpoint is not None:
        load_checkpoint(model, args.checkpoint)
        print(f"loaded model weights from '{args.checkpoint}'")
    for m in (model.extractor.derm_backbone, model.extractor.clinic_backbone):
        m.sm3_dtype = amp_dtype(args)
    model.to(dev).eval()
    size = (args.test_sz, args.test_sz)
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
    saved, seconds = backbone_cam.run(model, data, args.target, args.cam_layer)
    saved.update(indices=indices, target=args.target, layer=args.cam_layer, labels=list(CLASSES_NAME),
                 split=args.split if real else "synthetic", mlc_proj=args.mlc_proj)
    return backbone_cam.save(saved, args, seconds, "mlc_cam")


if __name__ == "__main__":
    main()
