"""Label-free cross-modal retrieval report of an SSL checkpoint on MI355X: no training and no labels -- one eval-mode pass over
the held-out pairs, then, for every case, where the clinical image of the same case comes back among all held-out cases when
its dermoscopy image asks (and the other way round): Recall@k, mean / median rank, MRR with case-resampling bootstrap
intervals, and the held-out cross-modal InfoNCE value (sm3hip/retrieval.py).

    python tools/backbone_retrieval.py -a resnet50 --arch-version v32 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 128 -j 4 --img-sz 224 224 \
        --pretrain-path logs/backbone/ckp_399.pth --log-path logs/backbone/retrieval_399 --retrieval-k 1 5 10 --bootstrap 2000

Takes backbone_train's model flags (-a, --arch-version, --proj-dim, --amp, --amp-dtype) and backbone_eval's data flags and
validation chain (Resize -> Normalize of the whole image, the split backbone_eval validates on); --pretrain-path is a
checkpoint.pth.tar / ckp_N.pth of backbone_train.  The embeddings are the cross-modal projections (cross_proj) in eval mode
(sm3hip.retrieval.embed): a case's embedding is the same bits whatever -b is.  retrieval.json and retrieval.csv go to
--log-path, retrieval_embeddings.pt too with --save-embeddings; --against other/retrieval_embeddings.pt adds the paired
difference to another checkpoint's embeddings of the same cases (retrieval_compare.json).  `--data-name synthetic`: --val-steps
batches of backbone_train's latent-pattern pairs (their first views); without a checkpoint the model is the untrained one.
"""
import json
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

import backbone_train  # noqa: E402
import eval_cli  # noqa: E402
from sm3hip import retrieval  # noqa: E402

EMBEDDINGS = "retrieval_embeddings.pt"


def get_parser():
    from src.utils.misc import get_parser as base_parser
    p = base_parser("SM3 cross-modal retrieval report (MI355X)")
    p.add_argument("--arch-version", default="v3", type=str, choices=["v3", "v311", "v312", "v32", "v321", "v322"])
    p.add_argument("--arch-weights", default=None, type=str)
    p.add_argument("--proj-dim", default=128, type=int)
    p.add_argument("--val-steps", default=4, type=int, help="synthetic data only: batches of held-out pairs")
    retrieval.add_flags(p)
    p.add_argument("--save-embeddings", action="store_true", help=f"store the two embedding matrices in {EMBEDDINGS}")
    p.add_argument("--against", default=None, type=str,
                   help=f"a {EMBEDDINGS} of another checkpoint on the same cases: adds the paired differences")
    p.set_defaults(arch="resnet50", batch_size=128)
    return p


def build_model(args):
    """The model of backbone_train for these flags, on the CPU; SystemExit for an -a it cannot build."""
    from src.models.simclr import SimCLRSkinV3, SimCLRSkinV32
    from src.utils.misc import amp_dtype
    cls = SimCLRSkinV3 if args.arch_version in ("v3", "v311", "v312") else SimCLRSkinV32
    try:
        model = cls(arch=args.arch, weights=args.arch_weights, proj_dim=args.proj_dim, temperature=0.5)
    except (KeyError, NotImplementedError, ValueError, TypeError) as e:
        raise SystemExit(f"backbone_retrieval: -a {args.arch} cannot be built ({type(e).__name__}: {e})") from None
    model.sm3_dtype = amp_dtype(args)
    return model


def load_checkpoint(model, path):
    state = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
    model.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in state.items()})


def synthetic_pairs(steps, bs, size, dev, seed):
    """The first views of `steps` latent-pattern batches of backbone_train.synthetic_batch, from a generator of their own."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    for _ in range(steps):
        derm, clinic = backbone_train.synthetic_batch(bs, size, dev, gen, kind="latent")
        yield derm[0], clinic[0]


def embed_all(model, pairs):
    zd, zc = [], []
    for derm, clinic in pairs:
        a, b = retrieval.embed(model, derm, clinic)
        zd.append(a)
        zc.append(b)
    return torch.cat(zd), torch.cat(zc)


def load_embeddings(path):
    d = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(d, dict) or "derm" not in d or "clinic" not in d:
        raise SystemExit(f"backbone_retrieval: {path} is not a {EMBEDDINGS} (no 'derm' / 'clinic')")
    return d


def check_checkpoint(args, real, who="backbone_retrieval"):
    """The refusals about --pretrain-path: real data needs a checkpoint, and a named checkpoint must exist."""
    if real and not (args.pretrain_path and os.path.isfile(args.pretrain_path)):
        raise SystemExit(f"{who}: no checkpoint at --pretrain-path {args.pretrain_path!r}: a report on real data is "
                         "a report of a pre-trained model")
    if args.pretrain_path and not os.path.isfile(args.pretrain_path):
        raise SystemExit(f"{who}: no checkpoint at --pretrain-path {args.pretrain_path!r}")


def count_cases(args, real, who="backbone_retrieval", least=1, most=None):
    """The number of held-out cases these flags embed; SystemExit outside least .. most (MAX_CASES by default)."""
    most = retrieval.MAX_CASES if most is None else most
    if real:
        from src.utils.data.datasets import read_split
        N = len(read_split(args.data_path, "test")[2])
    else:
        if args.val_steps < 1 or args.batch_size < 1:
            raise SystemExit(f"{who}: --val-steps and -b must be positive")
        N = args.val_steps * args.batch_size
    if not least <= N <= most:
        raise SystemExit(f"{who}: {N} held-out cases, {least} to MAX_CASES = {most} are supported")
    return N


def embed_held_out(args, parser, real):
    """Builds the model of these flags, loads --pretrain-path, and embeds the held-out pairs on cuda:0: (z_derm, z_clinic,
    labels [N, 8] int64 on the CPU or None for synthetic data, seconds)."""
    model = build_model(args)
    eval_cli.ignored_notice(args, parser, real)
    if args.pretrain_path:
        load_checkpoint(model, args.pretrain_path)
        print(f"loaded pre-trained model weights from '{args.pretrain_path}'")
    # ---- the device, from here on
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    model.to(dev).eval()
    labels = None
    if real:
        store, aug = eval_cli.image_store(args, ["test"], dev)
        labels = store.splits["test"].labels.cpu()
        pairs = eval_cli.split_batches(args, store, store.splits["test"], aug, labels=False)
    else:
        pairs = synthetic_pairs(args.val_steps, args.batch_size, args.img_sz, dev, args.seed + 2000)
    torch.cuda.synchronize()
    t0 = time.time()
    zd, zc = embed_all(model, pairs)
    torch.cuda.synchronize()
    return zd, zc, labels, time.time() - t0


def embeddings_record(zd, zc, args):
    """What --save-embeddings stores."""
    return {"derm": zd.cpu(), "clinic": zc.cpu(), "N": zd.shape[0], "arch": args.arch, "arch_version": args.arch_version,
            "pretrain_path": args.pretrain_path}


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    retrieval.check_flags(args, "backbone_retrieval")
    from src.utils.misc import require_data
    real = require_data(args, "backbone_retrieval")
    check_checkpoint(args, real)
    if args.against and not os.path.isfile(args.against):
        raise SystemExit(f"backbone_retrieval: --against {args.against} does not exist")
    count_cases(args, real)
    zd, zc, _, embed_s = embed_held_out(args, parser, real)
    t1 = time.time()
    rep = retrieval.cross_modal_report(zd, zc, **retrieval.flag_settings(args))
    torch.cuda.synchronize()
    t2 = time.time()
    os.makedirs(args.log_path, exist_ok=True)
    retrieval.save(rep, args.log_path)
    if args.save_embeddings:
        torch.save(embeddings_record(zd, zc, args), os.path.join(args.log_path, EMBEDDINGS))
    for d in rep["directions"]:
        print(f"retrieval N={zd.shape[0]}: {retrieval.stats_line(rep[d], d)}", flush=True)
    print(f"retrieval N={zd.shape[0]}: embedded in {embed_s:.2f} s ({zd.shape[0] / max(embed_s, 1e-9):.0f} pairs/s), report in "
          f"{t2 - t1:.3f} s", flush=True)
    out = {"report": rep, "derm": zd, "clinic": zc}
    if args.against:
        other = load_embeddings(args.against)
        if tuple(other["derm"].shape[:1]) != (zd.shape[0],):
            raise SystemExit(f"backbone_retrieval: --against holds {other['derm'].shape[0]} cases, this run {zd.shape[0]}")
        rep_b = retrieval.cross_modal_report(other["derm"].to(zd.device), other["clinic"].to(zd.device),
                                             **retrieval.flag_settings(args))
        cmp = retrieval.compare(rep, rep_b)
        with open(os.path.join(args.log_path, "retrieval_compare.json"), "w") as f:
            json.dump(retrieval._plain(cmp), f, indent=1)
        for d in cmp["directions"]:
            parts = []
            for i, name in enumerate(cmp[d]["series"]):
                s = f"{name} {float(cmp[d]['delta'][i]):+.4f}"
                if "lo" in cmp[d]:
                    s += f" [{float(cmp[d]['lo'][i]):+.4f}, {float(cmp[d]['hi'][i]):+.4f}]"
                parts.append(s)
            print(f"retrieval difference to {args.against}: {d} " + " ".join(parts), flush=True)
        out["compare"] = cmp
    return out


if __name__ == "__main__":
    main()
