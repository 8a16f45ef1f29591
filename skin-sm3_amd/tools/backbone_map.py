"""Exact t-SNE map of an SSL checkpoint's cross-modal embeddings on MI355X: the held-out cases' dermoscopy and clinical projections
in one 2-D picture -- do the two images of a case land together, do the diagnoses form islands before any label was used
(sm3hip/tsne.py).  The map is a function of (embeddings, settings, seed), bit for bit.

    python tools/backbone_map.py <backbone_retrieval's line> --log-path logs/backbone/map_399 --perplexity 30 --colour-by DIAG
    python tools/backbone_map.py --data-name synthetic --data-path - --embeddings logs/backbone/retrieval_399/retrieval_embeddings.pt \
        --log-path logs/backbone/map_399 --pair-lines

Takes backbone_retrieval's line (its model, data and checkpoint flags; its report flags are accepted and unused) and embeds the
held-out pairs as it does; with --embeddings path/retrieval_embeddings.pt (backbone_retrieval --save-embeddings) no model is
built.  Writes to --log-path: map.csv (case, modality, x, y and the eight derm7pt labels where known; repr of the fp32
coordinates, which parse back exactly), map.json (settings, history, final KL, preservation of the 10 nearest neighbours, median
partner rank) and map.png (--colour-by modality, or one of the derm7pt labels with real data; --pair-lines joins the two points
of each case).
"""
import json
import os
import sys

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
for _p in (ROOT_PATH, SCRIPT_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402

import backbone_retrieval  # noqa: E402
from sm3hip import tsne  # noqa: E402
from src.utils.data.datasets import LABEL_ORD  # noqa: E402

WHO = "backbone_map"
MAX_CASES = tsne.MAX_POINTS // 2


def get_parser():
    p = backbone_retrieval.get_parser()
    p.description = "SM3 exact t-SNE map of the cross-modal embeddings (MI355X)"
    tsne.add_flags(p)
    p.add_argument("--embeddings", default=None, type=str,
                   help=f"a {backbone_retrieval.EMBEDDINGS} of backbone_retrieval --save-embeddings: map it, build no model")
    p.add_argument("--colour-by", default="modality", choices=["modality"] + LABEL_ORD,
                   help="what the colours of map.png show (a label needs real data)")
    p.add_argument("--pair-lines", action="store_true", help="join the two points of every case in map.png")
    return p


def write_csv(path, derm, clinic, labels):
    with open(path, "w") as f:
        f.write(",".join(["case", "modality", "x", "y"] + LABEL_ORD) + "\n")
        for m, y in zip(tsne.MODALITIES, (derm, clinic)):
            for n in range(y.shape[0]):
                lab = [""] * len(LABEL_ORD) if labels is None else [str(int(v)) for v in labels[n]]
                f.write(",".join([str(n), m, repr(float(y[n, 0])), repr(float(y[n, 1]))] + lab) + "\n")


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    from src.utils.misc import require_data
    real = require_data(args, WHO)
    if args.colour_by != "modality" and not real:
        raise SystemExit(f"{WHO}: --colour-by {args.colour_by} needs the labels of a real dataset (--data-name SevenPCBaseDataset)")
    emb = None
    if args.embeddings:
        if not os.path.isfile(args.embeddings):
            raise SystemExit(f"{WHO}: --embeddings {args.embeddings} does not exist")
        emb = backbone_retrieval.load_embeddings(args.embeddings)
        N = int(emb["derm"].shape[0])
        if not 2 <= N <= MAX_CASES:
            raise SystemExit(f"{WHO}: {N} cases in --embeddings, 2 to {MAX_CASES} are supported")
    else:
        backbone_retrieval.check_checkpoint(args, real, WHO)
        N = backbone_retrieval.count_cases(args, real, WHO, least=2, most=MAX_CASES)
    tsne.check_flags(args, 2 * N, WHO)
    labels = None
    if emb is not None and real:
        from src.utils.data.datasets import read_split
        labels = read_split(args.data_path, "test")[2]
        if len(labels) != N:
            raise SystemExit(f"{WHO}: --embeddings holds {N} cases, the test split of --data-path {len(labels)}")
    # ---- the device, from here on
    if emb is None:
        zd, zc, labels, _ = backbone_retrieval.embed_held_out(args, parser, real)
    else:
        dev = torch.device("cuda", 0)
        zd, zc = emb["derm"].float().to(dev), emb["clinic"].float().to(dev)
    rep = tsne.cross_modal_map(zd, zc, **tsne.flag_settings(args))
    torch.cuda.synchronize()
    os.makedirs(args.log_path, exist_ok=True)
    derm, clinic = rep["derm"].numpy(), rep["clinic"].numpy()
    write_csv(os.path.join(args.log_path, "map.csv"), derm, clinic, labels)
    t = rep["tsne"]
    summary = {k: t[k] for k in ("N", "D", "perplexity", "iters", "exaggeration", "exaggeration_iters", "learning_rate", "init",
                                 "seed", "check_every", "min_grad_norm", "patience", "iters_run", "kl")}
    summary.update(cases=N, history=[list(h) for h in t["history"]], preservation=rep["preservation"], k=rep["k"],
                   median_partner_rank=rep["median_partner_rank"], colour_by=args.colour_by,
                   embeddings=args.embeddings, pretrain_path=args.pretrain_path)
    with open(os.path.join(args.log_path, "map.json"), "w") as f:
        json.dump(summary, f, indent=1)
    if args.colour_by == "modality":
        classes = np.repeat(np.arange(2), N)
    else:
        classes = np.tile(np.asarray(labels)[:, LABEL_ORD.index(args.colour_by)], 2)
    pairs = np.stack([np.arange(N), np.arange(N) + N], axis=1) if args.pair_lines else None
    tsne.render(np.concatenate([derm, clinic]), tsne.class_colours(classes), os.path.join(args.log_path, "map.png"),
                pair_lines=pairs)
    print(f"map N={N} cases ({2 * N} points): KL {t['kl']:.4f} after {t['iters_run']} iterations, preservation@{rep['k']} "
          f"{rep['preservation']:.4f}, median partner rank {rep['median_partner_rank']:.0f} of {2 * N - 1}", flush=True)
    if args.save_embeddings and emb is None:
        torch.save(backbone_retrieval.embeddings_record(zd, zc, args), os.path.join(args.log_path, backbone_retrieval.EMBEDDINGS))
    return {"map": rep, "derm": zd, "clinic": zc, "labels": labels}


if __name__ == "__main__":
    main()
