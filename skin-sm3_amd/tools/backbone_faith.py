"""Deletion / insertion faithfulness curves of a linear probe's attribution maps on MI355X: does each of the 8 derm7pt label
predictions fall when the pixels a map calls important are taken away, and rise when only they are shown (sm3hip/faith.py)?

    python tools/backbone_faith.py -a resnet50 --data-name SevenPCBaseDataset --data-path ./data/7PC \
        --mean 0.7833 0.6712 0.6026 --std 0.2139 0.2472 0.2571 -b 8 -j 4 --img-sz 224 224 \
        --linear-path logs/eval/best_linear.pth --log-path logs/eval/faith --method ig --steps 32 --curve-steps 32 --max-cases 64

    python tools/backbone_faith.py ... --method rise --rise-masks 4000 --rise-cells 7 --rise-p 0.5 --curve-steps 32

Takes tools/backbone_cam.py's and tools/backbone_attr.py's command lines with --method cam|ig|smoothgrad|random|rise (and that
method's own flags: --cam-layer; --steps / --samples / --sigma / --squared / --attr-seed; --rise-masks / --rise-cells /
--rise-p), --curve-steps, --curve-mode
both|deletion|insertion, --modality joint|derm|clinic and --chunk (curve steps per encoder forward).  random ranks a uniform
random map seeded by --attr-seed: the control a faithfulness table needs.  rise makes the black-box maps of sm3hip/rise.py
(masks seeded by --attr-seed, the curves' baseline and --modality, the planned chunk) and also writes them: maps [n, 8, 2, H, W]
fp16.  The maps are computed with the chosen method on the
engine, then ranked and scored; the baseline is zero in normalised space (the dataset-mean image).  faith.pt goes to --log-path:
deletion / insertion [n, 8, curve-steps + 1] fp64, deletion_auc / insertion_auc [n, 8] fp64, logits and baseline_logits (8
tensors [n, classes]), targets [n, 8], target_class [n, 8], indices [n], method, labels.  A low deletion AUC and a high insertion
AUC say that the map is faithful.
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

import explain_cli as cli  # noqa: E402
from sm3hip import attr, cam, faith, rise  # noqa: E402
from sm3hip.metrics import CLASSES_NAME, NUM_CLASSES  # noqa: E402


def get_parser():
    return cli.add_faith_args(cli.backbone_parser(
        "SM3 deletion / insertion faithfulness curves of a linear probe's attribution maps (MI355X)"))


def make_maps(model, derm, clinic, args, gen):
    """(maps [N, 8, 2, H, W] fp32 on the images' device, target for the curves) by --method; gen: the CPU generator of random."""
    if args.method == "random":
        N, _, H, W = derm.shape
        return torch.rand(N, len(NUM_CLASSES), 2, H, W, generator=gen).to(derm.device), args.target
    if args.method == "cam":
        out = cam.grad_cam(model, derm, clinic, layer=args.cam_layer, target=args.target)
    elif args.method == "ig":
        out = attr.integrated_gradients(model, derm, clinic, target=args.target, steps=args.steps)
    elif args.method == "rise":
        out = rise.rise(model, derm, clinic, target=args.target, masks=args.rise_masks, cells=args.rise_cells, p=args.rise_p,
                        seed=args.attr_seed, modality=args.modality)
    else:
        out = attr.smooth_grad(model, derm, clinic, target=args.target, samples=args.samples, sigma=args.sigma,
                               squared=args.squared, seed=args.attr_seed)
    return out["maps"], out["target_class"]  # the curves follow the classes the maps explain


def run(args, parser, tool, mlc):
    """Maps, then curves, batch by batch; the report of the mean AUCs."""
    gens = []  # the CPU generator of --method random: made at the first batch, after every refusal

    def per_batch(model, derm, clinic, lab, args):
        if not gens:
            gens.append(torch.Generator().manual_seed(args.attr_seed))
        maps, target = make_maps(model, derm, clinic, args, gens[0])
        out = faith.deletion_insertion(model, derm, clinic, maps, target=target, steps=args.curve_steps, modality=args.modality,
                                       mode=args.curve_mode, chunk=args.chunk)
        curves = [n for n in ("deletion", "insertion") if args.curve_mode in ("both", n)]
        got = {k: out[k] for k in curves + [n + "_auc" for n in curves]}
        got.update(targets=lab, target_class=out["target_class"], logits=out["logits"], baseline_logits=out["baseline_logits"])
        if args.method == "rise":
            got["maps"] = maps.half()
        return got

    saved, stat = cli.explain(args, parser, tool, mlc, per_batch, "faith.pt",
                              check=lambda a, t: cli.check_faith_args(a, t, cli.image_size(a, mlc)), target=args.target,
                              method=args.method, modality=args.modality, curve_steps=args.curve_steps)
    print(f"{tool} ({args.method}, {args.target}, {args.modality}, {args.curve_steps} curve steps): {stat['cases']} cases x "
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
    return run(parser.parse_args(argv), parser, "backbone_faith", False)


if __name__ == "__main__":
    main()
