"""Exact t-SNE maps of SSL embeddings: where the points of a checkpoint's embedding space lie relative to each other, in two
dimensions -- whether a case's dermoscopy and clinical projections land together, whether the diagnoses form islands before any
label was used.  The exact O(N^2) method (van der Maaten & Hinton 2008) with the schedule of scikit-learn's TSNE(method="exact"),
on kernels whose sums have an order that depends on N alone: the map is a function of (x, settings, seed), bit for bit.

Input: x [N, D] float32 on the GPU, 4 <= N <= MAX_POINTS, 1 <= D <= 4096, all finite.

  * squared distances: D2[i, j] = sum_k (x_ik - x_jk)^2 in fp32, fma-accumulated with k ascending; by differences, not by
    |x|^2 + |y|^2 - 2xy (L2-normalised projections are close, the norms would cancel).  D2 == D2.T in bits, the diagonal is 0.
  * conditional affinities, fp64, one row at a time: d'_j = D2[i, j] - min_{j != i} D2[i, j]; c_ij = exp(-beta_i d'_j) / S0.
    beta_i by the bisection of scikit-learn's _binary_search_perplexity from beta = 1, exactly 100 steps, no tolerance and no early
    exit, so beta does not depend on one.  c is stored as fp32, c_ii = 0.  A row whose other points are all at one distance is
    uniform, never NaN.
  * P = fp32((c + c.T in fp64) / (2 N)): symmetric in bits; zeros stay zeros, there is no epsilon clamp.
  * per iteration, for every point i (map y [N, 2] fp32): per pair in fp32 dx, dy, w = 1 / (1 + dx^2 + dy^2) (two fma, one IEEE
    division); in fp64 over j != i: Z_i = sum w, A_i = sum p_ij w (dx, dy), R_i = sum w^2 (dx, dy).  Then Z = sum_i Z_i,
    g_i = 4 (e A_i - R_i / Z) with e the exaggeration of this iteration (P itself is never rewritten), and scikit-learn's
    _gradient_descent rule in fp64 from the stored fp32 state, rounded once on store: gains + 0.2 where update g < 0, else x 0.8,
    at least 0.01; update = momentum update - lr gains g; y += update.
  * KL = sum_{p_ij > 0} p_ij (log p_ij - log w_ij + log Z), fp64, always with the true P; at the check iterations and at the end.
  * every sum above: term j goes to partial j mod 256 in ascending j, the 256 partials fold by a fixed halving tree.  No atomics.
  * schedule: exaggeration for the first exaggeration_iters iterations with momentum 0.5, then 1 and 0.8; learning_rate "auto" =
    max(N / exaggeration / 4, 50).  After the exaggeration phase, every check_every iterations: stop when the KL has not improved
    for more than `patience` iterations, or when the gradient norm is at most min_grad_norm.

The kernels are sm3_tsne_sqdist, _affinities, _symmetrise, _forces, _update and _kl (csrc/tsne.hip)."""
import numpy as np
import torch

from . import ops

MAX_POINTS = ops.TSNE_MAX_POINTS
MAX_DIM = ops.TSNE_MAX_DIM
INITS = ("random", "pca")
MODALITIES = ("derm", "clinic")


def check_inputs(x, perplexity, who="tsne"):
    """Type, shape, the size limits, finiteness, the perplexity, then the device; returns (N, D)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"{who}: x must be a 2-D float32 tensor [N, D]")
    N, D = x.shape
    if not 4 <= N <= MAX_POINTS:
        raise ValueError(f"{who}: {N} points, 4 to MAX_POINTS = {MAX_POINTS} are supported")
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"{who}: {D} features, 1 to {MAX_DIM} are supported")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{who}: x is not finite (a NaN has no distance)")
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float)) or not 1 <= perplexity <= (N - 1) / 3:
        raise ValueError(f"{who}: perplexity must be a number in [1, (N - 1) / 3 = {(N - 1) / 3:.4g}], got {perplexity!r}")
    if not x.is_cuda:
        raise ValueError(f"{who}: x must be a tensor of a GPU (the SM3 HIP path has no CPU fallback)")
    return N, D


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)


def check_settings(iters, exaggeration, exaggeration_iters, learning_rate, init, seed, check_every, min_grad_norm, patience,
                   who="tsne"):
    """The refusals of everything but x and the perplexity."""
    if not _is_int(iters) or iters < 1:
        raise ValueError(f"{who}: iters must be a positive integer, got {iters!r}")
    if not _is_num(exaggeration) or exaggeration < 1:
        raise ValueError(f"{who}: exaggeration must be a finite number of at least 1, got {exaggeration!r}")
    if not _is_int(exaggeration_iters) or exaggeration_iters < 0:
        raise ValueError(f"{who}: exaggeration_iters must be a non-negative integer, got {exaggeration_iters!r}")
    if learning_rate != "auto" and (not _is_num(learning_rate) or learning_rate <= 0):
        raise ValueError(f"{who}: learning_rate must be 'auto' or a positive finite number, got {learning_rate!r}")
    if isinstance(init, str) and init not in INITS:
        raise ValueError(f"{who}: init must be one of {', '.join(INITS)} or an [N, 2] array, got {init!r}")
    if not _is_int(seed) or not 0 <= seed < 2 ** 63:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^63), got {seed!r}")
    if not _is_int(check_every) or check_every < 1:
        raise ValueError(f"{who}: check_every must be a positive integer, got {check_every!r}")
    if not _is_num(min_grad_norm) or min_grad_norm < 0:
        raise ValueError(f"{who}: min_grad_norm must be a non-negative finite number, got {min_grad_norm!r}")
    if not _is_int(patience) or patience < 0:
        raise ValueError(f"{who}: patience must be a non-negative integer, got {patience!r}")


def pca_init(x):
    """x [N, D] -> [N, 2] fp32 on the CPU: the coordinates along the two leading principal axes (torch.linalg.eigh of the fp64
    covariance, on the CPU), each axis signed so that its largest-magnitude loading is positive, the whole scaled so that the first
    coordinate has standard deviation 1e-4.  The same bits only for one LAPACK build."""
    x = x.detach().to(device="cpu", dtype=torch.float64)
    N, D = x.shape
    if D < 2:
        raise ValueError("tsne: init='pca' needs at least two features")
    xc = x - x.mean(dim=0, keepdim=True)
    _, vec = torch.linalg.eigh(xc.T @ xc / (N - 1))
    axes = vec[:, [D - 1, D - 2]]
    lead = axes.abs().argmax(dim=0)
    axes = axes * torch.where(axes[lead, torch.arange(2)] < 0, -1.0, 1.0)
    y = xc @ axes
    std = float(y[:, 0].std(unbiased=False))
    return (y * (1e-4 / std if std > 0 else 0.0)).float()


def initial_map(x, init, seed, who="tsne"):
    """The first map [N, 2] fp32 on the CPU: "random" = 1e-4 randn of a CPU generator seeded with `seed` (the same values on every
    machine), "pca" = pca_init(x), or the given [N, 2] array."""
    N = x.shape[0]
    if isinstance(init, str):
        if init == "random":
            return 1e-4 * torch.randn(N, 2, generator=torch.Generator().manual_seed(seed))
        return pca_init(x)
    y = torch.as_tensor(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init), dtype=torch.float32)
    if tuple(y.shape) != (N, 2) or not bool(torch.isfinite(y).all()):
        raise ValueError(f"{who}: an initial map must be a finite [{N}, 2] array")
    return y.clone()


def _affinities(x, perplexity):
    N = x.shape[0]
    dev = x.device
    d2 = torch.empty(N, N, dtype=torch.float32, device=dev)
    ops.tsne_sqdist(x, d2)
    cond = torch.empty(N, N, dtype=torch.float32, device=dev)
    beta = torch.empty(N, dtype=torch.float64, device=dev)
    ops.tsne_affinities(d2, float(perplexity), cond, beta)
    P = torch.empty(N, N, dtype=torch.float32, device=dev)
    ops.tsne_symmetrise(cond, P)
    return P, beta, d2, cond


def affinities(x, perplexity=30.0):
    """{"P" [N, N] float32, "beta" [N] float64, "sqdist" [N, N] float32}, on the device of x."""
    check_inputs(x, perplexity, "affinities")
    with torch.no_grad(), torch.cuda.device(x.device), ops.stream_scope():
        P, beta, d2, _ = _affinities(x.detach().contiguous(), perplexity)
    return {"P": P, "beta": beta, "sqdist": d2}


def tsne(x, perplexity=30.0, iters=1000, exaggeration=12.0, exaggeration_iters=250, learning_rate="auto", init="random", seed=0,
         check_every=50, min_grad_norm=1e-7, patience=300, return_p=False):
    """The exact t-SNE map of x (see the module docstring for the arithmetic).

    Returns {"map" [N, 2] float32, "kl" (the fp64 value of the returned map), "history" [(iteration, kl, grad_norm)] of every
    check, "iters_run", "beta" [N] float64, "N", "D" and the settings ("learning_rate" resolved; "init" the name, or "array")} and,
    with return_p, "P" [N, N] float32 on the device; everything else on the CPU.  x is not modified.

    Equal inputs give equal bits, whatever ran before and whatever else is allocated.  For init="pca" that holds only for one
    LAPACK build: the principal axes come from torch.linalg.eigh on the CPU."""
    who = "tsne"
    N, D = check_inputs(x, perplexity, who)
    check_settings(iters, exaggeration, exaggeration_iters, learning_rate, init, seed, check_every, min_grad_norm, patience, who)
    y0 = initial_map(x, init, seed, who)
    lr = max(N / float(exaggeration) / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    dev = x.device
    with torch.no_grad(), torch.cuda.device(dev), ops.stream_scope():
        P, beta, d2, cond = _affinities(x.detach().contiguous(), perplexity)
        del d2, cond
        y = y0.to(dev).contiguous()
        upd = torch.zeros(N, 2, dtype=torch.float32, device=dev)
        gains = torch.ones(N, 2, dtype=torch.float32, device=dev)
        F = torch.empty(N, 5, dtype=torch.float64, device=dev)
        rows = torch.empty(N, dtype=torch.float64, device=dev)
        res = torch.empty(2, 2, dtype=torch.float64, device=dev)  # row 0: (KL, Z) of tsne_kl, row 1: (sum (gains g)^2, Z) of the step
        history, best, best_it, it = [], float("inf"), exaggeration_iters, -1
        for it in range(iters):
            early = it < exaggeration_iters
            ops.tsne_forces(P, y, F)
            check = (it + 1) % check_every == 0
            if check:
                ops.tsne_kl(P, y, F, rows, res[0])
            ops.tsne_update(F, exaggeration if early else 1.0, 0.5 if early else 0.8, lr, y, upd, gains, res[1])
            if check:
                r = res.cpu()
                err, gn = float(r[0, 0]), float(r[1, 0]) ** 0.5
                history.append((it, err, gn))
                if not early:
                    if err < best:
                        best, best_it = err, it
                    elif it - best_it > patience:
                        break
                    if gn <= min_grad_norm:
                        break
        ops.tsne_forces(P, y, F)
        ops.tsne_kl(P, y, F, rows, res[0])
        kl = float(res[0, 0].cpu())
        out = {"map": y.cpu(), "kl": kl, "history": history, "iters_run": it + 1, "beta": beta.cpu(), "N": N, "D": D,
               "perplexity": float(perplexity), "iters": iters, "exaggeration": float(exaggeration),
               "exaggeration_iters": exaggeration_iters, "learning_rate": lr, "init": init if isinstance(init, str) else "array",
               "seed": seed, "check_every": check_every, "min_grad_norm": float(min_grad_norm), "patience": patience}
        if return_p:
            out["P"] = P
    return out


def _dist64(a):
    a = a.double()
    return torch.cdist(a, a, compute_mode="donot_use_mm_for_euclid_dist")


def _neighbours(d, k):
    """The k nearest other points of every row of the distance matrix d, ties by the lower index."""
    d = d.clone()
    d.fill_diagonal_(float("inf"))
    return torch.sort(d, dim=1, stable=True).indices[:, :k]


def preservation(x, y, k=10):
    """The share of each point's k nearest neighbours in x [N, D] that are among its k nearest neighbours in the map y [N, 2],
    averaged over the points (Euclidean distances in fp64, ties by the lower index).  Plain torch, on the device of x."""
    x, y = torch.as_tensor(x), torch.as_tensor(y).to(torch.as_tensor(x).device)
    N = x.shape[0]
    if y.shape[0] != N or not _is_int(k) or not 1 <= k <= N - 1:
        raise ValueError(f"preservation: x and y must have the same N rows and 1 <= k <= N - 1, got {x.shape[0]}, {y.shape[0]}, {k!r}")
    nx, ny = _neighbours(_dist64(x), k), _neighbours(_dist64(y), k)
    member = torch.zeros(N, N, dtype=torch.bool, device=x.device)
    member.scatter_(1, nx, True)
    return float(member.gather(1, ny).double().sum(dim=1).div(k).mean())


def partner_ranks(derm_map, clinic_map):
    """[N, 2] int64: for case n, the 1-based rank of its clinical point among all other 2N - 1 points by map distance from its
    dermoscopy point (column 0), and the other way round (column 1); ties by the lower index in the stacked order."""
    y = torch.cat([torch.as_tensor(derm_map), torch.as_tensor(clinic_map)]).double()
    N = y.shape[0] // 2
    d = _dist64(y)
    idx = torch.arange(2 * N, device=y.device)
    partner = torch.cat([idx[N:], idx[:N]])
    dp = d[idx, partner][:, None]
    before = (d < dp) | ((d == dp) & (idx[None, :] < partner[:, None]))
    before[idx, idx] = False
    before[idx, partner] = False
    rank = before.sum(dim=1) + 1
    return torch.stack([rank[:N], rank[N:]], dim=1).cpu()


def cross_modal_map(derm_z, clinic_z, k=10, **settings):
    """One map of the 2N stacked points (the N dermoscopy embeddings first): {"derm" [N, 2], "clinic" [N, 2], "partner_rank"
    [N, 2] int64 (partner_ranks), "median_partner_rank", "preservation" (of the k nearest neighbours, k = 10), "k", "tsne": the
    report of tsne() on the stacked points}."""
    who = "cross_modal_map"
    for t, name in ((derm_z, "derm_z"), (clinic_z, "clinic_z")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a 2-D float32 tensor [N, D]")
    if derm_z.shape != clinic_z.shape:
        raise ValueError(f"{who}: derm_z {tuple(derm_z.shape)} and clinic_z {tuple(clinic_z.shape)} must be of the same cases and width")
    if derm_z.device != clinic_z.device:
        raise ValueError(f"{who}: derm_z and clinic_z must be tensors of one GPU (the SM3 HIP path has no CPU fallback)")
    N = derm_z.shape[0]
    x = torch.cat([derm_z.detach(), clinic_z.detach()])
    rep = tsne(x, **settings)
    y = rep["map"]
    ranks = partner_ranks(y[:N].to(x.device), y[N:].to(x.device))
    return {"derm": y[:N].clone(), "clinic": y[N:].clone(), "partner_rank": ranks,
            "median_partner_rank": float(ranks.double().median()), "k": k,
            "preservation": preservation(x, y.to(x.device), min(k, 2 * N - 1)), "tsne": rep}


# ---- drawing ------------------------------------------------------------------------------------------------------------
PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
           (127, 127, 127))
BACKGROUND = (255, 255, 255)
LINE = (200, 200, 200)


def pixel_coords(map, size=1024):
    """[N, 2] int64 (column, row) of every point in a size x size picture: one scale for both axes, the map's bounding box centred
    inside a margin of size // 32 pixels, +y upwards."""
    y = np.asarray(map.detach().cpu() if isinstance(map, torch.Tensor) else map, dtype=np.float64)
    if y.ndim != 2 or y.shape[1] != 2 or not np.isfinite(y).all():
        raise ValueError("render: map must be a finite [N, 2] array")
    if not _is_int(size) or not 16 <= size <= 16384:
        raise ValueError(f"render: size must be an integer in [16, 16384], got {size!r}")
    margin = size // 32
    lo, hi = y.min(axis=0), y.max(axis=0)
    span = float((hi - lo).max())
    room = size - 1 - 2 * margin
    scale = room / span if span > 0 else 0.0
    off = margin + (room - (hi - lo) * scale) / 2.0
    px = np.rint(off + (y - lo) * scale).astype(np.int64)
    px[:, 1] = size - 1 - px[:, 1]
    return px


def point_radius(size):
    return max(1, size // 256)


def render(map, colours, path, size=1024, pair_lines=None):
    """Writes a size x size RGB PNG of the map to `path` (PIL): white background, point n a filled square of side
    2 point_radius(size) + 1 in colours[n] (an [N, 3] array of 0..255) centred on pixel_coords(map, size)[n]; the points are drawn
    in index order, so a later point covers an earlier one.  pair_lines: an [M, 2] array of point indices, each pair joined by
    a grey line under the points.  Returns the pixel coordinates."""
    from PIL import Image, ImageDraw
    px = pixel_coords(map, size)
    N = px.shape[0]
    col = np.asarray(colours.cpu() if isinstance(colours, torch.Tensor) else colours)
    if col.shape != (N, 3) or col.min() < 0 or col.max() > 255:
        raise ValueError(f"render: colours must be an [{N}, 3] array of values in 0 .. 255")
    col = col.astype(np.uint8)
    im = Image.new("RGB", (size, size), BACKGROUND)
    draw = ImageDraw.Draw(im)
    if pair_lines is not None:
        pairs = np.asarray(pair_lines, dtype=np.int64).reshape(-1, 2)
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= N):
            raise ValueError(f"render: pair_lines must index the {N} points")
        for a, b in pairs:
            draw.line([tuple(int(v) for v in px[a]), tuple(int(v) for v in px[b])], fill=LINE, width=1)
    r = point_radius(size)
    for n in range(N):
        cx, cy = int(px[n, 0]), int(px[n, 1])
        draw.rectangle([cx - r, cy - r, cx + r, cy + r], fill=tuple(int(v) for v in col[n]))
    im.save(path, format="PNG")
    return px


def class_colours(classes):
    """[N, 3] uint8: PALETTE[c % 8] for every class index."""
    return np.asarray(PALETTE, dtype=np.uint8)[np.asarray(classes, dtype=np.int64) % len(PALETTE)]


# ---- what the command-line tools share ----------------------------------------------------------------------------------
def add_flags(parser):
    parser.add_argument("--perplexity", type=float, default=30.0, help="t-SNE perplexity, in [1, (points - 1) / 3]")
    parser.add_argument("--map-iters", type=int, default=1000, help="t-SNE iterations")
    parser.add_argument("--map-init", default="random", choices=list(INITS), help="the first map")
    parser.add_argument("--map-seed", type=int, default=0, help="seed of the random first map")
    return parser


def check_flags(args, points, who="backbone_map"):
    """The refusals of the flags that argparse does not make, for a map of `points` points, before any work is done."""
    try:
        if not 4 <= points <= MAX_POINTS:
            raise ValueError(f"{who}: {points} points, 4 to MAX_POINTS = {MAX_POINTS} are supported")
        if not 1 <= args.perplexity <= (points - 1) / 3:
            raise ValueError(f"{who}: --perplexity must lie in [1, (points - 1) / 3 = {(points - 1) / 3:.4g}], got {args.perplexity!r}")
        check_settings(args.map_iters, 12.0, 250, "auto", args.map_init, args.map_seed, 50, 1e-7, 300, who)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def flag_settings(args):
    return dict(perplexity=args.perplexity, iters=args.map_iters, init=args.map_init, seed=args.map_seed)
