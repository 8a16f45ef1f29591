"""Label-free cross-modal retrieval report of an SSL checkpoint: given a case's dermoscopy embedding, does the clinical embedding
of the same case come back first among all held-out cases (and the other way round)?  Recall@k, mean / median rank, MRR with
case-resampling bootstrap intervals, and the held-out InfoNCE value -- the question the cross-modal term of the pre-training loss
(`cross_proj`, reference src/models/simclr.py:290-322,415-434) trains for, asked without labels.

Inputs: query, gallery [N, D] float32 GPU tensors, 1 <= N <= MAX_CASES, D >= 1, all finite (NaN / inf are refused on the host).
Row i of each belongs to case i: the positive of query i is gallery row i.

  * similarity: S = query . gallery^T from the exact-f32 gather-GEMM, as KNNBank.similarity produces it (D zero-padded to a
    multiple of 32, N to a multiple of 4); the queries are taken in chunks that keep S under max_s_bytes.  normalize=True (the
    default): both sides first go through sm3hip.knn.normalize.
  * beats: for j != i, b[i][j] = 1 iff S[i][j] > S[i][i], or S[i][j] == S[i][i] and j < i; b[i][i] = 0.  The lower index wins a
    tie (as in sm3_knn_vote): the order is total and nothing depends on the launch.  Packed: bits [N, W] (uint32 words held in an
    int32 tensor), W = ceil(N / 32), bit j & 31 of word j >> 5 holds b[i][j]; the bits of j >= N are 0.
  * rank: with integer case multiplicities m[n] >= 0, sum m = N: rho_i = sum_j m_j b[i][j], 0-based.  Copies of case i in the
    gallery count as its positive, not as competitors.  The point estimate has m = 1.
  * counts per replicate, all int64, for the levels ks = (k_1 .. k_L), 1 <= L <= 8, 1 <= k <= MAX_CASES:
        H_l = sum_i m_i [rho_i < k_l],  R = sum_i m_i rho_i,  Q = sum_i m_i floor(2^32 / (rho_i + 1)),
        M   = the least rho with 2 sum_i m_i [rho_i <= rho] >= N   (the lower weighted median);
    the record is (H_1 .. H_L, R, Q, M), L + 3 words.
  * values, fp64, on the host, ONE IEEE division each:
        R@k = H / N,  mean_rank = 1 + R / N,  MRR = Q / (N 2^32),  median_rank = M + 1.
    The Q32 rule of MRR (as the calibration report's): each case's 1 / (rho + 1) enters as floor(2^32 / (rho + 1)), below the
    exact reciprocal by less than 2^-32; both operands of the division are exactly represented (Q <= N 2^32 < 2^46), so the value
    is within 2^-32 of the exact mean reciprocal rank.
  * resampling and interval: the rule of resample.py.  With the same seed and the same N cases the intervals are joint with
    those of the evaluation, calibration and operating reports.  Nothing is ever undefined: every denominator is N.
  * point-only extras, fp64, no interval:
        loss(T) = mean_i [log sum_{j<N} exp(S_ij / T) - S_ii / T], S widened to fp64 before the division; the row terms come
        from the kernel in one fixed order and are added on the host in ascending i;  positive_similarity = mean_i S_ii, added
        the same way.  (A bootstrap of the loss would need a floating N x N sum per replicate: out of scope)
  * equal inputs give equal bits, whatever chunk, max_s_bytes, bootstrap size or launch geometry: a replicate is a function of
    (seed, r, N, bits) alone.

The kernels are sm3_retrieval_beats and sm3_retrieval_counts (csrc/retrieval.hip)."""
import numpy as np
import torch

from . import ops, report, resample
from .knn import _GEMM_MAX_BYTES, KNNBank, normalize as _normalize

MAX_CASES = ops.REPORT_MAX_CASES
MAX_LEVELS = ops.RETRIEVAL_MAX_LEVELS
DIRECTIONS = ("derm->clinic", "clinic->derm")
DEFAULT_CHUNK = report.DEFAULT_CHUNK
_TWO32 = float(2 ** 32)


def series_names(ks):
    return [f"R@{k}" for k in ks] + ["mean_rank", "median_rank", "MRR"]


def check_levels(ks, temperature, who="retrieval_report"):
    """The refusals of ks and the temperature; returns ks as a tuple."""
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"{who}: ks must be a sequence of integers, got {ks!r}") from None
    if not 1 <= len(ks) <= MAX_LEVELS:
        raise ValueError(f"{who}: 1 to {MAX_LEVELS} Recall@k levels, got {len(ks)}")
    for k in ks:
        if not resample.is_int(k) or not 1 <= k <= MAX_CASES:
            raise ValueError(f"{who}: every k must be an integer in [1, MAX_CASES = {MAX_CASES}], got {k!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0 < temperature < float("inf"):
        raise ValueError(f"{who}: temperature must be a positive finite number, got {temperature!r}")
    return ks


def check_inputs(query, gallery, who="retrieval_report"):
    """Types, shapes, the size limit, finiteness, then the device; returns (N, D)."""
    for t, name in ((query, "query"), (gallery, "gallery")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a 2-D float32 tensor [N, D]")
    if query.shape != gallery.shape:
        raise ValueError(f"{who}: query {tuple(query.shape)} and gallery {tuple(gallery.shape)} must be of the same cases and width")
    N, D = query.shape
    if N < 1 or D < 1:
        raise ValueError(f"{who}: no cases or no features ({N} x {D})")
    if N > MAX_CASES:
        raise ValueError(f"{who}: {N} cases, at most MAX_CASES = {MAX_CASES} are supported")
    for t, name in ((query, "query"), (gallery, "gallery")):
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{who}: {name} is not finite (a NaN has no rank)")
    if not (query.is_cuda and gallery.is_cuda) or query.device != gallery.device:
        raise ValueError(f"{who}: query and gallery must be tensors of one GPU (the SM3 HIP path has no CPU fallback)")
    return N, D


def values_from_counts(counts, N):
    """counts [..., L + 3] int64 (H_1 .. H_L, R, Q, M) of N cases -> values [..., L + 3] fp64 (R@k .., mean_rank, median_rank, MRR)."""
    counts = np.asarray(counts, dtype=np.int64)
    L = counts.shape[-1] - 3
    n = np.float64(N)
    out = np.empty(counts.shape, dtype=np.float64)
    out[..., :L] = counts[..., :L].astype(np.float64) / n
    out[..., L] = np.float64(1.0) + counts[..., L].astype(np.float64) / n
    out[..., L + 1] = (counts[..., L + 2] + 1).astype(np.float64)
    out[..., L + 2] = counts[..., L + 1].astype(np.float64) / np.float64(N * 2 ** 32)
    return out


def _ascending_sum(v):
    """v [N] fp64 added one at a time in ascending index."""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1])


def beats(query, gallery, temperature=0.1, max_s_bytes=1 << 30):
    """The kernel stage on prepared [N, D] float32 GPU tensors: (bits [N, W] int32, rank [N] int32 0-based, term [N] float64,
    diag [N] float32 = S_ii), all on the device.  The rows do not depend on the chunking."""
    N, D = query.shape
    dev = query.device
    bank = KNNBank(gallery, torch.zeros(N, dtype=torch.int32, device=dev), 1)  # its padding and column blocks; no targets are used
    W = (N + 31) // 32
    bits = torch.empty(N, W, dtype=torch.int32, device=dev)
    rank = torch.empty(N, dtype=torch.int32, device=dev)
    term = torch.empty(N, dtype=torch.float64, device=dev)
    diag = torch.empty(N, dtype=torch.float32, device=dev)
    rows = max(1, min(N, max_s_bytes // (4 * bank.ld), _GEMM_MAX_BYTES // (4 * bank.Dp)))
    S = torch.empty(rows, bank.ld, dtype=torch.float32, device=dev)
    for q0 in range(0, N, rows):
        q = query[q0:q0 + rows]
        n = q.shape[0]
        q = q.contiguous() if bank.Dp == D else torch.nn.functional.pad(q, (0, bank.Dp - D))
        Sc = S[:n]
        bank.similarity(q, Sc)
        ops.retrieval_beats(Sc, q0, N, temperature, bits[q0:q0 + n], rank[q0:q0 + n], term[q0:q0 + n])
        diag[q0:q0 + n] = Sc[:, q0:q0 + n].diagonal()
    return bits, rank, term, diag


def counts(bits, ks, bootstrap=0, seed=0, chunk=None):
    """(point [L + 3], replicates [B, L + 3] or None) int64 numpy, from the packed flags on the device."""
    (point,), (reps,) = resample.replicate_tables(
        lambda outs, seed, r0, point: ops.retrieval_counts(bits, ks, outs[0], seed, r0, point=point),
        [(len(ks) + 3,)], bootstrap, seed, chunk, DEFAULT_CHUNK, bits.device)
    return point, reps


def retrieval_report(query, gallery, ks=(1, 5, 10), temperature=0.1, normalize=True, bootstrap=0, confidence=0.95, seed=0,
                     chunk=None, max_s_bytes=1 << 30):
    """The report of one direction: query i looks for gallery i among the N gallery rows.

    Returns {"N", "ks", "temperature", "normalize", "series": R@k .., mean_rank, median_rank, MRR, "ranks" [N] int64 (1-based),
    "counts" [L + 3] int64, "values" [L + 3] fp64, "loss", "positive_similarity"} and, with bootstrap > 0, "replicates" [B, L + 3]
    fp64, "lo", "hi" [L + 3], "bootstrap", "seed", "confidence".  All tensors on the CPU; the inputs are not modified."""
    who = "retrieval_report"
    report.check_settings(bootstrap, confidence, seed, chunk, who)
    ks = check_levels(ks, temperature, who)
    if not resample.is_int(max_s_bytes) or max_s_bytes < 1:
        raise ValueError(f"{who}: max_s_bytes must be a positive integer, got {max_s_bytes!r}")
    N, _ = check_inputs(query, gallery, who)
    with torch.no_grad(), torch.cuda.device(query.device), ops.stream_scope():
        q, g = query.detach(), gallery.detach()
        if normalize:
            q, g = _normalize(q), _normalize(g)
        bits, rank, term, diag = beats(q, g, float(temperature), max_s_bytes)
        point, reps = counts(bits, ks, bootstrap, seed, chunk)
        rank, term, diag = rank.cpu(), term.cpu().numpy(), diag.cpu().numpy()
    out = {"N": N, "ks": list(ks), "temperature": float(temperature), "normalize": bool(normalize), "series": series_names(ks),
           "ranks": rank.long() + 1, "counts": torch.from_numpy(point), "values": torch.from_numpy(values_from_counts(point, N)),
           "loss": _ascending_sum(term) / N, "positive_similarity": _ascending_sum(diag) / N}
    if bootstrap:
        resample.pack_intervals(out, [("", values_from_counts(reps, N), None)], bootstrap, seed, confidence)
    return out


def cross_modal_report(derm_z, clinic_z, **settings):
    """Both directions of one set of paired embeddings: {"directions", "derm->clinic": retrieval_report(derm_z, clinic_z),
    "clinic->derm": retrieval_report(clinic_z, derm_z)}.  Each direction has its own S and bits; both share the seed, so replicate
    r of the two resamples the same cases."""
    return {"directions": list(DIRECTIONS), DIRECTIONS[0]: retrieval_report(derm_z, clinic_z, **settings),
            DIRECTIONS[1]: retrieval_report(clinic_z, derm_z, **settings)}


def _is_cross(rep):
    return isinstance(rep, dict) and "directions" in rep


def compare(a, b):
    """The paired difference of two reports of the SAME cases (equal N, ks, bootstrap, seed and confidence; ValueError otherwise),
    so replicate r of both resamples the same cases: {"delta": a.values - b.values, "series"} and, with a bootstrap, "lo", "hi" by
    the interval rule on a.replicates - b.replicates, "frac_le_zero", "bootstrap", "seed", "confidence".  Two cross-modal reports
    give {"directions", direction: comparison}."""
    if _is_cross(a) and _is_cross(b):
        return {"directions": list(DIRECTIONS), **{d: compare(a[d], b[d]) for d in DIRECTIONS}}
    resample.check_paired(a, b, "retrieval_report (or two from cross_modal_report)", ("values", "ks"),
                          (("N", "the number of cases differs ({} and {})"), ("ks", "ks differ ({} and {})")))
    return resample.paired_intervals({"delta": a["values"] - b["values"], "series": list(a["series"]),
                                      "loss_delta": a["loss"] - b["loss"]}, a, b)


def _plain(rep):
    """Everything but the replicates and the ranks, as lists."""
    return resample.plain(rep, ("replicates", "ranks"))


def to_json(rep, path):
    resample.write_json(rep, path, ("replicates", "ranks"))


def csv_rows(rep):
    """[(direction, series, value, lo, hi)]: the series, then loss and positive_similarity (no interval); repr of the fp64
    values, which parse back exactly."""
    rows = []
    for d in (rep["directions"] if _is_cross(rep) else [""]):
        r = rep[d] if d else rep
        for i, name in enumerate(r["series"]):
            rows.append((d, name, repr(float(r["values"][i])), repr(float(r["lo"][i])) if "lo" in r else "",
                         repr(float(r["hi"][i])) if "hi" in r else ""))
        for name in ("loss", "positive_similarity"):
            rows.append((d, name, repr(float(r[name])), "", ""))
    return rows


def to_csv(rep, path):
    with open(path, "w") as f:
        f.write("direction,series,value,lo,hi\n")
        for row in csv_rows(rep):
            f.write(",".join(row) + "\n")


def save(rep, log_path, stem="retrieval"):
    """<stem>.json and <stem>.csv under log_path."""
    resample.save(rep, log_path, stem, to_json, to_csv)


def stats_line(rep, name=""):
    """One direction in one line: R@k (with the interval when the report has one), the median rank, MRR and the loss."""
    parts = [name] if name else []
    L = len(rep["ks"])
    for i in list(range(L)) + [L + 2]:
        s = f"{rep['series'][i]} {float(rep['values'][i]):.4f}"
        if "lo" in rep:
            s += f" [{float(rep['lo'][i]):.4f}, {float(rep['hi'][i]):.4f}]"
        parts.append(s)
    parts.append(f"median {int(rep['values'][L + 1])}")
    parts.append(f"mean {float(rep['values'][L]):.2f}")
    parts.append(f"loss {rep['loss']:.4f}")
    return " ".join(parts)


def embed(model, derm, clinic):
    """The cross-modal projections (z_derm, z_clinic) [B, proj_dim] float32 of one batch of pairs, for a SimCLRSkinV3 / V32 on
    the GPU: the encoders and then cross_proj[0] / cross_proj[1] (v3: the shared cross_proj) on the model's own engine, all in
    eval mode whatever the modules' flags say -- every BatchNorm on its running statistics, one fused conv + scale / shift (+
    ReLU) launch per layer.  Each output row is a fixed-order function of its own image, so a case's embedding is the same bits
    whatever batch it arrives in (what tests/test_retrieval_gpu.py demands).  Parameters, running statistics and
    num_batches_tracked are read, never written."""
    from . import bridge
    kind = getattr(model, "_KIND", None)
    if kind not in ("v3", "v32"):
        raise ValueError("embed: the model must be a SimCLRSkinV3 or SimCLRSkinV32 (a model with cross-modal projectors)")
    for x, name in ((derm, "derm"), (clinic, "clinic")):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"embed: {name} must be a float32 GPU tensor [B, 3, H, W]")
    if derm.shape[0] != clinic.shape[0] or derm.shape[0] < 1:
        raise ValueError(f"embed: {derm.shape[0]} dermoscopy and {clinic.shape[0]} clinical images are not pairs")
    eng = bridge.sm3_engine_for(model, kind)
    B = derm.shape[0]
    out = []
    with torch.no_grad():
        for side, (branch, x) in enumerate((("derm", derm), ("clinic", clinic))):
            f32, _ = eng.encoder_only(branch, x.contiguous(), False, False)
            if eng.tdt == torch.float32:
                ft = f32
            else:
                ft = torch.empty(f32.shape, dtype=eng.tdt, device=f32.device)
                ops.cast_from_f32(eng.dtype, f32, ft)
            z = torch.empty(B, model.proj_dim, dtype=torch.float32, device=x.device)
            eng.projector_forward(eng.cross[side], ft, B, False, z)
            out.append(z)
    return out[0], out[1]


# ---- what the command-line tools share ----------------------------------------------------------------------------------
def add_flags(parser):
    """--retrieval-k / --retrieval-t and the bootstrap flags of the report family."""
    parser.add_argument("--retrieval-k", type=int, nargs="+", default=[1, 5, 10], help="the Recall@k levels (1 to 8 of them)")
    parser.add_argument("--retrieval-t", type=float, default=0.1, help="temperature of the held-out InfoNCE value")
    return resample.add_bootstrap_flags(parser)


def check_flags(args, who="backbone_retrieval"):
    """The refusals of the flags that argparse does not make, before any work is done."""
    try:
        check_levels(args.retrieval_k, args.retrieval_t, who)
        report.check_settings(args.bootstrap, args.confidence, args.bootstrap_seed, None, who)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def flag_settings(args):
    return dict(ks=tuple(args.retrieval_k), temperature=args.retrieval_t, bootstrap=args.bootstrap, confidence=args.confidence,
                seed=args.bootstrap_seed)
