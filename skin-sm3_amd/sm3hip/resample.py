"""What the case-resampling bootstrap reports share: report.py (evaluation), calibration.py, operating.py, retrieval.py,
checklist.py, conformal.py, selective.py.

THE RESAMPLING RULE (csrc/resample.h states it for the device, DESIGN.md 8.10 in prose; the five modules point here).  Integer
case multiplicities m[n] >= 0 with sum m = N weigh every count of a report; the point estimate has m = 1.  Replicate r makes N
draws: draw d (0 <= d < N) is word d % 4 of Philox4x32-10 (csrc/exact_f32.h) with key = the 64-bit seed (low word first) and
counter (d / 4, r, 0, 2) -- the last word keeps the stream apart from SmoothGrad's 0 and RISE's 1; it hits case (w * N) >> 32 in
64-bit integers; m_r[i] = the number of draws that hit case i.  m_r is a function of (seed, r, N) alone: not of B, the chunk,
the launch geometry or the report.  So with one seed replicate r resamples the same cases in all five reports -- their intervals
are joint -- and in two reports of the same cases, which makes `compare` paired at no cost.

Interval: per series the B replicate values sorted ascending, lo = v[i], hi = v[B - 1 - i], i = floor((B - 1) * (1 - confidence)
/ 2) in float64.  A replicate whose denominator was 0 has the value 0, stays in the order statistic and is counted in
`undefined`.  Values are ONE IEEE fp64 division of two integers each (safe_div).

Everything here is host-side and small; nothing touches torch.cuda but device_for."""
import json
import os

import numpy as np
import torch

MAX_BOOTSTRAP = 2 ** 24


# ---- settings and intervals ---------------------------------------------------------------------------------------------------
def is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_settings(bootstrap, confidence, seed, chunk, who="evaluation_report"):
    """The refusals that need neither a tensor nor a device."""
    if not is_int(bootstrap) or not 0 <= bootstrap <= MAX_BOOTSTRAP:
        raise ValueError(f"{who}: bootstrap must be an integer in [0, 2^24], got {bootstrap!r}")
    if isinstance(confidence, bool) or not isinstance(confidence, (int, float)) or not 0 < confidence < 1:
        raise ValueError(f"{who}: confidence must be a number with 0 < confidence < 1, got {confidence!r}")
    if not is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    if chunk is not None and (not is_int(chunk) or not 1 <= chunk <= max(bootstrap, 1)):
        raise ValueError(f"{who}: chunk must be None or an integer in [1, {max(bootstrap, 1)}], got {chunk!r}")


def interval_index(B, confidence):
    """i of lo = v[i], hi = v[B - 1 - i] over the B sorted replicate values: floor((B - 1) * (1 - confidence) / 2) in float64."""
    return int(np.floor(np.float64(B - 1) * (np.float64(1.0) - np.float64(confidence)) / np.float64(2.0)))


def interval(replicates, confidence):
    """replicates [B, ...] fp64 -> (lo, hi) [...] by the order-statistic rule."""
    v = np.sort(np.asarray(replicates, dtype=np.float64), axis=0)
    B = v.shape[0]
    i = interval_index(B, confidence)
    return v[i], v[B - 1 - i]


def safe_div(num, den):
    """(num / den in fp64, 0 where den == 0; den == 0): ONE division of two exactly represented integers.  num and den
    broadcast."""
    num, den = np.broadcast_arrays(np.asarray(num).astype(np.float64), np.asarray(den).astype(np.float64))
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out, den == 0


# ---- the Philox stream on the host ---------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC 2011; csrc/exact_f32.h on the device) on uint64 arrays holding 32-bit words -> the four
    output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def philox_words(n, seed, r, stream):
    """n 32-bit words (uint64 array): word d is word d % 4 of the call with key = the 64-bit seed (low word first) and counter
    (d / 4, r, 0, stream).  Streams in use: 0 SmoothGrad, 1 RISE, 2 the bootstrap draws above, 3 and 4 sm3hip/logreg.py,
    5 the swap bits of sm3hip/significance.py, 6 the bootstrap draws of the calibration split of sm3hip/conformal.py (the rule
    above on N_cal cases), 7 the case and element words of sm3hip/corrupt.py (its own counters: see that module's text)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(q, np.uint64(r), np.uint64(0), np.uint64(stream), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1).reshape(-1)[:n]


# ---- the device and the replicate loop ----------------------------------------------------------------------------------------
def device_for(preds, who):
    """The device a report of `preds` runs on: that of preds[0] if it is a GPU's, else the current GPU."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: needs a GPU (the SM3 HIP path has no CPU fallback)")
    return preds[0].device if preds[0].is_cuda else torch.device("cuda", torch.cuda.current_device())


def replicate_tables(launch, shapes, bootstrap, seed, chunk, default_chunk, device):
    """The point tables and the replicate tables of a report.  launch(outs, seed, r0, point) fills outs, one int64 tensor [c, *shape]
    per entry of `shapes`, for the replicates r0 .. r0 + c - 1, or (point, c = 1) for the point estimate.  One point call, then
    the B = bootstrap replicates `chunk` at a time (None: at most default_chunk), the last chunk short; a replicate does not
    depend on the chunk.  Returns (points, replicates): numpy int64 arrays [*shape] and [B, *shape] (None without a bootstrap)."""
    point = [torch.empty((1,) + tuple(s), dtype=torch.int64, device=device) for s in shapes]
    launch(point, seed, 0, True)
    reps = [None] * len(point)
    if bootstrap:
        c = min(bootstrap, default_chunk) if chunk is None else chunk
        reps = [torch.empty((bootstrap,) + tuple(s), dtype=torch.int64, device=device) for s in shapes]
        for r0 in range(0, bootstrap, c):
            launch([t[r0:r0 + min(c, bootstrap - r0)] for t in reps], seed, r0, False)
        reps = [t.cpu().numpy() for t in reps]
    return [t[0].cpu().numpy() for t in point], reps


def pack_intervals(out, tables, bootstrap, seed, confidence):
    """Adds a bootstrap's keys to the report dict `out`, in the order the files are written in: per (prefix, replicates [B, ...]
    fp64, undefined counts [...] or None) of `tables` "<prefix>replicates", "<prefix>lo", "<prefix>hi" and "<prefix>undefined"
    (int64; left out for None); then "bootstrap", "seed", "confidence"."""
    for prefix, replicates, undefined in tables:
        lo, hi = interval(replicates, confidence)
        out[prefix + "replicates"] = torch.from_numpy(replicates)
        out[prefix + "lo"], out[prefix + "hi"] = torch.from_numpy(lo.copy()), torch.from_numpy(hi.copy())
        if undefined is not None:
            out[prefix + "undefined"] = torch.from_numpy(np.asarray(undefined).astype(np.int64))
    out.update({"bootstrap": bootstrap, "seed": seed, "confidence": float(confidence)})
    return out


def check_paired(a, b, source, required, same=()):
    """The refusals of a paired comparison of the reports a and b, in this order: anything but two dicts with the `required` keys
    (from `source`), different cases ("targets", when required), a difference in one of the module's own keys `same` = ((key,
    message with {} {} for the two values), ...), then in bootstrap, seed, confidence."""
    for r in (a, b):
        if not isinstance(r, dict) or any(k not in r for k in required):
            raise ValueError(f"compare: two dicts from {source} are needed")
    if "targets" in required and (tuple(a["targets"].shape) != tuple(b["targets"].shape)
                                  or not bool(torch.equal(a["targets"], b["targets"]))):
        raise ValueError("compare: the two reports must be of the same cases (equal targets)")
    for key, message in same:
        if a.get(key) != b.get(key):
            raise ValueError("compare: " + message.format(a.get(key), b.get(key)))
    if a.get("bootstrap", 0) != b.get("bootstrap", 0):
        raise ValueError(f"compare: bootstrap differs ({a.get('bootstrap', 0)} and {b.get('bootstrap', 0)})")
    if a.get("seed") != b.get("seed"):
        raise ValueError(f"compare: seed differs ({a.get('seed')} and {b.get('seed')}): the replicates would not be paired")
    if a.get("confidence") != b.get("confidence"):
        raise ValueError(f"compare: confidence differs ({a.get('confidence')} and {b.get('confidence')})")


def paired_intervals(out, a, b, prefixes=("",)):
    """What a bootstrap adds to the comparison `out` of the checked reports a and b: per prefix "<prefix>lo", "<prefix>hi" by the
    interval rule on a's replicates minus b's and "<prefix>frac_le_zero" = the fraction of replicates with a difference <= 0,
    then "bootstrap", "seed", "confidence"."""
    if a.get("bootstrap", 0):
        for p in prefixes:
            d = (a[p + "replicates"] - b[p + "replicates"]).numpy()
            lo, hi = interval(d, a["confidence"])
            out.update({p + "lo": torch.from_numpy(lo.copy()), p + "hi": torch.from_numpy(hi.copy()),
                        p + "frac_le_zero": torch.from_numpy((d <= 0).sum(axis=0) / float(d.shape[0]))})
        out.update({"bootstrap": a["bootstrap"], "seed": a["seed"], "confidence": a["confidence"]})
    return out


# ---- writers and flags --------------------------------------------------------------------------------------------------------
def plain(v, skip=()):
    """v with every tensor as a list, without the keys `skip` of any dict in it."""
    if isinstance(v, torch.Tensor):
        return v.tolist()
    if isinstance(v, dict):
        return {k: plain(x, skip) for k, x in v.items() if k not in skip}
    if isinstance(v, (list, tuple)):
        return [plain(x, skip) for x in v]
    return v


def write_json(rep, path, skip=()):
    """plain(rep, skip) as JSON (json writes repr of a float: the values parse back exactly; inf is written as Infinity)."""
    with open(path, "w") as f:
        json.dump(plain(rep, skip), f, indent=1)


def write_long_csv(path, header, rows):
    """The long format: `header`, then a line per row; repr of the fp64 values (they parse back exactly), str of the rest."""
    with open(path, "w") as f:
        f.write(header + "\n")
        for row in rows:
            f.write(",".join(repr(v) if isinstance(v, float) else str(v) for v in row) + "\n")


def save(rep, log_path, stem, to_json, to_csv):
    """<stem>.json and <stem>.csv under log_path, by the module's two writers."""
    os.makedirs(log_path, exist_ok=True)
    to_json(rep, os.path.join(log_path, stem + ".json"))
    to_csv(rep, os.path.join(log_path, stem + ".csv"))


def add_bootstrap_flags(parser, of=""):
    """--bootstrap / --bootstrap-seed / --confidence of every tool of the report family."""
    parser.add_argument("--bootstrap", type=int, default=0,
                        help=f"case-resampling bootstrap replicates{of} (0: point estimate only)")
    parser.add_argument("--bootstrap-seed", type=int, default=0, help="64-bit seed of the bootstrap replicates")
    parser.add_argument("--confidence", type=float, default=0.95, help="confidence of the bootstrap intervals")
    return parser
