"""Pixel-level attributions of the linear probe (src/models/baseline.py `Baseline`) and of the SM3 multi-label model
(inference.py `Model`) on the HIP engine: Integrated Gradients (Sundararajan et al., ICML 2017) and SmoothGrad (Smilkov et
al., 2017), one attribution per derm7pt label, image modality and pixel.

    IG_t(x)  = (x - b) * 1/S sum_k  d logit_t / dx (b + alpha_k (x - b)),  alpha_k = (k + 1/2) / S   (midpoint rule)
    SG_t(x)  =           1/S sum_k f(d logit_t / dx (x + sigma (max x - min x) z_k)),  z_k ~ N(0, 1),  f = identity or square

The path (IG) is joint over the two images of a pair: both move from their baselines to the images with the same alpha, and
the heads see the features of the same path point.  The targets are chosen once, at x.  Per chunk of c path points (noise
samples) and modality: sm3_attr_path / sm3_attr_noise build the [c * N, 3, H, W] inputs, ONE encoder forward keeps the records
of all of them, the heads give the 8 per-label seeds d logit_t / d feats (explain.Subject.head_grads), and 8 data-only backward
passes (engine.encoder_backward(dx_out=, params=False)) from the shared forward each end in sm3_attr_accumulate, which adds the c
gradients of every image into acc[t, modality] in ascending step order -- so the bits do not depend on the chunk.
sm3_attr_finish multiplies by (x - b) (IG), sums |.| over the channels for the maps and adds the attributions of every
(label, image) in float64 by a fixed tree: with the logits that gives IG's completeness gap
delta = sum(attributions) - (logit_t(x) - logit_t(b)), the quadrature error of the rule at S steps.

Everything runs under torch.no_grad: parameters, .grad fields, BatchNorm buffers and the engines' flat gradient buffers are left
as they were.  Accumulators and outputs are fp32 in every arithmetic mode of the encoders."""
import torch

from . import ops
from .bridge import scratch_grads
from .explain import Subject, baseline_images, expand_baseline, forward_measured
from .metrics import NUM_CLASSES

METHODS = ("ig", "smoothgrad")


def plan_chunk(steps, n, image_bytes, free_bytes, share=0.5):
    """Path points per encoder forward: as many as fit `share` of the free device memory, at least 1 and at most `steps`.
    n: image pairs; image_bytes: what one path point of one pair holds while its chunk is in flight (see _pair_bytes)."""
    if steps < 1 or n < 1 or image_bytes <= 0:
        raise ValueError("plan_chunk: steps, n and image_bytes must be positive")
    return int(max(1, min(steps, (share * max(free_bytes, 0)) // (n * image_bytes))))


def _pair_bytes(saved_bytes, E):
    """Device bytes per path point of one image pair: the saved records of both encoders and the transient buffers of one
    backward (counted as one more set of records), the two fp32 inputs and one fp32 input gradient."""
    return 3 * saved_bytes + 3 * 4 * E


def _resolve_chunk(chunk, steps, N, saved_bytes, E, dev):
    if chunk is None:
        free, _ = torch.cuda.mem_get_info(dev)
        return plan_chunk(steps, N, _pair_bytes(saved_bytes, E), free)
    if not isinstance(chunk, int) or not 1 <= chunk <= steps:
        raise ValueError(f"chunk must be None or an integer in [1, {steps}], got {chunk!r}")
    return chunk


class _Run:
    """The state shared by the two methods: engines, targets, accumulators, and the chunk loop."""

    def __init__(self, model, derm, clinic, target, who):
        self.sub = Subject(model, who).check(derm, clinic, target)
        if (derm.shape[2] * derm.shape[3]) % 4:
            raise ValueError(f"{who}: H * W must be a multiple of 4")
        self.target, self.engs = target, self.sub.engs
        self.x = [derm.contiguous(), clinic.contiguous()]
        self.N, self.dev, self.T = derm.shape[0], derm.device, len(NUM_CLASSES)

    def forward_at(self, xs, measure=False):
        """(logits, target_class, saved bytes per image or 0) at the images xs (the targets: self.target)."""
        feats, saved = [], 0
        for eng, x in zip(self.engs, xs):
            if measure:  # what one image's records hold, for the chunk planner: bound and laid out first, so only they count
                eng.prepare(x.device)
                eng.refresh_weights()
                f, bytes_ = forward_measured(eng, x)
                saved = max(saved, bytes_)
            else:
                f, _ = eng.encoder_only("main", x, False, False)
            feats.append(f)
        logits, tc, _ = self.sub.head_grads(torch.cat(feats, dim=1), self.target)
        return logits, tc, saved

    def accumulate(self, make_inputs, steps, chunk, weight, squared):
        """acc [2, T, N, 3, H, W] fp32: for every chunk [k0, k0 + c) make_inputs(m, k0, out [c, N, 3, H, W]) fills modality
        m's inputs; one forward per modality, the 8 head seeds, 8 x 2 data-only backward passes."""
        N, T, dev = self.N, self.T, self.dev
        shape = tuple(self.x[0].shape[1:])
        acc = torch.zeros((2, T, N) + shape, dtype=torch.float32, device=dev)
        for k0 in range(0, steps, chunk):
            c = min(chunk, steps - k0)
            ctxs, feats = [], []
            for m, eng in enumerate(self.engs):
                xin = torch.empty((c, N) + shape, dtype=torch.float32, device=dev)
                make_inputs(m, k0, xin)
                f, ctx = eng.encoder_only("main", xin.view((c * N,) + shape), False, True)
                ctxs.append(ctx), feats.append(f)
                del xin
            _, _, dfeats = self.sub.head_grads(torch.cat(feats, dim=1), self.tc.repeat(c, 1))
            dx = torch.empty((c, N) + shape, dtype=torch.float32, device=dev)
            off = 0
            for m, (eng, ctx, f) in enumerate(zip(self.engs, ctxs, feats)):
                F_ = f.shape[1]
                # BatchNorm parameter gradients that the data-gradient launches accumulate go to a scratch buffer
                with scratch_grads(eng):
                    d = torch.empty(c * N, F_, dtype=eng.tdt, device=dev)
                    for t in range(T):
                        ops.cast_from_f32(eng.dtype, dfeats[t, :, off:off + F_].contiguous(), d)
                        eng.encoder_backward(ctx, d, last_view=True, dx_out=dx.view((c * N,) + shape), params=False)
                        ops.attr_accumulate(dx, acc[m, t], weight, squared)
                off += F_
            del ctxs, feats, dfeats, dx
        return acc

    def finish(self, acc, bases, mode):
        """(attributions [N, T, 2, 3, H, W], maps [N, T, 2, H, W], sums [2, T, N] fp64) of acc [2, T, N, 3, H, W]."""
        T, N = self.T, self.N
        H, W = self.x[0].shape[2:]
        attr = torch.empty_like(acc)
        maps = torch.empty(2, T, N, H, W, dtype=torch.float32, device=self.dev)
        sums = torch.empty(2, T, N, dtype=torch.float64, device=self.dev)
        for m in range(2):
            ops.attr_finish(acc[m], self.x[m], None if bases is None else bases[m], attr[m], maps[m], sums[m], mode)
        return attr.permute(2, 1, 0, 3, 4, 5).contiguous(), maps.permute(2, 1, 0, 3, 4).contiguous(), sums


def integrated_gradients(model, derm, clinic, target="pred", steps=32, baseline="zero", chunk=None):
    """Integrated Gradients of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs.

    model, derm, clinic, target: as sm3hip.cam.grad_cam takes them.  steps: points of the midpoint rule.  baseline: "zero" (zero
    in normalised space: the dataset-mean image) or a pair (derm, clinic) of tensors broadcastable to the images.  chunk: path
    points per encoder forward (None: from the free device memory); every 1 <= chunk <= steps gives the same bits.
    Returns {"attributions": [N, 8, 2, 3, H, W] fp32 (modality 0 derm, 1 clinic), "maps": [N, 8, 2, H, W] fp32 = sum_c
    |attributions|, "logits": 8 x [N, n_i] fp32, "target_class": [N, 8] int64, "baseline_logits": 8 x [N, n_i] fp32, "delta":
    [N, 8] fp64 = sum(attributions of both modalities) - (logit_t(x) - logit_t(baseline)), "steps", "chunk"}."""
    who = "integrated_gradients"
    if not isinstance(steps, int) or steps < 1:
        raise ValueError(f"{who}: steps must be a positive integer")
    pair = baseline_images(baseline, who)
    run = _Run(model, derm, clinic, target, who)
    with torch.no_grad(), ops.stream_scope():
        bases = [expand_baseline(None if pair is None else pair[m], run.x[m]) for m in range(2)]
        logits, run.tc, saved = run.forward_at(run.x, measure=True)
        run.target = run.tc  # fixed at x
        N = run.N
        base_logits, _, _ = run.forward_at([b.expand_as(x).contiguous() for b, x in zip(bases, run.x)])
        E = run.x[0][0].numel()
        c = _resolve_chunk(chunk, steps, N, saved, E, run.dev)
        acc = run.accumulate(lambda m, k0, out: ops.attr_path(run.x[m], bases[m], out, k0, steps), steps, c, 1.0 / steps,
                             False)
        attr, maps, sums = run.finish(acc, bases, 0)
        pick = lambda lg: torch.stack([o.double().gather(1, run.tc[:, t:t + 1])[:, 0] for t, o in enumerate(lg)], dim=1)
        delta = (sums[0] + sums[1]).t() - (pick(logits) - pick(base_logits))
        return {"attributions": attr, "maps": maps, "logits": logits, "target_class": run.tc, "baseline_logits": base_logits,
                "delta": delta, "steps": steps, "chunk": c}


def smooth_grad(model, derm, clinic, target="pred", samples=16, sigma=0.15, squared=False, seed=0, chunk=None):
    """SmoothGrad of the 8 derm7pt labels for a batch of (dermoscopic, clinical) image pairs: the mean over `samples` noisy copies
    of the input gradient of each label's target logit (squared=True: of its square).

    sigma: the noise's standard deviation relative to each image's max - min (per image and modality).  seed: the noise is a
    function of (seed, sample, image position, element) alone; sample k uses stream 2k for derm and 2k + 1 for clinic.  The
    rest as integrated_gradients.  Returns {"attributions", "maps", "logits", "target_class", "samples", "chunk"}."""
    who = "smooth_grad"
    if not isinstance(samples, int) or samples < 1:
        raise ValueError(f"{who}: samples must be a positive integer")
    if not sigma >= 0:
        raise ValueError(f"{who}: sigma must be non-negative")
    if not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64)")
    run = _Run(model, derm, clinic, target, who)
    with torch.no_grad(), ops.stream_scope():
        logits, run.tc, saved = run.forward_at(run.x, measure=True)
        run.target = run.tc
        sig = [((x.amax(dim=(1, 2, 3)) - x.amin(dim=(1, 2, 3))) * float(sigma)).contiguous() for x in run.x]
        E = run.x[0][0].numel()
        c = _resolve_chunk(chunk, samples, run.N, saved, E, run.dev)
        acc = run.accumulate(lambda m, k0, out: ops.attr_noise(run.x[m], sig[m], out, 2 * k0 + m, seed, stride=2), samples, c,
                             1.0 / samples, squared)
        attr, maps, _ = run.finish(acc, None, 1)
        return {"attributions": attr, "maps": maps, "logits": logits, "target_class": run.tc, "samples": samples, "chunk": c}
