"""What the explanation modules (cam.py, attr.py, faith.py) share: the two kinds of model they take -- the linear probe
(src/models/baseline.py `Baseline`) and the SM3 multi-label model (inference.py `Model`) -- their input checks, target classes,
logits and head gradients, the baseline images, and the measurement of what a forward's saved records hold."""
import gc
from itertools import accumulate

import torch

from .metrics import CLS_WEIGHTS, NUM_CLASSES

TARGETS = ("pred", "cls")


def target_class(logits, target, N, dev):
    """[N, 8] int64: `target` itself (a tensor), each label's argmax class ("pred") or the class AUC_AVG scores ("cls")."""
    if isinstance(target, torch.Tensor):
        return target.to(dev)
    if target == "pred":
        return torch.stack([o.argmax(dim=1) for o in logits], dim=1)
    return torch.tensor(CLS_WEIGHTS, dtype=torch.long, device=dev).expand(N, -1).contiguous()


class Subject:
    """The model one call explains: its kind, its two encoders and, after check(), their engines; logits and head gradients
    at pooled features of either kind of model."""

    def __init__(self, model, who):
        self.model, self.who = model, who
        if hasattr(model, "classifier") and hasattr(model, "derm_backbone"):
            self.mlc, self.encoders = False, (model.derm_backbone, model.clinic_backbone)
        elif hasattr(model, "extractor") and hasattr(model, "prototypes") and hasattr(model, "mlc_sa"):
            self.mlc, self.encoders = True, (model.extractor.derm_backbone, model.extractor.clinic_backbone)
        else:
            raise TypeError(f"{who}: model must be a Baseline (src/models/baseline.py) or an inference.py Model")

    def check(self, derm, clinic, target):
        """Refuse what the HIP path does not take, then bind the engines of the two encoders (self.engs).  Returns self."""
        model, who = self.model, self.who
        train = [n for n, m in model.named_modules() if m.training]
        if train:
            raise ValueError(f"{who}: the model must be in eval mode (model.eval()); in train mode: {train[0] or 'model'}")
        for name, x in (("derm", derm), ("clinic", clinic)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise ValueError(f"{who}: {name} must be a CUDA tensor (the SM3 HIP path has no CPU fallback)")
            if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(f"{who}: {name} must be float32 [N, 3, H, W]")
        if derm.shape != clinic.shape:
            raise ValueError(f"{who}: derm and clinic must have the same shape")
        if any(not p.is_cuda for p in model.parameters()):
            raise ValueError(f"{who}: the model's parameters must be on the GPU")
        N = derm.shape[0]
        if isinstance(target, str):
            if target not in TARGETS:
                raise ValueError(f"{who}: target must be 'pred', 'cls' or a LongTensor [N, 8], got {target!r}")
        else:
            if not isinstance(target, torch.Tensor) or target.dtype != torch.int64 or \
                    tuple(target.shape) != (N, len(NUM_CLASSES)):
                raise ValueError(f"{who}: a target tensor must be int64 [N, 8]")
            t = target.cpu()
            for i, n in enumerate(NUM_CLASSES):
                if bool(((t[:, i] < 0) | (t[:, i] >= n)).any()):
                    raise ValueError(f"{who}: target class out of range for label {i} ({n} classes)")
        from .bridge import encoder_engine_for
        self.engs = [encoder_engine_for(enc) for enc in self.encoders]
        return self

    def _heads(self):
        """The eval-mode heads of sm3hip/mlc.py (exact f32, dropout off, BatchNorm1d on running statistics), kept on the model."""
        from .mlc import MLCHeads
        heads = self.model.__dict__.get("_sm3_mlc_heads")
        if heads is None:
            heads = MLCHeads(self.model)
            self.model.__dict__["_sm3_mlc_heads"] = heads
        return heads

    def logits(self, feats):
        """8 x [rows, n_i] fp32 at feature rows [rows, F]."""
        if not self.mlc:
            return [clf(feats).float() for clf in self.model.classifier]  # stock PyTorch heads, as Baseline.forward runs them
        heads = self._heads()
        _, out, _ = heads.forward(feats.contiguous(), 0, train=False)
        return [o.float() for o in out.split(heads.sizes, dim=1)]

    def label_logits(self, feats):
        """For t = 0 .. T - 1 in turn: label t's logits [c * N, n_t] fp32 of label t's rows only, at feats [c, T, N, F]."""
        c, T, N, F_ = feats.shape
        if not self.mlc:
            for t, clf in enumerate(self.model.classifier):
                yield clf(feats[:, t].reshape(c * N, F_)).float()
            return
        heads = self._heads()
        _, out, _ = heads.forward(feats.reshape(c * T * N, F_), 0, train=False)
        out = out.view(c, T, N, -1)
        off = [0] + list(accumulate(heads.sizes))
        for t in range(T):
            yield out[:, t, :, off[t]:off[t + 1]].reshape(c * N, -1).float()

    def head_grads(self, feats, target):
        """(logits: 8 x [N, n_i] fp32, target_class [N, 8], dfeats [T, N, F] fp32 = d logit_t[target] / d feats)."""
        N, dev, T = feats.shape[0], feats.device, len(NUM_CLASSES)
        if not self.mlc:
            logits = self.logits(feats)
            tc = target_class(logits, target, N, dev)
            dfeats = torch.stack([clf.weight.index_select(0, tc[:, t]) for t, clf in enumerate(self.model.classifier)])
            return logits, tc, dfeats.float().contiguous()
        heads = self._heads()
        # the T target copies of the batch through the eval-mode heads (rows are independent: per-sample attention, running
        # BatchNorm1d statistics), one backward with a one-hot seed at copy t's target logit
        _, out, sv = heads.forward(feats.repeat(T, 1).contiguous(), 0, train=False)
        logits = [o.float() for o in out[:N].split(heads.sizes, dim=1)]
        tc = target_class(logits, target, N, dev)
        off = torch.tensor([0] + list(accumulate(heads.sizes))[:-1], dtype=torch.long, device=dev)
        seed = torch.zeros(T, N, out.shape[1], dtype=torch.float32, device=dev)
        seed.scatter_(2, (tc.t() + off[:, None]).unsqueeze(2), 1.0)
        _, dfeats = heads.backward(sv, seed.view(T * N, -1), need_dfeats=True, need_proj=False)
        return logits, tc, dfeats.view(T, N, -1)


def baseline_images(baseline, who):
    """None for "zero", else the pair (derm, clinic) of baseline tensors."""
    if isinstance(baseline, str):
        if baseline != "zero":
            raise ValueError(f"{who}: baseline must be 'zero' or a pair of tensors, got {baseline!r}")
        return None
    if not isinstance(baseline, (tuple, list)) or len(baseline) != 2:
        raise ValueError(f"{who}: baseline must be 'zero' or a pair (derm, clinic) of tensors")
    return baseline


def expand_baseline(b, x):
    """b (None: zero) as a contiguous fp32 [1 or N, 3, H, W] on x's device."""
    if b is None:
        return torch.zeros((1,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    b = torch.as_tensor(b, dtype=torch.float32, device=x.device)
    rows = x.shape[0] if b.dim() == 4 and b.shape[0] != 1 else 1
    return torch.broadcast_to(b, (rows,) + tuple(x.shape[1:])).contiguous()


def forward_measured(eng, x):
    """(features, device bytes per image that the saved records took) of one eval forward of x that keeps the records; they
    are dropped on return.  For the chunk planners."""
    # The figure is a difference of the allocator's counter, so nothing else may be released inside the window: unreachable
    # cycles that still hold device tensors (engines and models of earlier calls) go first, and the collector stays off
    # until the second reading -- collected in the middle of the forward they made the difference negative.
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        before = torch.cuda.memory_allocated(x.device)
        f, ctx = eng.encoder_only("main", x, False, True)
        return f, (torch.cuda.memory_allocated(x.device) - before) // x.shape[0]
    finally:
        if was_on:
            gc.enable()
