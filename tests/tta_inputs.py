"""Inputs and restatements for the test-time-augmentation tests (tests/test_tta_cpu.py, tests/test_tta_gpu.py): the dihedral
elements as torch expressions, the five crop boxes, the fp64 numpy softmax -> Q32 of a view, and the integer reduction over
views.  Nothing here touches a device."""
import numpy as np
import torch

NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
OFF = np.concatenate([[0], np.cumsum(NUM_CLASSES)])
CLS_WEIGHTS = [2, 2, 1, 2, 2, 2, 2, 1]
GROUPS = {"none": [0], "hflip": [0, 1], "flips": [0, 1, 2, 3], "d4": list(range(8))}
ONE = 1 << 32


def torch_view(R, g):
    """Element g of R [..., H, W]: transpose if bit 2, then flip the rows if bit 1, then the columns if bit 0."""
    out = R.transpose(-1, -2) if g & 4 else R
    if g & 2:
        out = out.flip(-2)
    if g & 1:
        out = out.flip(-1)
    return out.contiguous()


def index_view(R, g):
    """The same element from the index formula: out[y][x] = R[y'][x'], a = fy ? H - 1 - y : y, b = fx ? W - 1 - x : x,
    (y', x') = tr ? (b, a) : (a, b)."""
    H, W = R.shape[-2:]
    out = torch.empty_like(R)
    for y in range(H):
        for x in range(W):
            a, b = (H - 1 - y if g & 2 else y), (W - 1 - x if g & 1 else x)
            yy, xx = (b, a) if g & 4 else (a, b)
            out[..., y, x] = R[..., yy, xx]
    return out


def distinct_images(B, H, W, seed=0):
    """[B, 3, H, W] float32 with a different value in every element, in a shuffled order."""
    n = B * 3 * H * W
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(n, generator=g).float() - n // 2).view(B, 3, H, W)


def boxes(h, w, s):
    """The five (i, j, ch, cw) boxes of an h x w image at scale s: centre, top-left, top-right, bottom-left, bottom-right."""
    ch, cw = max(1, round(s * h)), max(1, round(s * w))
    return [((h - ch) // 2, (w - cw) // 2, ch, cw), (0, 0, ch, cw), (0, w - cw, ch, cw), (h - ch, 0, ch, cw),
            (h - ch, w - cw, ch, cw)]


IMAGE_SIZES = [(1, 1), (7, 5), (37, 73), (64, 64), (301, 33)]


def arena(seed=5):
    """A hand-built image arena: random uint8 images of IMAGE_SIZES packed HWC one after another.
    (arena uint8 [bytes], offset int64, img_h int32, img_w int32) on the host."""
    g = np.random.default_rng(seed)
    imgs = [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in IMAGE_SIZES]
    nbytes = np.array([a.size for a in imgs], dtype=np.int64)
    offset = np.cumsum(nbytes) - nbytes
    return (torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])), torch.from_numpy(offset),
            torch.tensor([h for h, _ in IMAGE_SIZES], dtype=torch.int32), torch.tensor([w for _, w in IMAGE_SIZES], dtype=torch.int32))


def random_logits(B, V, seed):
    g = np.random.default_rng(seed)
    return (4.0 * g.standard_normal((B, V, 24))).astype(np.float32)


def edge_logits(V, seed):
    """Three cases: every logit equal (ties go to the lowest index); label 0 = [80, -80, 0, 0, 0] in every view; label 1 all -80."""
    z = random_logits(3, V, seed)
    z[0] = 0.5
    z[1, :, 0:5] = np.float32([80, -80, 0, 0, 0])
    z[2, :, 5:8] = -80.0
    return z


def q_of(logits):
    """int64 [B, V, 24]: per (case, view, label) the fp64 softmax -- z - max, exp, the sum in ascending class order, one division --
    as Q32, rint(p * 2^32)."""
    z = logits.astype(np.float64)
    q = np.empty(z.shape, dtype=np.int64)
    for t in range(8):
        zt = z[..., OFF[t]:OFF[t + 1]]
        e = np.exp(zt - zt.max(axis=-1, keepdims=True))
        s = np.zeros(e.shape[:-1])
        for c in range(e.shape[-1]):
            s = s + e[..., c]
        q[..., OFF[t]:OFF[t + 1]] = np.rint(e / s[..., None] * 4294967296.0).astype(np.int64)
    return q


def reduce_ints(q, logits):
    """Everything that crosses views, from the integers q [B, V, 24] and the argmax of the views' logits."""
    B, V, _ = q.shape
    out = {"sum_q": q.sum(axis=1), "min_q": q.min(axis=1), "max_q": q.max(axis=1)}
    vc, ac = np.empty((B, V, 8), dtype=np.int64), np.empty((B, 8), dtype=np.int64)
    for t in range(8):
        vc[:, :, t] = logits[:, :, OFF[t]:OFF[t + 1]].argmax(axis=2)       # numpy: the first maximum
        ac[:, t] = out["sum_q"][:, OFF[t]:OFF[t + 1]].argmax(axis=1)
    out.update(view_class=vc, agg_class=ac, disagree=(vc != ac[:, None, :]).sum(axis=1))
    return out


def preds_of(sum_q, V):
    return np.log(np.maximum(sum_q, 1).astype(np.float64) / (V * 4294967296.0)).astype(np.float32)
