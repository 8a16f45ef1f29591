"""The ragged vs the fixed crop kernel at derm7pt size (B=256 images of 462 x 718 -> 224 x 224), outputs compared; run under
rocprofv3 --kernel-trace --stats (profiles/derm7pt_crop_kernels.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import torch  # noqa: E402
from sm3hip import _lib, ops  # noqa: E402
from sm3hip.augment import SimCLRAugment  # noqa: E402

B, Hs, Ws, H, W = 256, 462, 718, 224, 224
dev = torch.device("cuda", 0)
src = torch.randint(0, 256, (B, Hs, Ws, 3), dtype=torch.uint8, device=dev)
arena = src.reshape(-1)
off = torch.arange(B, dtype=torch.int64) * Hs * Ws * 3
hh, ww = torch.full((B,), Hs, dtype=torch.int32), torch.full((B,), Ws, dtype=torch.int32)
idx = torch.arange(B, dtype=torch.int32)
p = SimCLRAugment((H, W), [0.0] * 3, [1.0] * 3).sample(B, Hs, Ws, torch.Generator().manual_seed(0))
box, flip = p.box.to(dev), p.flip.to(dev)
lib, st = _lib.load(), ops._stream()
a = torch.empty(B, 3, H, W, device=dev)
b = torch.empty_like(a)
for _ in range(20):
    _lib.check(lib.sm3_aug_resized_crop(ops._ptr(src), B, Hs, Ws, ops._ptr(box), ops._ptr(flip), ops._ptr(a), H, W, st), "f")
    _lib.check(lib.sm3_aug_resized_crop_ragged(ops._ptr(arena), arena.numel(), off.data_ptr(), hh.data_ptr(), ww.data_ptr(), B,
                                               idx.data_ptr(), p.box.data_ptr(), p.flip.data_ptr(), B, ops._ptr(b), H, W, st), "r")
torch.cuda.synchronize()
assert torch.equal(a, b)
print("crop kernels ok, outputs equal")
