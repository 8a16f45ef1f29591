"""Decoded derm7pt images resident on the GPU, where the augmentation kernels read them (csrc/augment.hip,
sm3_aug_resized_crop_ragged).

Every image of the splits a tool uses is decoded ONCE per process (src/utils/data/datasets.load_rgb: PIL, EXIF orientation,
RGB, 25 px border crop) on at most min(workers, 16) host threads and packed HWC, one image after another, into one uint8
arena on the rank's device; per image the host keeps its int64 byte offset and int32 height / width (what the kernel's
host-side checks and the crop-box draws need).  A split has one entry per derm image and one per clinic image, and its
int64 [N, 8] labels on the device, so a batch's labels are one index_select.  At derm7pt's size the three splits take about
2 GB (~1 000 cases x 2 images x 462 x 718 x 3 bytes); every rank holds the whole of each split it uses.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from src.utils.data.datasets import load_rgb


class StoreSplit:
    """One split in the store: derm_ids / clinic_ids [N] (host int32 image indices of case i), labels [N, 8] on the device."""

    def __init__(self, derm_ids, clinic_ids, labels):
        self.derm_ids, self.clinic_ids, self.labels = derm_ids, clinic_ids, labels

    def __len__(self):
        return len(self.derm_ids)


class ImageStore:
    def __init__(self, datasets, device, workers=8):
        """datasets: {mode: SevenPCBaseDataset}; builds the arena on `device`."""
        t0 = time.time()
        paths, self.splits = [], {}
        for mode, ds in datasets.items():
            n, base = len(ds), len(paths)
            paths += list(ds.derm_data) + list(ds.clinic_data)
            ids = torch.arange(base, base + 2 * n, dtype=torch.int32)
            self.splits[mode] = StoreSplit(ids[:n], ids[n:], ds.labels.to(device=device, dtype=torch.int64))
        threads = max(1, min(int(workers), 16))
        with ThreadPoolExecutor(threads) as ex:
            images = list(ex.map(lambda p: np.ascontiguousarray(load_rgb(p)), paths))
        self.img_h = torch.tensor([a.shape[0] for a in images], dtype=torch.int32)
        self.img_w = torch.tensor([a.shape[1] for a in images], dtype=torch.int32)
        nbytes = self.img_h.long() * self.img_w.long() * 3
        self.offset = torch.cumsum(nbytes, 0) - nbytes
        self.arena = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=device)
        for k, a in enumerate(images):
            o = int(self.offset[k])
            self.arena[o:o + a.size].copy_(torch.from_numpy(a).reshape(-1))
            images[k] = None
        torch.cuda.synchronize(device)
        self.paths = paths
        self.build_seconds = time.time() - t0

    def __len__(self):
        return len(self.paths)

    def image(self, k):
        """[H, W, 3] uint8 device view of image k."""
        o, h, w = int(self.offset[k]), int(self.img_h[k]), int(self.img_w[k])
        return self.arena[o:o + h * w * 3].view(h, w, 3)

    def augment(self, aug, ids, gen=None, n_views=1, whole=False):
        """n_views independently augmented [B, 3, H, W] batches of the images `ids` (host int32 [B]) through `aug`
        (a SimCLRAugment chain), or the validation Resize of them when `whole`."""
        from .augment import whole_image_params
        ids = torch.as_tensor(ids, dtype=torch.int32)
        hs, ws = self.img_h[ids.long()], self.img_w[ids.long()]
        out = []
        for _ in range(n_views):
            p = whole_image_params(hs, ws) if whole else aug.sample_ragged(hs, ws, gen)
            out.append(aug.apply_ragged(self.arena, self.offset, self.img_h, self.img_w, ids, p))
        return out


def build_for(args, modes, device, return_index=False):
    """The store of a tool's splits (`modes` of SevenPCBaseDataset) for --data-path; prints what it built."""
    from src.utils.data.datasets import SevenPCBaseDataset
    datasets = {m: SevenPCBaseDataset(args, None, m, return_index=return_index) for m in modes}
    store = ImageStore(datasets, device, args.workers)
    mib = store.arena.numel() / 2 ** 20
    print(f"image store: {len(store)} images of {', '.join(f'{m} {len(d)}' for m, d in datasets.items())} cases, "
          f"{mib:.0f} MiB on {device}, built in {store.build_seconds:.1f} s", flush=True)
    return store
