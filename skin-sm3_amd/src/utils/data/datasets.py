"""The derm7pt dataset as the reference's tools read it (reference src/utils/data/datasets.py, `SevenPCBaseDataset`).

Files under `--data-path DIR`:

    DIR/meta.csv                  one row per case; the label columns below, `derm` / `clinic` (image names under
                                  DIR/images/), and `elevation`, `sex`, `location`
    DIR/train_indexes.csv         column `indexes`: rows of meta.csv in the split
    DIR/valid_indexes.csv
    DIR/test_indexes.csv
    DIR/images/...

Modes `train` / `val` / `test` select the splits train / valid / test.  Every case has eight labels, in LABEL_ORD order
(diagnosis and the seven-point checklist), grouped into NUM_CLASSES classes each; a label string that no class lists raises
ValueError, index lists that share a row raise ValueError, index lists that do not cover every row of meta.csv only warn.

Images are decoded with PIL: EXIF orientation applied (`ImageOps.exif_transpose`, as cv2.imread's default flags do),
`convert("RGB")`, then CROP pixels removed from every border (the black frame of the derm7pt photographs).  The reference
decodes with cv2 (BGR -> RGB); cv2 is not a dependency here, so a JPEG's decoded pixels are not pinned to cv2's decoder
(libjpeg versions and IDCT choices may differ by a few LSB); PNG decodes are exact.
"""
import os

import numpy as np
import pandas as pd
import torch
from PIL import Image, ImageOps

CROP = 25
LABEL_ORD = ["DIAG", "PN", "BWV", "VS", "PIG", "STR", "DaG", "RS"]
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
COLUMNS = {"DIAG": "diagnosis", "PN": "pigment_network", "BWV": "blue_whitish_veil", "VS": "vascular_structures",
           "PIG": "pigmentation", "STR": "streaks", "DaG": "dots_and_globules", "RS": "regression_structures"}
META_COLUMNS = ("elevation", "sex", "location")


def _classes(*groups):
    """groups[c] = the derm7pt strings of class c -> {string: c}"""
    return {name: c for c, names in enumerate(groups) for name in names}


_NEVI = ("nevus", "blue nevus", "clark nevus", "combined nevus", "congenital nevus", "dermal nevus", "recurrent nevus",
         "reed or spitz nevus")
_MELANOMA = ("melanoma", "melanoma (in situ)", "melanoma (less than 0.76 mm)", "melanoma (0.76 to 1.5 mm)",
             "melanoma (more than 1.5 mm)", "melanoma metastasis")
_OTHER = ("DF/LT/MLS/MISC", "dermatofibroma", "lentigo", "melanosis", "miscellaneous", "vascular lesion")
_ABSENT_REG_IRREG = _classes(("absent",), ("regular",), ("irregular",))

# column -> {derm7pt string: class}; diagnosis and vascular structures / pigmentation / regression structures grouped into
# the classes the paper's tasks use, the other four criteria as derm7pt writes them
LABEL_CLASSES = {
    "DIAG": _classes(("basal cell carcinoma",), _NEVI, _MELANOMA, _OTHER, ("seborrheic keratosis",)),
    "PN": _classes(("absent",), ("typical",), ("atypical",)),
    "BWV": _classes(("absent",), ("present",)),
    "VS": _classes(("absent",), ("regular", "arborizing", "comma", "hairpin", "within regression", "wreath"),
                   ("dotted/irregular", "dotted", "linear irregular")),
    "PIG": _classes(("absent",), ("regular", "diffuse regular", "localized regular"),
                    ("irregular", "diffuse irregular", "localized irregular")),
    "STR": _ABSENT_REG_IRREG,
    "DaG": _ABSENT_REG_IRREG,
    "RS": _classes(("absent",), ("present", "blue areas", "white areas", "combinations")),
}
SPLITS = {"train": "train", "val": "valid", "test": "test"}


def label_column(strings, abbrev):
    """derm7pt strings of one column -> int64 classes; ValueError naming the strings no class lists."""
    strings = np.asarray(strings)
    table = LABEL_CLASSES[abbrev]
    out = np.array([table.get(s, -1) if isinstance(s, str) else -1 for s in strings], dtype=np.int64)
    missing = np.where(out == -1)
    if len(missing[0]):
        raise ValueError("The value `%s` in `strings` do not exist in `names`. Did you spell something wrong?"
                         % strings[missing[0]])
    return out


def read_split(data_path, mode):
    """(derm image paths, clinic image paths, int64 labels [N, 8]) of one split, rows in index-file order."""
    if mode not in SPLITS:
        raise ValueError(f"unknown mode `{mode}` (one of {', '.join(SPLITS)})")
    meta = pd.read_csv(os.path.join(data_path, "meta.csv"))
    idx = {s: list(pd.read_csv(os.path.join(data_path, f"{s}_indexes.csv"))["indexes"]) for s in ("train", "valid", "test")}
    labels = np.stack([label_column(meta[COLUMNS[a]], a) for a in LABEL_ORD], axis=1)
    for col in META_COLUMNS:
        if col not in meta.columns:
            raise ValueError(f"meta.csv has no `{col}` column")
    every = np.concatenate([idx["train"], idx["valid"], idx["test"]])
    if not np.array_equal(np.sort(every), np.arange(len(meta))):
        print("Warning! The train/valid/test indexes do not match the total number of samples.")
    if len(set(every.tolist())) != len(every):
        raise ValueError("Error! There are duplicate indexes in train, valid, or test.")
    rows = np.asarray(idx[SPLITS[mode]], dtype=np.int64)
    if len(rows) and (rows.min() < -len(meta) or rows.max() >= len(meta)):
        raise IndexError(f"{mode} indexes outside meta.csv's {len(meta)} rows")
    images = os.path.join(data_path, "images")
    derm = [os.path.join(images, str(n)) for n in meta["derm"].to_numpy()[rows]]
    clinic = [os.path.join(images, str(n)) for n in meta["clinic"].to_numpy()[rows]]
    return derm, clinic, torch.from_numpy(labels[rows].copy())


def load_rgb(path, crop=CROP):
    """Decoded, EXIF-transposed, border-cropped [H, W, 3] uint8 of one image file."""
    with Image.open(path) as im:
        a = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))
    if a.shape[0] <= 2 * crop or a.shape[1] <= 2 * crop:
        raise ValueError(f"{path}: {a.shape[1]}x{a.shape[0]} image, a side of {2 * crop} px or less leaves nothing after "
                         f"the {crop} px border crop")
    return a[crop:-crop, crop:-crop]


class SevenPCBaseDataset(torch.utils.data.Dataset):
    LABEL_ORD = LABEL_ORD

    def __init__(self, args, data_trans, mode, return_index=False):
        super().__init__()
        self.data_path = os.path.join(args.data_path, "images")
        self.meta_dir = args.data_path
        self.data_trans = data_trans
        self.mode = mode
        self.return_index = return_index
        self.crop_amount = CROP
        self.derm_data, self.clinic_data, self.labels = read_split(args.data_path, mode)

    def __len__(self):
        return len(self.derm_data)

    def __getitem__(self, index):
        derm = Image.fromarray(load_rgb(self.derm_data[index], self.crop_amount))
        clinic = Image.fromarray(load_rgb(self.clinic_data[index], self.crop_amount))
        if self.data_trans is None:
            pass
        elif isinstance(self.data_trans, list):
            derm, clinic = [t(derm) for t in self.data_trans], [t(clinic) for t in self.data_trans]
        else:
            derm, clinic = self.data_trans(derm), self.data_trans(clinic)
        out = (derm, clinic, self.labels[index])
        return (index, out) if self.return_index else out
