"""Hand-run generator of the derm7pt metadata fixture (tests/golden/derm7pt_meta/) and of what the REFERENCE'S OWN
`SevenPCBaseDataset` reads from it (tests/golden/derm7pt_ref.npz).

The fixture is a small meta.csv in derm7pt's format that uses every label string the reference's tables know, in every
label column, at least once (plus elevation / sex / location), and the three index files.  The reference's dataset module is
imported from its source at generation time (nothing of it is stored here) with inert stand-ins for what it imports but does
not use to read metadata: `cv2` (imread / cvtColor / COLOR_BGR2RGB), the torchvision.transforms names its functional.py
builds at module level, and numpy 2's removed `np.alltrue`.  The classes are only constructed, never asked for pixels.  The npz also keeps the reference's ValueError message for a
label string no table lists.

    python tests/golden/gen_derm7pt_golden.py [path/to/reference]
"""
import importlib
import os
import sys
import types

import numpy as np
import pandas as pd
import torch  # noqa: F401  (imported before the stand-ins are installed)

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_META = os.path.join(HERE, "derm7pt_meta")

# every string each column's table knows (diagnosis / VS / PIG / RS: the grouped tables the reference's dataset uses)
STRINGS = {
    "diagnosis": ["basal cell carcinoma", "nevus", "blue nevus", "clark nevus", "combined nevus", "congenital nevus",
                  "dermal nevus", "recurrent nevus", "reed or spitz nevus", "melanoma", "melanoma (in situ)",
                  "melanoma (less than 0.76 mm)", "melanoma (0.76 to 1.5 mm)", "melanoma (more than 1.5 mm)",
                  "melanoma metastasis", "DF/LT/MLS/MISC", "dermatofibroma", "lentigo", "melanosis", "miscellaneous",
                  "vascular lesion", "seborrheic keratosis"],
    "pigment_network": ["absent", "typical", "atypical"],
    "blue_whitish_veil": ["absent", "present"],
    "vascular_structures": ["absent", "regular", "arborizing", "comma", "hairpin", "within regression", "wreath",
                            "dotted/irregular", "dotted", "linear irregular"],
    "pigmentation": ["absent", "regular", "diffuse regular", "localized regular", "irregular", "diffuse irregular",
                     "localized irregular"],
    "streaks": ["absent", "regular", "irregular"],
    "dots_and_globules": ["absent", "regular", "irregular"],
    "regression_structures": ["absent", "present", "blue areas", "white areas", "combinations"],
}
N_CASES = 30


def write_fixture():
    rng = np.random.default_rng(7)
    rows = []
    for i in range(N_CASES):
        row = {"case_num": i + 1}
        for col, names in STRINGS.items():
            # the first len(names) cases walk the table, the rest draw from it
            row[col] = names[i % len(names)] if i < len(names) else names[int(rng.integers(len(names)))]
        row.update({"seven_point_score": int(rng.integers(0, 8)), "management": "excision",
                    "clinic": f"Case{i:03d}/c{i:03d}.jpg", "derm": f"Case{i:03d}/d{i:03d}.jpg",
                    "elevation": ["flat", "palpable", "nodular"][i % 3], "location": ["back", "abdomen", "head neck"][i % 3],
                    "sex": ["female", "male"][i % 2], "diagnosis_difficulty": "low"})
        rows.append(row)
    os.makedirs(OUT_META, exist_ok=True)
    pd.DataFrame(rows).to_csv(os.path.join(OUT_META, "meta.csv"), index=False)
    perm = rng.permutation(N_CASES)
    splits = {"train": perm[:17], "valid": perm[17:22], "test": perm[22:]}
    for name, idx in splits.items():
        pd.DataFrame({"indexes": idx}).to_csv(os.path.join(OUT_META, f"{name}_indexes.csv"), index=False)


def reference_dataset_module():
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda *a, **k: None
    cv2.cvtColor = lambda *a, **k: None
    cv2.COLOR_BGR2RGB = 4
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class _Inert:
        def __init__(self, *a, **k):
            pass

    def _attr(name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Inert

    tr.__getattr__ = _attr
    tv.transforms = tr
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tr})
    if not hasattr(np, "alltrue"):
        np.alltrue = np.all
    pkg = types.ModuleType("refdata")
    pkg.__path__ = [os.path.join(REF, "src", "utils", "data")]
    sys.modules["refdata"] = pkg
    return importlib.import_module("refdata.datasets")


def main():
    write_fixture()
    ds_mod = reference_dataset_module()
    args = types.SimpleNamespace(data_path=OUT_META, logger_name="gen")
    out = {}
    for mode in ("train", "val", "test"):
        ds = ds_mod.SevenPCBaseDataset(args, None, mode)
        labels = np.stack([np.asarray(ds.labels[a]) for a in ds_mod.SevenPCBaseDataset.LABEL_ORD], axis=1).astype(np.int64)
        images = os.path.join(OUT_META, "images")
        out[f"{mode}_labels"] = labels
        out[f"{mode}_derm"] = np.array([os.path.relpath(p, images) for p in ds.derm_data])
        out[f"{mode}_clinic"] = np.array([os.path.relpath(p, images) for p in ds.clinic_data])
        print(mode, labels.shape)
    # the reference's message for a label string no table lists (pigment_network "faint" in the first case)
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        for f in os.listdir(OUT_META):
            shutil.copy(os.path.join(OUT_META, f), tmp)
        meta = pd.read_csv(os.path.join(tmp, "meta.csv"))
        meta.loc[0, "pigment_network"] = "faint"
        meta.to_csv(os.path.join(tmp, "meta.csv"), index=False)
        try:
            ds_mod.SevenPCBaseDataset(types.SimpleNamespace(data_path=tmp, logger_name="gen"), None, "train")
            raise SystemExit("the reference accepted an unknown label")
        except ValueError as e:
            out["unknown_label_message"] = np.array(str(e))
            print("unknown label:", e)
    np.savez(os.path.join(HERE, "derm7pt_ref.npz"), **out)


if __name__ == "__main__":
    main()
