"""Hand-run generator of tests/golden/checklist_points.json: per label the class numbers, abbreviations and seven-point `scores`
of the label tables that the REFERENCE'S OWN `SevenPCBaseDataset` uses -- the class `SevenPCGroupDataset`, whose diagnosis, VS,
PIG and RS tables are the grouped ones and whose other tables are the base class's.

The reference's dataset module is imported from its source at generation time (nothing of it is stored here), with the inert
stand-ins of gen_derm7pt_golden.py for what it imports but does not use to read metadata.  The dataset is constructed on the
metadata fixture tests/golden/derm7pt_meta/ and asked which metadata class it built; the tables are read from that class by the
attribute names its `tags` table lists.  Diagnosis has no `scores` column (null in the file).

    python tests/golden/gen_checklist_golden.py [path/to/reference]
"""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    spec = importlib.util.spec_from_file_location("gen_derm7pt_golden", os.path.join(HERE, "gen_derm7pt_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)  # its REF is argv[1] or the default
    ds_mod = gen.reference_dataset_module()
    seen = []
    group = ds_mod.SevenPCGroupDataset
    init = group.__init__

    def recording_init(self, *a, **k):
        seen.append(type(self))
        init(self, *a, **k)

    group.__init__ = recording_init
    try:
        ds_mod.SevenPCBaseDataset(types.SimpleNamespace(data_path=gen.OUT_META, logger_name="gen"), None, "train")
    finally:
        group.__init__ = init
    assert seen == [group], "SevenPCBaseDataset no longer reads its labels through SevenPCGroupDataset"
    out = {"label_order": list(ds_mod.SevenPCBaseDataset.LABEL_ORD), "labels": {}}
    for _, tag in group.tags.iterrows():
        table = getattr(group, tag.colnames)
        out["labels"][tag.abbrevs] = {
            "column": tag.colnames, "seven_pt": int(tag.seven_pt), "nums": [int(v) for v in table.nums],
            "abbrevs": [str(v) for v in table.abbrevs],
            "scores": [int(v) for v in table.scores] if "scores" in table.columns else None}
        print(tag.abbrevs, out["labels"][tag.abbrevs])
    with open(os.path.join(HERE, "checklist_points.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
