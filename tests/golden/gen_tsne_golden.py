"""Writes tests/golden/tsne_sklearn_ref.json: what scikit-learn's exact t-SNE reaches on tests/tsne_ref.py:blobs(300, 16, 6, 0)
over 20 seeds -- the final KL divergence and trustworthiness(n_neighbors=10) of each run.  The spread over the seeds is the
margin of the quality condition in tests/test_tsne_cpu.py and tests/test_tsne_gpu.py, which read only the JSON.

    python tests/golden/gen_tsne_golden.py        (needs scikit-learn; about a minute on a CPU)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tsne_ref  # noqa: E402

SEEDS = list(range(20))
INPUT = {"N": 300, "D": 16, "k": 6, "seed": 0}
SETTINGS = {"method": "exact", "init": "random", "perplexity": 30, "max_iter": 1000}


def main():
    import sklearn
    from sklearn.manifold import TSNE, trustworthiness
    x, _ = tsne_ref.blobs(**INPUT)
    runs = []
    for s in SEEDS:
        t = TSNE(random_state=s, **SETTINGS)
        y = t.fit_transform(x)
        runs.append({"seed": s, "kl": float(t.kl_divergence_), "trustworthiness": float(trustworthiness(x, y, n_neighbors=10)),
                     "n_iter": int(t.n_iter_)})
        print(runs[-1], flush=True)
    # the restatement's trustworthiness must be scikit-learn's: checked on the last map, recorded for the tests
    own = tsne_ref.trustworthiness(x, y, 10)
    assert abs(own - runs[-1]["trustworthiness"]) < 1e-12, (own, runs[-1])
    out = {"sklearn": sklearn.__version__, "input": INPUT, "settings": SETTINGS, "n_neighbors": 10, "runs": runs,
           "input_checksum": float(np.asarray(x, dtype=np.float64).sum())}
    with open(os.path.join(HERE, "tsne_sklearn_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
