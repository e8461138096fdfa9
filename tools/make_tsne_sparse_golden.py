"""Writes tests/golden/tsne/sparse_end_to_end.json: what the fp64 restatement of sparse-affinity t-SNE (tests/tsne_sparse_reference.py,
numpy only) reaches on the end-to-end inputs of tests/test_gpu_tsne_sparse.py from five random starts — each run's final error
(recomputed from its embedding over the stored entries) and trustworthiness. The GPU test holds nvsm_tsne_sparse to the band these
runs span, widened by its own width on either side (tools/make_tsne_golden.py's rule). The generator asserts that every run separates
the three clusters; rerun it with another seed if one does not.
Beside the bands, and asserted by nothing, it records scikit-learn's own method='barnes_hut' at angle 0 and at its default 0.5 on the
same rows where scikit-learn is installed: what the tree approximation costs, next to what this restatement reaches.

    python tools/make_tsne_sparse_golden.py [--seed 2024]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tsne_reference as tr  # noqa: E402
from tests import tsne_sparse_reference as ts  # noqa: E402


def sklearn_runs(X, csr):
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return []
    out = []
    for angle in (0.0, 0.5):
        sk = TSNE(n_components=2, method="barnes_hut", angle=angle, init="pca", random_state=0, perplexity=30.0, max_iter=1000)
        Y = sk.fit_transform(X)
        out.append(dict(angle=angle, kl=ts.kl_sparse(*csr, Y), kl_reported=float(sk.kl_divergence_), trustworthiness=tr.trustworthiness(X, Y, 5),
                        n_iter=int(sk.n_iter_)))
        print("sklearn", out[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    X, labels = tr.clusters(np.random.RandomState(args.seed))      # n = 300, d = 16, three clusters, spread 0.25
    csr = ts.affinities_nn(X, 30.0)[:3]
    runs = []
    for start in range(5):
        Y0 = (1e-4 * np.random.RandomState(start).standard_normal((len(X), 2))).astype(np.float32)
        Y, kl, n_iter = ts.tsne_sparse(X, perplexity=30.0, max_iter=1000, init=Y0)
        agree = tr.nearest_label_agreement(Y, labels)
        assert agree == 1.0, "start %d leaves %.4f of the points next to their own cluster: choose other inputs" % (start, agree)
        runs.append(dict(start=start, kl=ts.kl_sparse(*csr, Y), kl_reported=kl, trustworthiness=tr.trustworthiness(X, Y, 5), n_iter=n_iter))
        print(runs[-1])
    out = dict(seed=args.seed, n=300, d=16, clusters=3, spread=0.25, perplexity=30.0, n_neighbors_affinities=ts.default_neighbors(300, 30.0),
               max_iter=1000, n_neighbors=5, runs=runs, sklearn_barnes_hut=sklearn_runs(X, csr))
    path = os.path.join(ROOT, "tests", "golden", "tsne", "sparse_end_to_end.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
