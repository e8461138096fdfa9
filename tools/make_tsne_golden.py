"""Writes tests/golden/tsne/end_to_end.json: what the fp64 restatement of exact t-SNE (tests/tsne_reference.py, numpy only) reaches on
the end-to-end inputs of tests/test_gpu_tsne.py from five random starts — each run's final KL (recomputed from its embedding) and
trustworthiness. The GPU test holds nvsm_tsne to the band these runs span, widened by its own width on either side: a chaotic
optimiser can be held to the spread over starts and to nothing finer. The generator asserts that every run separates the three
clusters (each point's nearest neighbour in the picture carries its label); rerun it with another seed if one does not.

    python tools/make_tsne_golden.py [--seed 2024]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tsne_reference as tr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2024)
    args = ap.parse_args()
    X, labels = tr.clusters(np.random.RandomState(args.seed))      # n = 300, d = 16, three clusters, spread 0.25
    P = tr.affinities(X, 30.0)[0]
    runs = []
    for start in range(5):
        Y0 = (1e-4 * np.random.RandomState(start).standard_normal((len(X), 2))).astype(np.float32)
        Y, kl, n_iter = tr.tsne(X, perplexity=30.0, max_iter=1000, init=Y0)
        agree = tr.nearest_label_agreement(Y, labels)
        assert agree == 1.0, "start %d leaves %.4f of the points next to their own cluster: choose other inputs" % (start, agree)
        runs.append(dict(start=start, kl=tr.kl_divergence(P, Y), kl_reported=kl, trustworthiness=tr.trustworthiness(X, Y, 5), n_iter=n_iter))
        print(runs[-1])
    out = dict(seed=args.seed, n=300, d=16, clusters=3, spread=0.25, perplexity=30.0, max_iter=1000, n_neighbors=5, runs=runs)
    path = os.path.join(ROOT, "tests", "golden", "tsne", "end_to_end.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
