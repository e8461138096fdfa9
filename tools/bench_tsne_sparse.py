#!/usr/bin/env python
"""Times nvsm_tsne_sparse (Model.tsne(method="sparse")) on seeded random document tables.

Per n: seconds per synchronous call on the host clock and, from the handle's profiler in a second call, milliseconds per iteration
(tsne_forces — attraction, repulsion, Z — plus tsne_update), the once-per-call stages (rows, the neighbour rounds with their
selection and sort, the perplexity search, the symmetrisation), the convergence checks, and the pairs per second the repulsion
reaches. At the sizes nvsm_tsne still serves (default 8 000 and 20 000 rows) the exact call runs on the same rows from the same
start, and the trustworthiness (5 neighbours, sklearn's definition, evaluated with PyTorch-ROCm on the device) of both pictures is
reported. The sizes beyond its cap (default 100 000 and 500 000) run alone, with --big-iterations iterations. The rows are
--clusters Gaussian clusters, so that a picture has something to keep. One JSON line per n on stdout and, with --out, in that file.
One box, one run, no threshold attached. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trustworthiness(torch, X, Y, k=5, chunk=1024):
    """sklearn.manifold.trustworthiness (Euclidean) on the device, rows in chunks"""
    n = X.shape[0]
    total = 0.0
    for c0 in range(0, n, chunk):
        rows = torch.arange(c0, min(n, c0 + chunk), device=X.device)
        dX = torch.cdist(X[rows].double(), X.double())
        dX[torch.arange(len(rows)), rows] = float("inf")
        rank = torch.empty_like(dX, dtype=torch.int64)
        rank.scatter_(1, torch.argsort(dX, dim=1, stable=True), torch.arange(1, n + 1, device=X.device).expand(len(rows), n).contiguous())
        dY = torch.cdist(Y[rows].double(), Y.double())
        dY[torch.arange(len(rows)), rows] = float("inf")
        near = torch.topk(dY, k, dim=1, largest=False).indices
        total += float((rank.gather(1, near) - k).clamp_min(0).sum())
    return 1.0 - total * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="8000,20000", help="sizes that also run nvsm_tsne on the same rows")
    ap.add_argument("--big-rows", default="100000,500000", help="sizes beyond nvsm_tsne's cap: the sparse call alone")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--big-iterations", type=int, default=100)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_tsne_sparse.py needs a GPU (MI355X): the t-SNE kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    sink = open(args.out, "w") if args.out else None
    small = [int(x) for x in args.rows.split(",") if x]
    big = [int(x) for x in args.big_rows.split(",") if x]

    for n in small + big:
        iterations = args.iterations if n in small else args.big_iterations
        rs = np.random.RandomState(77 + n)
        centres = rs.standard_normal((args.clusters, args.dim))
        E = (centres[np.arange(n) % args.clusters] + 0.25 * rs.standard_normal((n, args.dim))).astype(np.float32)
        cfg = ca.default_config(num_words=100, num_entities=n, word_repr_size=8, entity_repr_size=args.dim, window_size=2,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=8, device=args.device)
        m = ca.Model(cfg)
        m.set_param("entity_representations-representations", E)
        kw = dict(max_iter=iterations, init="random", n_iter_without_progress=iterations)
        m.tsne(max_iter=2, init="random", method="sparse")                 # scratch allocated, kernels loaded
        t0 = time.perf_counter()
        Y, kl, n_iter = m.tsne(method="sparse", **kw)
        seconds = time.perf_counter() - t0
        m.profile_enable(True)
        m.profile_reset()
        m.tsne(method="sparse", **kw)
        prof = m.profile()
        m.profile_enable(False)
        forces, update = prof["tsne_forces"], prof["tsne_update"]
        ms_iter = forces[0] / forces[1] + update[0] / update[1]
        k = min(n - 1, 91)
        line = dict(rows=n, dim=args.dim, neighbors=k, iterations=n_iter + 1, kl=round(kl, 4), call_s=round(seconds, 3),
                    ms_per_iteration=round(ms_iter, 4), forces_ms=round(forces[0] / forces[1], 4), update_ms=round(update[0] / update[1], 4),
                    pairs_per_s=round(float(n) * (n - 1) / (forces[0] / forces[1] * 1e-3), -9),
                    rows_ms=round(prof["tsne_rows"][0], 3), nn_scan_ms=round(prof["tsne_nn_scan"][0], 3),
                    nn_select_sort_ms=round(prof["rank_select"][0] + prof["rank_sort"][0], 3), conditionals_ms=round(prof["tsne_conditionals"][0], 3),
                    symmetrize_ms=round(prof["tsne_symmetrize"][0], 3), kl_checks_ms=round(prof["tsne_kl"][0], 3),
                    exact_call_s=None, exact_ms_per_iteration=None, exact_kl=None, trustworthiness=None, exact_trustworthiness=None)
        if n in small:
            X = torch.from_numpy(E).to(dev)
            line["trustworthiness"] = round(trustworthiness(torch, X, torch.from_numpy(Y).to(dev)), 4)
            m.tsne(max_iter=2, init="random")
            t0 = time.perf_counter()
            Ye, kle, _ = m.tsne(**kw)
            exact_s = time.perf_counter() - t0
            m.profile_enable(True)
            m.profile_reset()
            m.tsne(**kw)
            pe = m.profile()
            m.profile_enable(False)
            line.update(exact_call_s=round(exact_s, 3), exact_kl=round(kle, 4),
                        exact_ms_per_iteration=round(pe["tsne_forces"][0] / pe["tsne_forces"][1] + pe["tsne_update"][0] / pe["tsne_update"][1], 4),
                        exact_trustworthiness=round(trustworthiness(torch, X, torch.from_numpy(Ye).to(dev)), 4))
            del X
            torch.cuda.empty_cache()
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()
        m.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
