#!/usr/bin/env python
"""Times nvsm_kmeans (Model.kmeans) on seeded random tables.

Per shape (n, d, k) — default (100 000, 256, 64), (2 000 000, 256, 1024) and (500 000, 300, 256); d = 300 clusters the words table,
every other d the documents table — a call of --iterations Lloyd iterations from a given start (tol 0, so only a strict stop could
end it early): iterations per second on the host clock, and from the handle's profiler in a second call the milliseconds per
iteration of the assignment pass and of the centre update, the assignment pass's fp32 rate (2·n·k·d flop) and the share of it that
reading the rows once (n·d·4 bytes) would take at the 5.5 TB/s streaming reads reach. In the same process the same iteration as ONE
PyTorch-ROCm expression on resident tensors —
    labels = (|c|² − 2 X·Cᵀ).argmin(1);  sums = zeros(k, d).index_add_(0, labels, X);  C = sums / bincount(labels)
— timed over --torch-iterations launches wherever its n × k intermediate fits --baseline-gb. One JSON line per shape on stdout. One
box, one run, no threshold attached. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_BYTES_PER_S = 5.5e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="100000,256,64;2000000,256,1024;500000,300,256", help="n,d,k;n,d,k;...")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--torch-iterations", type=int, default=5)
    ap.add_argument("--baseline-gb", type=float, default=48.0, help="largest PyTorch expression that is still run")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_kmeans.py needs a GPU (MI355X): the k-means kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)

    for shape in args.shapes.split(";"):
        n, d, k = [int(x) for x in shape.split(",")]
        rs = np.random.RandomState(77 + k)
        # k loose blobs: labels keep moving for the iterations timed
        X = (rs.standard_normal((k, d)).astype(np.float32)[rs.randint(0, k, n)] + rs.standard_normal((n, d)).astype(np.float32))
        words = d == 300
        cfg = ca.default_config(num_words=n if words else 100, num_entities=100 if words else n, word_repr_size=d if words else 8,
                                entity_repr_size=8 if words else d, window_size=2, num_random_entities=1, batch_normalization=0,
                                nonlinearity="tanh", update_method="sgd", max_batch_size=8, device=args.device)
        m = ca.Model(cfg)
        m.set_param("word_representations-representations" if words else "entity_representations-representations", X)
        start = X[rs.choice(n, k, replace=False)]
        kw = dict(space="words" if words else "entities", num_clusters=k, init=start, max_iter=args.iterations, tol=0.0)
        m.kmeans(**dict(kw, max_iter=1))                                  # scratch allocated, kernels loaded
        t0 = time.perf_counter()
        labels, centers, counts, inertia, n_iter = m.kmeans(**kw)
        seconds = time.perf_counter() - t0
        m.profile_enable(True)
        m.profile_reset()
        m.kmeans(**kw)
        prof = m.profile()
        m.profile_enable(False)
        assign, update = prof["kmeans_assign"], prof["kmeans_update"]
        assign_ms, update_ms = assign[0] / assign[1], update[0] / update[1]
        line = dict(rows=n, dim=d, clusters=k, iterations=n_iter, inertia=round(inertia, 2), call_s=round(seconds, 3),
                    iterations_per_s=round(n_iter / seconds, 3), assign_ms=round(assign_ms, 4), update_ms=round(update_ms, 4),
                    assign_tflops=round(2.0 * n * k * d / assign_ms / 1e9, 2),
                    row_read_share=round(n * d * 4.0 / STREAM_BYTES_PER_S * 1e3 / assign_ms, 4),
                    rows_ms=round(prof["kmeans_rows"][0], 3), inertia_ms=round(prof["kmeans_inertia"][0], 3),
                    torch_ms_per_iteration=None, speedup=None)
        m.close()
        del m
        if (n * k * 4.0 * 2 + n * d * 4.0 * 2) <= args.baseline_gb * 2 ** 30:
            Xt = torch.from_numpy(X).to(dev)
            Ct = torch.from_numpy(start).to(dev)

            def step(Ct):
                lab = ((Ct * Ct).sum(dim=1)[None, :] - 2.0 * (Xt @ Ct.T)).argmin(dim=1)
                sums = torch.zeros_like(Ct).index_add_(0, lab, Xt)
                cnt = torch.bincount(lab, minlength=k).clamp_min(1).to(Ct.dtype)
                return sums / cnt[:, None]

            Ct = step(Ct)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.torch_iterations):
                Ct = step(Ct)
            torch.cuda.synchronize(dev)
            tb = (time.perf_counter() - t0) / args.torch_iterations * 1e3
            line.update(torch_ms_per_iteration=round(tb, 4), speedup=round(tb / (seconds / n_iter * 1e3), 2))
            del Xt, Ct
            torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
