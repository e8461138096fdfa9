#!/usr/bin/env python
"""Times nvsm_tsne (Model.tsne) on seeded random document tables.

Per n (default 2 000, 8 000 and 20 000 rows, d = 256, 1 000 iterations, perplexity 30, a random start): seconds per synchronous call
on the host clock; from the handle's profiler in a second call, milliseconds per iteration (tsne_forces + tsne_update), the share
of an iteration that reading P once (n²·4 bytes) would take at the 5.5 TB/s streaming reads reach, and the once-per-call stages
(tsne_rows, tsne_affinities) and, from a one-iteration call with the default start, the PCA start (tsne_pca: the covariance on the
device and the Jacobi solver on the host, which the timed calls bypass with their random start). In the same process the same iteration as ONE PyTorch-ROCm expression on resident tensors —
    d = Y[:, None] − Y[None];  q = 1 / (1 + Σ d²), q_ii = 0;  g = 4·(Σ_j e·P·q·d − Σ_j q²·d / Σ q);  gains, update, Y as sklearn
— timed over --torch-iterations launches wherever its intermediates (about 6·n²·4 bytes) fit --baseline-gb. One JSON line per n on
stdout. One box, one run, no threshold attached. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_BYTES_PER_S = 5.5e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="2000,8000,20000")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--torch-iterations", type=int, default=20)
    ap.add_argument("--baseline-gb", type=float, default=48.0, help="largest PyTorch expression that is still run")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_tsne.py needs a GPU (MI355X): the t-SNE kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)

    for n in [int(x) for x in args.rows.split(",")]:
        rs = np.random.RandomState(77 + n)
        E = rs.standard_normal((n, args.dim)).astype(np.float32)
        cfg = ca.default_config(num_words=100, num_entities=n, word_repr_size=8, entity_repr_size=args.dim, window_size=2,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=8, device=args.device)
        m = ca.Model(cfg)
        m.set_param("entity_representations-representations", E)
        kw = dict(max_iter=args.iterations, init="random", n_iter_without_progress=args.iterations)
        m.tsne(max_iter=2, init="random")                                  # scratch allocated, kernels loaded
        t0 = time.perf_counter()
        Y, kl, n_iter = m.tsne(**kw)
        seconds = time.perf_counter() - t0
        m.profile_enable(True)
        m.profile_reset()
        m.tsne(**kw)
        prof = m.profile()
        m.profile_enable(False)
        m.profile_enable(True)
        m.profile_reset()
        t0 = time.perf_counter()
        m.tsne(max_iter=1, init="pca")                                     # the default start: covariance on the device, Jacobi on the host
        pca_call = time.perf_counter() - t0
        pca_ms = m.profile()["tsne_pca"][0]
        m.profile_enable(False)
        forces, update = prof["tsne_forces"], prof["tsne_update"]
        ms_iter = forces[0] / forces[1] + update[0] / update[1]
        line = dict(rows=n, dim=args.dim, iterations=n_iter + 1, kl=round(kl, 4), call_s=round(seconds, 3), ms_per_iteration=round(ms_iter, 4),
                    forces_ms=round(forces[0] / forces[1], 4), update_ms=round(update[0] / update[1], 4),
                    p_read_share=round(n * n * 4.0 / STREAM_BYTES_PER_S * 1e3 / ms_iter, 4),
                    rows_ms=round(prof["tsne_rows"][0], 3), affinities_ms=round(prof["tsne_affinities"][0], 3),
                    kl_checks_ms=round(prof["tsne_kl"][0], 3), pca_start_ms=round(pca_ms, 3), one_iteration_call_with_pca_s=round(pca_call, 3), torch_ms_per_iteration=None, speedup=None)
        if 6.0 * n * n * 4 <= args.baseline_gb * 2 ** 30:
            P = torch.rand((n, n), device=dev)
            P = (P + P.T) / (2.0 * n * n)
            Yt = torch.from_numpy(1e-4 * rs.standard_normal((n, 2)).astype(np.float32)).to(dev)
            upd, gains = torch.zeros_like(Yt), torch.ones_like(Yt)

            def step(Yt, upd, gains, e=12.0, momentum=0.5, lr=200.0):
                d = Yt[:, None, :] - Yt[None, :, :]
                q = 1.0 / (1.0 + (d * d).sum(dim=2))
                q.fill_diagonal_(0.0)
                g = 4.0 * (((e * P * q)[:, :, None] * d).sum(dim=1) - ((q * q / q.sum())[:, :, None] * d).sum(dim=1))
                gains = torch.where(upd * g < 0, gains + 0.2, gains * 0.8).clamp_min(0.01)
                upd = momentum * upd - lr * (g * gains)
                return Yt + upd, upd, gains

            for _ in range(2):
                Yt, upd, gains = step(Yt, upd, gains)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.torch_iterations):
                Yt, upd, gains = step(Yt, upd, gains)
            torch.cuda.synchronize(dev)
            tb = (time.perf_counter() - t0) / args.torch_iterations * 1e3
            line.update(torch_ms_per_iteration=round(tb, 4), speedup=round(tb / ms_iter, 2))
            del P, Yt, upd, gains
            torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)
        m.close()


if __name__ == "__main__":
    main()
