#!/usr/bin/env python
"""Times nvsm_neighbors against the plumbing baseline on seeded synthetic tables.

Per shape (|V| rows in the words AND the documents table, d_w = 300, d_e = 256, top k = 30, Q queries given as row ids of the
searched space — what related_terms does) and per space (words, projected_words, entities): milliseconds per synchronous call
on the host clock, the algorithmic table bytes (rows·dim·4) over the time as a share of the 6.29 TB/s HBM delivers, the
2·Q·rows·dim FLOP over the time as a share of the 157 TFLOP/s of the exact-fp32 matrix pipe, and which of the two bounds the
shape. In the same process, call by call in alternation:
  * the same search as ONE PyTorch-ROCm expression on resident tensors, torch.topk(normalize(X[ids]) @ normalize(X).T, k),
    plus the copy of its results to the host (X: the table; for the projected space the projected matrix, computed by torch
    once, outside the timing — the call under test projects the vocabulary inside every call);
  * for the words space only, the call forced through rank_scan_plain_kernel (a test-hooks entry, no environment switch):
    `plain_minus_ours_ms` holds the pairwise differences (median, min, max over the alternating pairs) — the MFMA scan with
    the tail chunk serves d = 300 if the smallest difference is positive at every Q.
Every shape is warmed up and timed for at least --seconds of work per contender. One JSON line per shape on stdout.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12
MFMA_F32_FLOPS = 157e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--words", default="50000,500000", help="|V|: rows of the words and of the documents table")
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--spaces", default="words,projected_words,entities")
    ap.add_argument("--word-dim", type=int, default=300)
    ap.add_argument("--entity-dim", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=30)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and contender")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_neighbors.py needs a GPU (MI355X): the neighbour kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    dw, de = args.word_dim, args.entity_dim
    normalize = torch.nn.functional.normalize

    for V in [int(x) for x in args.words.split(",")]:
        k = min(args.top_k, V)
        gen = torch.Generator(device=dev)
        gen.manual_seed(4321 + V)
        W_t = torch.rand((V, dw), generator=gen, device=dev, dtype=torch.float32) - 0.5
        E_t = torch.rand((V, de), generator=gen, device=dev, dtype=torch.float32) - 0.5
        rs = np.random.RandomState(7)
        T = (rs.uniform(-1, 1, de * dw) * 0.2).astype(np.float32)
        b = rs.uniform(-0.1, 0.1, de).astype(np.float32)
        cfg = ca.default_config(num_words=V, num_entities=V, word_repr_size=dw, entity_repr_size=de, window_size=10,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=64, device=args.device)
        m = ca.Model(cfg)
        m.set_param("word_representations-representations", W_t.cpu().numpy())
        m.set_param("entity_representations-representations", E_t.cpu().numpy())
        m.set_param("word_entity_mapping-transform", T)
        m.set_param("word_entity_mapping-bias", b)
        # the projected vocabulary as torch computes it: tanh(W·T + b), T stored [d_w][d_e]
        X_p = torch.tanh(W_t @ torch.from_numpy(T.reshape(dw, de)).to(dev) + torch.from_numpy(b).to(dev))
        tables = {"words": W_t, "projected_words": X_p, "entities": E_t}
        for space in args.spaces.split(","):
            X = tables[space]
            dim = X.shape[1]
            for Q in [int(x) for x in args.queries.split(",")]:
                ids = rs.choice(V, Q, replace=False).astype(np.int64)
                ids_t = torch.from_numpy(ids).to(dev)

                def ours():
                    t0 = time.perf_counter()
                    out = m.neighbors(space, ids=ids, top_k=k)
                    return time.perf_counter() - t0, out

                def plain():
                    ca.lib().nvsm_debug_neighbors_force_plain(1)
                    try:
                        return ours()
                    finally:
                        ca.lib().nvsm_debug_neighbors_force_plain(0)

                def baseline():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    Xn = normalize(X, dim=1)
                    v, i = torch.topk(normalize(X[ids_t], dim=1) @ Xn.T, k, dim=1)
                    v, i = v.cpu(), i.cpu()                                  # host results, as nvsm_neighbors returns them
                    return time.perf_counter() - t0, (i.numpy(), v.numpy())

                with_plain = space == "words"
                for _ in range(2):
                    ours()
                    baseline()
                    if with_plain:
                        plain()
                t_ours, t_base, t_plain = [], [], []
                while sum(t_ours) < args.seconds or sum(t_base) < args.seconds or len(t_ours) < 5 or \
                        (with_plain and sum(t_plain) < args.seconds):
                    dt, got = ours()
                    t_ours.append(dt)
                    dt, ref = baseline()
                    t_base.append(dt)
                    if with_plain:
                        dt, got_plain = plain()
                        t_plain.append(dt)
                t, tb = float(np.median(t_ours)), float(np.median(t_base))
                table_bytes, flop = V * dim * 4.0, 2.0 * Q * V * dim
                line = dict(space=space, rows=V, dim=dim, queries=Q, top_k=k, calls=len(t_ours),
                            ms=round(t * 1e3, 4), ms_min=round(min(t_ours) * 1e3, 4), ms_max=round(max(t_ours) * 1e3, 4),
                            queries_per_s=round(Q / t, 1),
                            hbm_share=round(table_bytes / t / HBM_BYTES_PER_S, 4), tflops=round(flop / t / 1e12, 3),
                            mfma_share=round(flop / t / MFMA_F32_FLOPS, 4),
                            bound="hbm" if table_bytes / HBM_BYTES_PER_S >= flop / MFMA_F32_FLOPS else "mfma",
                            bound_ms=round(max(table_bytes / HBM_BYTES_PER_S, flop / MFMA_F32_FLOPS) * 1e3, 4),
                            baseline_ms=round(tb * 1e3, 4), baseline_ms_min=round(min(t_base) * 1e3, 4),
                            baseline_ms_max=round(max(t_base) * 1e3, 4), speedup=round(tb / t, 3),
                            same_ids_as_baseline=round(float((got[0] == ref[0]).mean()), 5))
                if with_plain:
                    d = (np.asarray(t_plain) - np.asarray(t_ours)) * 1e3
                    line.update(plain_ms=round(float(np.median(t_plain)) * 1e3, 4), plain_ms_min=round(min(t_plain) * 1e3, 4),
                                plain_ms_max=round(max(t_plain) * 1e3, 4),
                                plain_minus_ours_ms=[round(float(np.median(d)), 4), round(float(d.min()), 4), round(float(d.max()), 4)],
                                same_ids_as_plain=round(float((got[0] == got_plain[0]).mean()), 5))
                print(json.dumps(line), flush=True)
        m.close()
        del W_t, E_t, X_p, tables
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
