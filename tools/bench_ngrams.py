#!/usr/bin/env python
"""Times nvsm_ngram_search against the plumbing baseline on seeded synthetic tables.

Per shape (a vocabulary of m words out of |V| = max(m, 1000), d_w = 300, d_e = 256, 1- and 2-grams, top k = 20, Q queries given as
vectors of document space): milliseconds per synchronous call on the host clock, phrase rows per second, and the bytes the call
moves through the phrase slab (every row is written once by the generator and read once by the scan: 2·R·d_e·4) over the time as a
share of the 6.29 TB/s HBM delivers. In the same process, call by call in alternation, the same search as ONE PyTorch-ROCm
expression on resident tensors —
    G = W[S] @ T;  X = tanh(cat(G, 0.5·(G[a] + G[b])) + b);  topk(normalize(P) @ normalize(X).T, k)
plus the copy of its results to the host — wherever its intermediates (about 3·R·d_e·4 bytes) fit --baseline-gb; beyond that the
baseline columns are null. Every shape is warmed up and timed for at least --seconds of work per contender. One JSON line per shape
on stdout. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--words", default="500,2000,8000", help="m: words of the searched vocabulary")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--word-dim", type=int, default=300)
    ap.add_argument("--entity-dim", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and contender")
    ap.add_argument("--baseline-gb", type=float, default=48.0, help="largest PyTorch expression that is still run")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_ngrams.py needs a GPU (MI355X): the n-gram kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    dw, de = args.word_dim, args.entity_dim
    normalize = torch.nn.functional.normalize

    for m_words in [int(x) for x in args.words.split(",")]:
        V = max(m_words, 1000)
        R = ca.ngram_rows(m_words, 2)
        if R < 0:
            sys.exit("bench_ngrams.py: %d words reach the row limit" % m_words)
        k = min(args.top_k, R)
        rs = np.random.RandomState(4321 + m_words)
        W = rs.uniform(-0.5, 0.5, (V, dw)).astype(np.float32)
        T = (rs.uniform(-1, 1, de * dw) * 0.2).astype(np.float32)
        b = rs.uniform(-0.1, 0.1, de).astype(np.float32)
        voc = np.sort(rs.choice(V, m_words, replace=False)).astype(np.int64)
        cfg = ca.default_config(num_words=V, num_entities=8, word_repr_size=dw, entity_repr_size=de, window_size=10,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=64, device=args.device)
        m = ca.Model(cfg)
        m.set_param("word_representations-representations", W)
        m.set_param("word_entity_mapping-transform", T)
        m.set_param("word_entity_mapping-bias", b)
        W_t, T_t, b_t = torch.from_numpy(W).to(dev), torch.from_numpy(T.reshape(dw, de)).to(dev), torch.from_numpy(b).to(dev)
        voc_t = torch.from_numpy(voc).to(dev)
        with_baseline = 3.0 * R * de * 4 <= args.baseline_gb * 2 ** 30
        pairs = torch.triu_indices(m_words, m_words, 1, device=dev) if with_baseline else None      # combinations order
        for Q in [int(x) for x in args.queries.split(",")]:
            P = rs.standard_normal((Q, de)).astype(np.float32)
            P_t = torch.from_numpy(P).to(dev)

            def ours():
                t0 = time.perf_counter()
                out = m.nearest_ngrams(vectors=P, vocabulary=voc, max_cardinality=2, top_k=k)
                return time.perf_counter() - t0, out

            def baseline():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                G = W_t[voc_t] @ T_t
                X = torch.tanh(torch.cat([G, 0.5 * (G[pairs[0]] + G[pairs[1]])]) + b_t)
                v, i = torch.topk(normalize(P_t, dim=1) @ normalize(X, dim=1).T, k, dim=1)
                v, i = v.cpu(), i.cpu()                                      # host results, as nvsm_ngram_search returns them
                return time.perf_counter() - t0, (i.numpy(), v.numpy())

            for _ in range(2):
                ours()
                if with_baseline:
                    baseline()
            t_ours, t_base, ref = [], [], None
            while sum(t_ours) < args.seconds or len(t_ours) < 3 or (with_baseline and sum(t_base) < args.seconds):
                dt, got = ours()
                t_ours.append(dt)
                if with_baseline:
                    dt, ref = baseline()
                    t_base.append(dt)
            t = float(np.median(t_ours))
            slab_bytes = 2.0 * R * de * 4
            line = dict(words=m_words, phrase_rows=R, dim=de, queries=Q, top_k=k, calls=len(t_ours),
                        ms=round(t * 1e3, 4), ms_min=round(min(t_ours) * 1e3, 4), ms_max=round(max(t_ours) * 1e3, 4),
                        rows_per_s=round(R / t, 1), hbm_share=round(slab_bytes / t / HBM_BYTES_PER_S, 4),
                        baseline_ms=None, baseline_ms_min=None, baseline_ms_max=None, speedup=None, same_rows_as_baseline=None)
            if with_baseline:
                tb = float(np.median(t_base))
                line.update(baseline_ms=round(tb * 1e3, 4), baseline_ms_min=round(min(t_base) * 1e3, 4),
                            baseline_ms_max=round(max(t_base) * 1e3, 4), speedup=round(tb / t, 3),
                            same_rows_as_baseline=round(float((got[0] == ref[0]).mean()), 5))
            print(json.dumps(line), flush=True)
        m.close()
        del W_t, pairs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
