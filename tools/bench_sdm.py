#!/usr/bin/env python
"""Times nvsm_sdm_rank against nvsm_lexical_rank on the same seeded synthetic Zipf collection and the same queries.

Per shape (|D| documents of 1 .. 2·mean_len tokens over |V| words, Q queries of five ADJACENT tokens of the collection — so that their
pairs occur —, top k = 1000): milliseconds per synchronous call on the host clock for both calls, in the same process, call by call in
alternation; the ratio; queries/s; and the arena bytes (4 per token) the sequential-dependence call reads — TWO passes a round, the
collection counts and the scores — over its time, as a share of the 6.29 TB/s HBM delivers. Every shape is warmed up and timed for
at least --seconds of work per call. One JSON line per shape on stdout. No threshold is attached. There is no CPU fallback: without a
GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--mean-len", type=int, default=200)
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--method", default="dirichlet")
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and call")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np

    import cunvsm_amd as ca
    if ca.device_count() < 1:
        sys.exit("bench_sdm.py needs a GPU (MI355X): the lexical kernels have no CPU fallback")
    D, V, k = args.docs, args.words, min(args.top_k, args.docs)
    rs = np.random.RandomState(11)
    lens = rs.randint(1, 2 * args.mean_len + 1, D)
    p = 1.0 / np.arange(1, V + 1)
    p /= p.sum()
    tokens = rs.choice(V, size=int(lens.sum()), p=p).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = tokens.size
    cfg = ca.default_config(num_words=V, num_entities=D, word_repr_size=8, entity_repr_size=8, window_size=2, num_random_entities=1,
                            batch_normalization=0, nonlinearity="tanh", update_method="sgd", max_batch_size=8, device=args.device)
    m = ca.Model(cfg)
    m.upload_corpus(ca.Corpus(tokens, offsets))

    for Q in [int(x) for x in args.queries.split(",")]:
        starts = rs.randint(0, N - 5, Q)
        queries = [[int(t) for t in tokens[s:s + 5]] for s in starts]
        distinct = len({t for q in queries for t in q})
        pairs = len({(q[j], q[j + 1]) for q in queries for j in range(4)})
        rounds = max(1, -(-Q // 256), -(-distinct // 1024), -(-pairs // 1024))      # a lower bound

        def sdm():
            t0 = time.perf_counter()
            out = m.sdm_rank(queries, method=args.method, top_k=k, window=args.window)
            return time.perf_counter() - t0, out

        def unigram():
            t0 = time.perf_counter()
            out = m.lexical_rank(queries, method=args.method, top_k=k)
            return time.perf_counter() - t0, out

        for _ in range(2):
            sdm()
            unigram()
        t_sdm, t_uni = [], []
        while sum(t_sdm) < args.seconds or sum(t_uni) < args.seconds or len(t_sdm) < 5:
            dt, got = sdm()
            t_sdm.append(dt)
            dt, ref = unigram()
            t_uni.append(dt)
        t, tu = float(np.median(t_sdm)), float(np.median(t_uni))
        line = dict(docs=D, words=V, tokens=int(N), queries=Q, top_k=k, method=args.method, window=args.window, calls=len(t_sdm),
                    distinct_terms=distinct, distinct_pairs=pairs, rounds_at_least=rounds,
                    sdm_ms=round(t * 1e3, 4), sdm_ms_min=round(min(t_sdm) * 1e3, 4), sdm_ms_max=round(max(t_sdm) * 1e3, 4),
                    lexical_ms=round(tu * 1e3, 4), lexical_ms_min=round(min(t_uni) * 1e3, 4), lexical_ms_max=round(max(t_uni) * 1e3, 4),
                    sdm_over_lexical=round(t / tu, 3), queries_per_s=round(Q / t, 1), arena_bytes_per_pass=int(4 * N),
                    hbm_share=round(rounds * 2 * 4.0 * N / t / HBM_BYTES_PER_S, 5),
                    same_counts_as_lexical=bool((got[2] == ref[2]).all()))
        print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main()
