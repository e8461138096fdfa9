#!/usr/bin/env python
"""Times nvsm_lexical_rank_prf next to nvsm_lexical_rank on the seeded synthetic Zipf collection of tools/bench_lexical.py
(DESIGN.md §16).

Per shape (|D| documents of 1 .. 2·mean_len tokens over |V| words, Q queries of five words drawn from the collection's tokens,
top k = 1000, Jelinek-Mercer with the automatic parameter, feedback from 10 documents with 10 terms and original weight 0.5):
milliseconds per synchronous call on the host clock of the two calls, timed call by call in alternation in one process, their ratio,
and the parts of the feedback call that can be timed alone — the relevance model (first pass at top_k = fb_docs, accumulation and
selection over the vocabulary) and the weighted ranking of the expanded queries. The expectation to hold the ratio against: two scoring
passes plus a selection over the vocabulary, the second pass with about three times the terms and so, at Q = 256, three to four times
the rounds. One JSON line per shape on stdout and in profiles/prf_bench.jsonl. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--mean-len", type=int, default=200)
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--method", default="jm")
    ap.add_argument("--fb-docs", type=int, default=10)
    ap.add_argument("--fb-terms", type=int, default=10)
    ap.add_argument("--orig-weight", type=float, default=0.5)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and call")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prf_bench.jsonl"))
    args = ap.parse_args()

    import numpy as np

    import cunvsm_amd as ca
    if ca.device_count() < 1:
        sys.exit("bench_prf.py needs a GPU (MI355X): the lexical kernels have no CPU fallback")
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
    fb = dict(fb_docs=args.fb_docs, fb_terms=args.fb_terms)
    lines = []

    for Q in [int(x) for x in args.queries.split(",")]:
        queries = [[int(t) for t in tokens[rs.randint(0, N, 5)]] for _ in range(Q)]

        def timed(call):
            t0 = time.perf_counter()
            out = call()
            return time.perf_counter() - t0, out

        plain = lambda: m.lexical_rank(queries, method=args.method, top_k=k)
        prf = lambda: m.lexical_rank_prf(queries, orig_weight=args.orig_weight, method=args.method, top_k=k, **fb)
        model = lambda: m.relevance_model(queries, method=args.method, **fb)
        for _ in range(2):
            plain()
            prf()
        t_plain, t_prf = [], []
        while sum(t_plain) < args.seconds or sum(t_prf) < args.seconds or len(t_prf) < 5:
            t_prf.append(timed(prf)[0])
            t_plain.append(timed(plain)[0])
        # the parts, timed alone: the relevance model, and the weighted ranking of the queries it expands to
        _, (ids, probs, counts) = timed(model)
        t_model = [timed(model)[0] for _ in range(5)]
        xq, xw = [], []
        for i, q in enumerate(queries):      # (every query word occurs in the collection: L = len(q))
            n = int(counts[i])
            pi = probs[i, :n].astype(np.float64)
            xq.append(list(q) + [int(t) for t in ids[i, :n]])
            xw.append([np.float32(args.orig_weight / len(q))] * len(q) + [np.float32((1.0 - args.orig_weight) * x / pi.sum()) for x in pi])
        weighted = lambda: m.lexical_rank(xq, method=args.method, top_k=k, weights=xw)
        weighted()
        t_weighted = [timed(weighted)[0] for _ in range(5)]
        distinct = len({t for q in queries for t in q})
        distinct_expanded = len({t for q in xq for t in q})
        med = lambda ts: float(np.median(ts))
        line = dict(docs=D, words=V, tokens=int(N), queries=Q, top_k=k, method=args.method, fb_docs=args.fb_docs, fb_terms=args.fb_terms,
                    orig_weight=args.orig_weight, calls=len(t_prf),
                    prf_ms=round(med(t_prf) * 1e3, 4), prf_ms_min=round(min(t_prf) * 1e3, 4), prf_ms_max=round(max(t_prf) * 1e3, 4),
                    plain_ms=round(med(t_plain) * 1e3, 4), plain_ms_min=round(min(t_plain) * 1e3, 4), plain_ms_max=round(max(t_plain) * 1e3, 4),
                    ratio=round(med(t_prf) / med(t_plain), 3),
                    relevance_model_ms=round(med(t_model) * 1e3, 4), weighted_ms=round(med(t_weighted) * 1e3, 4),
                    distinct_terms=distinct, distinct_terms_expanded=distinct_expanded,
                    rounds_at_least=max(1, -(-Q // 256), -(-distinct // 1024)),
                    rounds_expanded_at_least=max(1, -(-Q // 256), -(-distinct_expanded // 1024)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
