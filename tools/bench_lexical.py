#!/usr/bin/env python
"""Times nvsm_lexical_rank on a seeded synthetic Zipf collection of the headline size.

Per shape (|D| documents of 1 .. 2·mean_len tokens over |V| words, Q queries of five words drawn from the collection's tokens,
top k = 1000, Jelinek-Mercer with the automatic parameter): milliseconds per synchronous call on the host clock, queries/s, the
rounds the call takes, and the arena bytes (4 per token) of ONE pass over the collection times the rounds, over the time, as a share
of the 6.29 TB/s HBM delivers. In the same process, call by call in alternation, the same scores as one PyTorch-ROCm formulation on
resident tensors: per query word, tf = bincount(doc_of[tokens == word]) and the fp64 log of the smoothed probability, summed per
query, -inf where no word matched, torch.topk. Every shape is warmed up and timed for at least --seconds of work per contender.
One JSON line per shape on stdout. There is no CPU fallback: without a GPU the tool fails."""
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
    ap.add_argument("--method", default="jm")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and contender")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_lexical.py needs a GPU (MI355X): the lexical kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
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
    tok_t = torch.from_numpy(tokens.astype(np.int64)).to(dev)
    doc_of = torch.repeat_interleave(torch.arange(D, device=dev), torch.from_numpy(lens).to(dev))
    len_t = torch.from_numpy(lens.astype(np.float64)).to(dev)
    cf = np.bincount(tokens, minlength=V)
    lam = 0.5
    mu = N / D

    for Q in [int(x) for x in args.queries.split(",")]:
        queries = [[int(t) for t in tokens[rs.randint(0, N, 5)]] for _ in range(Q)]
        distinct = len({t for q in queries for t in q})
        rounds = max(1, -(-Q // 256), -(-distinct // 1024))                # a lower bound: 256 queries and 1024 distinct words a round

        def ours():
            t0 = time.perf_counter()
            out = m.lexical_rank(queries, method=args.method, top_k=k)
            return time.perf_counter() - t0, out

        def baseline():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            scores = torch.zeros((Q, D), dtype=torch.float64, device=dev)
            matched = torch.zeros((Q, D), dtype=torch.bool, device=dev)
            tf_of = {}
            for i, q in enumerate(queries):
                for t in q:
                    if t not in tf_of:
                        tf_of[t] = torch.bincount(doc_of[tok_t == t], minlength=D).to(torch.float64)
                    tf, pt = tf_of[t], cf[t] / N
                    scores[i] += torch.log((1 - lam) * tf / len_t + lam * pt) if args.method == "jm" else torch.log((tf + mu * pt) / (len_t + mu))
                    matched[i] |= tf > 0
            scores = torch.where(matched, scores, torch.full_like(scores, float("-inf"))).to(torch.float32)
            vals, idx = torch.topk(scores, k, dim=1)
            vals, idx = vals.cpu(), idx.cpu()
            return time.perf_counter() - t0, (idx.numpy(), vals.numpy())

        for _ in range(2):
            ours()
            baseline()
        t_ours, t_base = [], []
        while sum(t_ours) < args.seconds or sum(t_base) < args.seconds or len(t_ours) < 5:
            dt, got = ours()
            t_ours.append(dt)
            dt, ref = baseline()
            t_base.append(dt)
        finite = np.isfinite(ref[1]) & np.isfinite(got[1])
        err = float(np.abs(got[1][finite].astype(np.float64) - ref[1][finite]).max()) if finite.any() else 0.0
        t, tb = float(np.median(t_ours)), float(np.median(t_base))
        line = dict(docs=D, words=V, tokens=int(N), queries=Q, top_k=k, method=args.method, calls=len(t_ours), distinct_terms=distinct,
                    rounds_at_least=rounds, ms=round(t * 1e3, 4), ms_min=round(min(t_ours) * 1e3, 4), ms_max=round(max(t_ours) * 1e3, 4),
                    queries_per_s=round(Q / t, 1), arena_bytes_per_pass=int(4 * N),
                    hbm_share=round(rounds * 4.0 * N / t / HBM_BYTES_PER_S, 5),
                    baseline_ms=round(tb * 1e3, 4), baseline_ms_min=round(min(t_base) * 1e3, 4), baseline_ms_max=round(max(t_base) * 1e3, 4),
                    speedup=round(tb / t, 3), same_counts_as_baseline=bool((np.isfinite(ref[1]).sum(1) == got[2].clip(max=k)).all()),
                    max_score_difference=err)
        print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main()
