#!/usr/bin/env python
"""Times nvsm_evaluate against what it replaces on seeded synthetic tables.

Per shape (|D| documents, d_e = 256, top k = 1000, Q queries of five words, 50 judged documents per query): milliseconds per
synchronous call on the host clock of
  evaluate   Model.evaluate: the ranking and the metrics in one call, only the metric rows come back from the device
  rank+numpy Model.rank (Q x k ids and scores come back) followed by the fp64 numpy metrics of tests/eval_reference.py
  rank       Model.rank alone — what the metrics cost on top is evaluate - rank
in the same process, call by call in alternation. Every shape is warmed up and timed for at least --seconds of work per
contender. One JSON line per shape on stdout; `max_abs_diff` is the largest difference between the two sets of metrics.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CUTOFFS = (5, 10, 20, 100, 1000)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", default="100000,2000000")
    ap.add_argument("--queries", default="16,256,4096")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--judged", type=int, default=50, help="judged documents per query")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and contender")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np

    import cunvsm_amd as ca
    from tests import eval_reference as er
    if ca.device_count() < 1:
        sys.exit("bench_eval.py needs a GPU (MI355X): the ranking and metric kernels have no CPU fallback")
    de, k = args.dim, args.top_k
    num_words, dw, words_per_query = 50000, 300, 5

    for D in [int(x) for x in args.docs.split(",")]:
        kk = min(k, D)
        rng = np.random.default_rng(1234 + D)
        rs = np.random.RandomState(7)
        cfg = ca.default_config(num_words=num_words, num_entities=D, word_repr_size=dw, entity_repr_size=de, window_size=10,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=64, device=args.device)
        m = ca.Model(cfg)
        m.set_param("word_representations-representations", rs.uniform(-1, 1, num_words * dw).astype(np.float32))
        m.set_param("word_entity_mapping-transform", (rs.uniform(-1, 1, de * dw) * 0.2).astype(np.float32))
        m.set_param("word_entity_mapping-bias", rs.uniform(-0.1, 0.1, de).astype(np.float32))
        m.set_param("entity_representations-representations", rng.random((D, de), dtype=np.float32) - 0.5)
        for Q in [int(x) for x in args.queries.split(",")]:
            queries = ca.Queries([rs.randint(0, num_words, words_per_query) for _ in range(Q)])
            # half of every query's judged documents come from its own top k, so that the metrics are not all zero
            top = m.rank(queries, top_k=kk)[0]
            judged = []
            for q in range(Q):
                n = min(args.judged, D)
                hit = rs.choice(top[q], min(n // 2, kk), replace=False)
                rest = np.setdiff1d(rs.randint(0, D, 2 * n), hit)[:n - hit.size]
                ids = np.concatenate([hit, rest])
                judged.append(np.stack([ids, rs.randint(0, 4, ids.size)], 1))
            judgments = ca.Judgments(judged)

            def evaluate():
                t0 = time.perf_counter()
                out = m.evaluate(queries, judgments, top_k=kk, cutoffs=CUTOFFS)
                return time.perf_counter() - t0, out

            def rank_numpy():
                t0 = time.perf_counter()
                ids, scores, counts = m.rank(queries, top_k=kk)
                out = er.evaluate(ids, counts, judged, CUTOFFS)
                return time.perf_counter() - t0, out

            def rank_alone():
                t0 = time.perf_counter()
                m.rank(queries, top_k=kk)
                return time.perf_counter() - t0, None

            contenders = (evaluate, rank_numpy, rank_alone)
            for _ in range(2):
                for f in contenders:
                    f()
            times = [[], [], []]
            outs = [None, None, None]
            while min(sum(t) for t in times) < args.seconds or len(times[0]) < 5:
                for i, f in enumerate(contenders):
                    dt, outs[i] = f()
                    times[i].append(dt)
            diff = max(float(np.abs(outs[0][name] - outs[1][name]).max()) for name in outs[0])
            med = [float(np.median(t)) for t in times]
            line = dict(docs=D, dim=de, queries=Q, top_k=kk, judged=args.judged, calls=len(times[0]),
                        evaluate_ms=round(med[0] * 1e3, 4), evaluate_ms_min=round(min(times[0]) * 1e3, 4), evaluate_ms_max=round(max(times[0]) * 1e3, 4),
                        rank_numpy_ms=round(med[1] * 1e3, 4), rank_numpy_ms_min=round(min(times[1]) * 1e3, 4),
                        rank_numpy_ms_max=round(max(times[1]) * 1e3, 4),
                        rank_ms=round(med[2] * 1e3, 4), rank_ms_min=round(min(times[2]) * 1e3, 4), rank_ms_max=round(max(times[2]) * 1e3, 4),
                        metrics_on_top_ms=round((med[0] - med[2]) * 1e3, 4), speedup_over_rank_numpy=round(med[1] / med[0], 3),
                        result_bytes_evaluate=Q * 8 * (7 + 3 * len(CUTOFFS)), result_bytes_rank=Q * kk * 12 + Q * 8,
                        max_abs_diff=diff, mean_map=round(float(outs[0]["map"].mean()), 4))
            print(json.dumps(line), flush=True)
        m.close()


if __name__ == "__main__":
    main()
