#!/usr/bin/env python
"""Times the alpha sweep of supervised run fusion on the seeded synthetic Zipf collection of tools/bench_lexical.py.

|D| documents of 1 .. 2·mean_len tokens over |V| words, Q queries of five words drawn from the collection's tokens, synthetic
judgments (per query --judged documents with grades 0 .. 2), top k = 1000, Jelinek-Mercer with the automatic parameter, the grid
0, step, 2·step, ... < 1. Two contenders, synchronous calls on the host clock, alternated call by call in one process:
  loop   what a caller writes without the sweep: one rank_ensemble(alpha, judgments) per grid point
  sweep  one ensemble_sweep over the grid
The metric tables of the two are compared bit for bit. A further sweep with the profiler on gives the share of the fuse_sweep scope
(HIP events around the launch) in that call's host time. One JSON line on stdout. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--words", type=int, default=50000)
    ap.add_argument("--mean-len", type=int, default=200)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--stepsize", type=float, default=0.01)
    ap.add_argument("--depth", type=int, default=0)
    ap.add_argument("--judged", type=int, default=50)
    ap.add_argument("--calls", type=int, default=9, help="timed calls per contender")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np

    import cunvsm_amd as ca
    if ca.device_count() < 1:
        sys.exit("bench_fusion_cv.py needs a GPU (MI355X): the fusion kernels have no CPU fallback")
    D, V, Q, k = args.docs, args.words, args.queries, min(args.top_k, args.docs)
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
    m.initialize(3)
    m.upload_corpus(ca.Corpus(tokens, offsets))
    queries = [[int(t) for t in tokens[rs.randint(0, N, 5)]] for _ in range(Q)]
    judged = ca.Judgments([list(zip(rs.choice(D, args.judged, replace=False).tolist(), rs.randint(0, 3, args.judged).tolist())) for _ in range(Q)])
    grid = ca.alpha_grid(args.stepsize)

    def loop():
        t0 = time.perf_counter()
        rows = [m.rank_ensemble(queries, alpha=float(a), judgments=judged, top_k=k)[0] for a in grid]
        return time.perf_counter() - t0, rows

    def sweep():
        t0 = time.perf_counter()
        table = m.ensemble_sweep(queries, judged, grid, depth=args.depth, top_k=k)
        return time.perf_counter() - t0, table

    m.rank_ensemble(queries, alpha=0.5, judgments=judged, top_k=k)      # warm-up: scratch, the cf table
    sweep()
    t_loop, t_sweep = [], []
    for _ in range(args.calls):
        dt, rows = loop()
        t_loop.append(dt)
        dt, table = sweep()
        t_sweep.append(dt)
    same = args.depth != 0 or all((table[name][a].view(np.uint64) == rows[a][name].view(np.uint64)).all()
                                  for a in range(grid.size) for name in table)
    m.profile_enable(True)
    m.profile_reset()
    dt, _ = sweep()
    prof = m.profile()
    m.profile_enable(False)
    tl, ts = float(np.median(t_loop)), float(np.median(t_sweep))
    line = dict(docs=D, words=V, tokens=int(N), queries=Q, top_k=k, alphas=int(grid.size), stepsize=args.stepsize, depth=args.depth,
                judged_per_query=args.judged, calls=args.calls,
                loop_ms=round(tl * 1e3, 2), loop_ms_min=round(min(t_loop) * 1e3, 2), loop_ms_max=round(max(t_loop) * 1e3, 2),
                sweep_ms=round(ts * 1e3, 2), sweep_ms_min=round(min(t_sweep) * 1e3, 2), sweep_ms_max=round(max(t_sweep) * 1e3, 2),
                loop_over_sweep=round(tl / ts, 2), same_bits_as_loop=bool(same),
                profiled_sweep_ms=round(dt * 1e3, 2), fuse_sweep_ms=round(prof["fuse_sweep"][0], 3), fuse_sweep_launches=int(prof["fuse_sweep"][1]),
                fuse_sweep_share=round(prof["fuse_sweep"][0] / (dt * 1e3), 4),
                map_by_alpha_min=float(table["map"].mean(1).min()), map_by_alpha_max=float(table["map"].mean(1).max()))
    print(json.dumps(line), flush=True)
    m.close()


if __name__ == "__main__":
    main()
