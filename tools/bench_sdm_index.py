#!/usr/bin/env python
"""Times sequential-dependence ranking served from the positional postings against the arena scan.

On the two collections of tools/bench_index.py (100 000 documents / 2·10⁷ tokens / V = 50 000 and 2·10⁶ documents / 10⁸ tokens /
V = 100 000, seeded Zipf tokens drawn on the device): the positional layer's build (milliseconds of the synchronous call, its bytes,
its peak build scratch), then per Q in {1, 8, 16, 32, 64, 128, 256}, queries of five ADJACENT tokens of the collection, Dirichlet
smoothing at its automatic parameter, W = 8, k = 1000, sdm_rank under "never", "always" and "auto". The three are called one by one
in alternation in one process; per contender the median, minimum and maximum of --repeats synchronous calls on the host clock. Every
cell asserts that the three returned the same bits. One JSON line per cell on stdout and appended to --out. There is no CPU fallback:
without a GPU the tool fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLLECTIONS = {"100k": (100_000, 50_000, 200), "2m": (2_000_000, 100_000, 50)}      # documents, words, mean length
USES = ("never", "always", "auto")
WINDOW = 8


def build_scratch_bytes(num_tokens, num_postings, num_words):
    """what nvsm_corpus_index_positions holds beside the layer while it builds (ranking.cpp positions_build): the sorted tokens and
    their documents with either the sort's workspace or the scan's and its discarded outputs"""
    pad = lambda b: (b + 255) // 256 * 256
    pairs = 2 * 4 * num_tokens
    sort_ws = 256 + 4 * 128 * 512 + 2 * pad(4 * num_tokens)
    scan_ws = 4 * ((num_tokens + 2047) // 2048 + 1) + 4 * num_postings + 2 * 8 * (num_words + 1)
    return pairs + max(sort_ws, scan_ws)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--collection", default="100k", choices=sorted(COLLECTIONS))
    ap.add_argument("--queries", default="1,8,16,32,64,128,256")
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdm_index_bench.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_sdm_index.py needs a GPU (MI355X): the kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    D, V, mean_len = COLLECTIONS[args.collection]
    k = min(args.top_k, D)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    lens = torch.randint(1, 2 * mean_len, (D,), generator=gen, device=dev, dtype=torch.int64)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    N = int(offsets[-1])
    cdf = torch.cumsum(1.0 / torch.arange(1, V + 1, device=dev, dtype=torch.float64), 0)
    cdf /= cdf[-1].clone()
    tokens = torch.searchsorted(cdf, torch.rand(N, generator=gen, device=dev, dtype=torch.float64)).clamp_(max=V - 1).to(torch.int32)
    tokens_h, offsets_h = tokens.cpu().numpy(), offsets.cpu().numpy()
    del tokens, offsets, cdf, lens
    torch.cuda.empty_cache()
    cfg = ca.default_config(num_words=V, num_entities=D, word_repr_size=8, entity_repr_size=8, window_size=2, num_random_entities=1,
                            batch_normalization=0, nonlinearity="tanh", update_method="sgd", max_batch_size=8, device=args.device)
    m = ca.Model(cfg)
    m.upload_corpus(ca.Corpus(tokens_h, offsets_h))
    out = open(args.out, "a")

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    info = m.index_corpus("never")
    t0 = time.perf_counter()
    layer = m.index_positions()
    build_ms = (time.perf_counter() - t0) * 1e3
    emit(dict(what="build", collection=args.collection, documents=D, words=V, tokens=N, build_ms=round(build_ms, 3),
              num_postings=info["num_postings"], index_bytes=info["bytes"], positions_bytes=layer["bytes"], arena_bytes=4 * N,
              build_scratch_bytes=build_scratch_bytes(N, info["num_postings"], V)))

    cf = np.bincount(tokens_h, minlength=V)

    def df_of(word):      # the count alone: capacity 0 copies nothing
        n = C.c_int64()
        ca.lib().nvsm_corpus_postings(m._h, int(word), 0, None, None, C.byref(n))
        return n.value

    def postings_work(qs):
        """what "auto" looks at (ranking.cpp sdm_rounds): the occurrences the round's distinct pairs merge, and per query the postings
        of its distinct words times its members (a word, and the pair it opens in O and in U)"""
        pairs = {(q[i], q[i + 1]) for q in qs for i in range(len(q) - 1)}
        work = sum(int(cf[a]) + int(cf[b]) for a, b in pairs)
        for q in qs:
            work += sum(df_of(t) for t in set(q)) * (len(q) + 2 * max(len(q) - 1, 0))
        return work

    rs = np.random.RandomState(21)
    long_enough = np.flatnonzero(np.diff(offsets_h) >= 5)
    for Q in [int(x) for x in args.queries.split(",")]:
        qs = []
        for d in long_enough[rs.randint(0, long_enough.size, Q)]:      # five adjacent tokens of one document
            s = offsets_h[d] + rs.randint(0, offsets_h[d + 1] - offsets_h[d] - 4)
            qs.append([int(t) for t in tokens_h[s:s + 5]])
        work = postings_work(qs)
        times, last = {u: [] for u in USES}, {}

        def timed(use):
            m.index_corpus(use)                    # (an indexed corpus: only sets `use`; outside the clock)
            t0 = time.perf_counter()
            res = m.sdm_rank(qs, method="dirichlet", top_k=k, window=WINDOW)
            return time.perf_counter() - t0, res

        for u in USES:                             # warm-up: scratch grown, cf made
            timed(u)
        m.profile_enable(True)
        m.profile_reset()
        timed("auto")
        auto_took = "postings" if any(n.startswith("sdm_postings") and c > 0 for n, (_, c) in m.profile().items()) else "scan"
        m.profile_enable(False)
        for _ in range(args.repeats):
            for u in USES:
                dt, last[u] = timed(u)
                times[u].append(dt)
        same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for u in USES[1:] for a, b in zip(last["never"], last[u]))
        line = dict(what="sdm_rank", collection=args.collection, documents=D, tokens=N, queries=Q, top_k=k, window=WINDOW, repeats=args.repeats,
                    postings_work=int(work), work_per_token=round(work / N, 4), auto_took=auto_took, same_bits=bool(same))
        for u in USES:
            line[u + "_ms"] = round(float(np.median(times[u])) * 1e3, 4)
            line[u + "_ms_min"] = round(min(times[u]) * 1e3, 4)
            line[u + "_ms_max"] = round(max(times[u]) * 1e3, 4)
        line["always_speedup"] = round(line["never_ms"] / line["always_ms"], 3)
        line["auto_within_never_range"] = bool(line["auto_ms"] <= line["never_ms_max"])
        emit(line)
        assert same, "the three uses returned different bits at Q = %d" % Q
    out.close()
    m.close()


if __name__ == "__main__":
    main()
