#!/usr/bin/env python
"""Times TF-IDF first-stage retrieval and the re-ranking of its candidates on a seeded synthetic collection.

Shape: |D| documents of Zipf-distributed tokens (lengths uniform in [1, 2 x mean - 1]) over |V| words, d_w = 300, d_e = 256, depth
and top_k 1000, queries of three words drawn from the tokens (frequent words: most queries match more documents than the depth).
Per number of queries Q, milliseconds per synchronous call on the host clock, the median of --repeats calls taken in alternation in
one process:
    tfidf      Model.tfidf_rank(top_k = depth)                      the first stage alone
    rerank     Model.rerank(depth, top_k)                           first stage, hand-over on the device, candidate scan
    composed   tfidf_rank -> host ids -> Model.rank(candidates=..)  the same result through the host (checked once: the same bits)
and once per collection the df pass (the profiler's group lex_df, inside the first TF-IDF call after the upload). One JSON line per
Q on stdout, one for the df pass. There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--documents", type=int, default=2_000_000)
    ap.add_argument("--words", type=int, default=100_000)
    ap.add_argument("--mean-length", type=int, default=50)
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--word-dim", type=int, default=300)
    ap.add_argument("--entity-dim", type=int, default=256)
    ap.add_argument("--depth", type=int, default=1000)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_rerank.py needs a GPU (MI355X): the kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    D, V, dw, de = args.documents, args.words, args.word_dim, args.entity_dim
    depth, k = min(args.depth, D), min(args.top_k, args.depth, D)

    # the collection and the tables are drawn on the device (seeded) and brought to the host, where the ABI takes them from
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    lens = torch.randint(1, 2 * args.mean_length, (D,), generator=gen, device=dev, dtype=torch.int64)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    N = int(offsets[-1])
    cdf = torch.cumsum(1.0 / torch.arange(1, V + 1, device=dev, dtype=torch.float64), 0)
    cdf /= cdf[-1].clone()
    tokens = torch.searchsorted(cdf, torch.rand(N, generator=gen, device=dev, dtype=torch.float64)).clamp_(max=V - 1).to(torch.int32)
    E = torch.randn(D, de, generator=gen, device=dev)
    W = torch.rand(V, dw, generator=gen, device=dev) - 0.5
    T = (torch.rand(de * dw, generator=gen, device=dev) * 2 - 1) * 0.2
    tokens_h, offsets_h = tokens.cpu().numpy(), offsets.cpu().numpy()
    cfg = ca.default_config(num_words=V, num_entities=D, word_repr_size=dw, entity_repr_size=de, window_size=10, num_random_entities=1,
                            batch_normalization=0, nonlinearity="tanh", update_method="sgd", max_batch_size=64, device=args.device)
    m = ca.Model(cfg)
    m.set_param("word_representations-representations", W.cpu().numpy().ravel())
    m.set_param("entity_representations-representations", E.cpu().numpy().ravel())
    m.set_param("word_entity_mapping-transform", T.cpu().numpy())
    m.set_param("word_entity_mapping-bias", np.zeros(de, np.float32))
    del E, W, T, tokens, offsets, cdf, lens
    torch.cuda.empty_cache()
    m.upload_corpus(ca.Corpus(tokens_h, offsets_h))

    rs = np.random.RandomState(21)
    m.profile_enable(True)
    t0 = time.perf_counter()
    m.tfidf_rank([[int(tokens_h[0])]], top_k=1)                              # the first call after the upload makes the df table
    first_ms = (time.perf_counter() - t0) * 1e3
    df_ms = m.profile().get("lex_df", (0.0, 0))[0]
    m.profile_enable(False)
    print(json.dumps(dict(what="df_pass", documents=D, words=V, tokens=N, lex_df_ms=df_ms, first_call_ms=first_ms)), flush=True)

    def composed(qs):
        ids, _, counts = m.tfidf_rank(qs, top_k=depth)
        return m.rank(qs, top_k=k, candidates=[ids[i, :counts[i]] for i in range(len(qs))])

    for Q in [int(x) for x in args.queries.split(",")]:
        qs = [[int(t) for t in tokens_h[rs.randint(0, N, 3)]] for _ in range(Q)]
        contenders = {"tfidf": lambda: m.tfidf_rank(qs, top_k=depth), "rerank": lambda: m.rerank(qs, depth=depth, top_k=k), "composed": lambda: composed(qs)}
        a, b = contenders["rerank"](), contenders["composed"]()               # warm-up, and the definition once
        same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        matches = m.tfidf_rank(qs, top_k=depth)[2]
        times = {name: [] for name in contenders}
        for _ in range(args.repeats):
            for name, call in contenders.items():                             # in alternation
                t0 = time.perf_counter()
                call()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = dict(what="rerank", documents=D, words=V, tokens=N, entity_dim=de, queries=Q, depth=depth, top_k=k, repeats=args.repeats,
                   same_bits=bool(same), mean_candidates=float(matches.mean()))
        for name, ms in times.items():
            row[name + "_ms"] = float(np.median(ms))
            row[name + "_ms_min"] = float(np.min(ms))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
