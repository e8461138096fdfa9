#!/usr/bin/env python
"""Times nvsm_rank against the plumbing baseline on seeded synthetic tables.

Per shape (|D| documents, d_e = 256, top k = 1000, Q queries of five words): milliseconds per synchronous call on the host
clock, queries/s, the algorithmic table bytes (|D|·d_e·4) over the time as a share of the 6.29 TB/s HBM delivers, the
2·Q·|D|·d_e FLOP over the time as a share of the 157 TFLOP/s of the exact-fp32 matrix pipe, and which of the two bounds
the shape. In the same process, call by call in alternation, the same ranking as ONE PyTorch-ROCm expression on resident
tensors: torch.topk(normalize(P) @ normalize(E).T, k) (chunked over the queries only if that does not fit).
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
    ap.add_argument("--docs", default="100000,2000000")
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per shape and contender")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_rank.py needs a GPU (MI355X): the ranking kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    de, k = args.dim, args.top_k
    num_words, dw, words_per_query = 50000, 300, 5

    for D in [int(x) for x in args.docs.split(",")]:
        kk = min(k, D)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234 + D)
        E_t = torch.rand((D, de), generator=gen, device=dev, dtype=torch.float32) - 0.5
        rs = np.random.RandomState(7)
        cfg = ca.default_config(num_words=num_words, num_entities=D, word_repr_size=dw, entity_repr_size=de, window_size=10,
                                num_random_entities=1, batch_normalization=0, nonlinearity="tanh", update_method="sgd",
                                max_batch_size=64, device=args.device)
        m = ca.Model(cfg)
        m.set_param("word_representations-representations", rs.uniform(-1, 1, num_words * dw).astype(np.float32))
        m.set_param("word_entity_mapping-transform", (rs.uniform(-1, 1, de * dw) * 0.2).astype(np.float32))
        m.set_param("word_entity_mapping-bias", rs.uniform(-0.1, 0.1, de).astype(np.float32))
        m.set_param("entity_representations-representations", E_t.cpu().numpy())
        for Q in [int(x) for x in args.queries.split(",")]:
            queries = [rs.randint(0, num_words, words_per_query) for _ in range(Q)]
            P_t = torch.from_numpy(m.infer(queries)).to(dev)

            def ours():
                t0 = time.perf_counter()
                out = m.rank(queries, top_k=kk)
                return time.perf_counter() - t0, out

            def baseline():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                En = torch.nn.functional.normalize(E_t, dim=1)
                Pn = torch.nn.functional.normalize(P_t, dim=1)
                chunk = max(1, min(Q, (8 << 30) // (4 * D)))              # the score matrix of a chunk: at most 8 GB
                vals, idx = [], []
                for q0 in range(0, Q, chunk):
                    v, i = torch.topk(Pn[q0:q0 + chunk] @ En.T, kk, dim=1)
                    vals.append(v)
                    idx.append(i)
                vals, idx = torch.cat(vals).cpu(), torch.cat(idx).cpu()      # host results, as nvsm_rank returns them
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
            same = float((got[0] == ref[0]).mean())
            t = float(np.median(t_ours))
            tb = float(np.median(t_base))
            table_bytes, flop = D * de * 4.0, 2.0 * Q * D * de
            line = dict(docs=D, dim=de, queries=Q, top_k=kk, calls=len(t_ours),
                        ms=round(t * 1e3, 4), ms_min=round(min(t_ours) * 1e3, 4), ms_max=round(max(t_ours) * 1e3, 4),
                        queries_per_s=round(Q / t, 1),
                        hbm_share=round(table_bytes / t / HBM_BYTES_PER_S, 4), tflops=round(flop / t / 1e12, 3),
                        mfma_share=round(flop / t / MFMA_F32_FLOPS, 4),
                        bound="hbm" if table_bytes / HBM_BYTES_PER_S >= flop / MFMA_F32_FLOPS else "mfma",
                        bound_ms=round(max(table_bytes / HBM_BYTES_PER_S, flop / MFMA_F32_FLOPS) * 1e3, 4),
                        baseline_ms=round(tb * 1e3, 4), baseline_ms_min=round(min(t_base) * 1e3, 4),
                        baseline_ms_max=round(max(t_base) * 1e3, 4), speedup=round(tb / t, 3), same_ids_as_baseline=round(same, 5))
            print(json.dumps(line), flush=True)
        m.close()
        del E_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
