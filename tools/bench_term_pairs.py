#!/usr/bin/env python
"""Times the term-mixed step (nvsm_step_term_mixed: text objective + term-term pairs on the words table) against the text-only step
(nvsm_step) of the SAME process and handle, in alternating timed regions, and the words-table pair kernel alone.

Shapes: the headline shape (|V| = 50 k, |D| = 100 k, 300 -> 256, window 10, 16 negatives, 51 200 windows, batch-norm + hard_tanh)
with M in {1 024, 6 400, 51 200} pairs, and the LSE shape (|V| = 200 k, 128 -> 256, 4 096 windows, tanh, no batch-norm) with
M = 4 096. Pair ids are drawn from the batch's Zipf(1) word distribution (hot words sit in many pairs). The reference refuses the
mixed objective for sparse Adam and Adagrad (the two shapes' usual optimisers), so the headline shape runs dense_adam and the LSE shape
sgd here — for BOTH contenders. Batches are resident in HBM.
Per shape one JSON line: milliseconds per step of every region (text, mixed, text, mixed, ...), their medians, the ratio, and the
pair kernel's own execution time in a forward pass of the pair objective alone (an event pair riding on the launch), its
algorithmic bytes (2·M·d_w·4 in, the same out) and their share of the 6.29 TB/s the memory system delivers.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12

SHAPES = {
    "headline": dict(num_words=50000, num_entities=100000, word_repr_size=300, entity_repr_size=256, window_size=10, num_random_entities=16,
                     batch_normalization=1, nonlinearity="hard_tanh", bias_negative_samples=0, update_method="dense_adam",
                     regularization_lambda=0.01, batch=51200, lr=1e-3, pairs=(1024, 6400, 51200)),
    "lse": dict(num_words=200000, num_entities=100000, word_repr_size=128, entity_repr_size=256, window_size=10, num_random_entities=16,
                batch_normalization=0, nonlinearity="tanh", bias_negative_samples=1, update_method="sgd",
                regularization_lambda=0.01, batch=4096, lr=1e-2, pairs=(4096,)),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="headline,lse")
    ap.add_argument("--regions", type=int, default=3, help="pairs of timed regions (text-only, mixed) per shape")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per region")
    ap.add_argument("--pair-weight", type=float, default=0.2, help="--term_similarity_weight: the mixture is (1 - w, w)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_term_pairs.py needs a GPU (MI355X): the pair kernel and the table passes have no CPU fallback")
    dev = torch.device("cuda", args.device)
    ca.bind_host_thread(args.device)

    for name in args.shapes.split(","):
        shape = dict(SHAPES[name])
        B, lr, Ms = shape.pop("batch"), shape.pop("lr"), shape.pop("pairs")
        cfg = ca.default_config(max_batch_size=max(B, max(Ms)), device=args.device, sampler=ca.SAMPLER_DEVICE, **shape)
        m = ca.Model(cfg)
        m.initialize(1)
        rs = np.random.RandomState(3)
        nV, nD, w, dw = cfg.num_words, cfg.num_entities, cfg.window_size, cfg.word_repr_size
        p = 1.0 / np.arange(1, nV + 1)
        p /= p.sum()
        words = torch.from_numpy(rs.choice(nV, size=B * w, p=p).astype(np.int64)).to(dev)
        labels = torch.from_numpy(rs.randint(0, nD, B).astype(np.int64)).to(dev)
        batch = ca.Batch(words, labels)
        weights = (1.0 - args.pair_weight, args.pair_weight)

        def run(step, seconds):
            for _ in range(5):
                step()
            m.synchronize()
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(20):
                    step()
                n += 20
                m.synchronize()
                if time.perf_counter() - t0 >= seconds:
                    break
            return (time.perf_counter() - t0) * 1e3 / n

        for M in Ms:
            pairs = torch.from_numpy(rs.choice(nV, size=(M, 2), p=p).astype(np.int64)).to(dev)
            pw = torch.from_numpy(rs.uniform(0, 2, M).astype(np.float32)).to(dev)
            pb = ca.PairBatch(pairs, pw)
            text_step = lambda: m.step(batch, lr)
            mixed_step = lambda: m.step_term_mixed(batch, pb, lr, weights)
            mixed_step(); text_step(); m.synchronize()          # (the first term-pair call allocates the workspaces)
            regions = []
            for _ in range(args.regions):
                regions.append(("text", run(text_step, args.seconds)))
                regions.append(("mixed", run(mixed_step, args.seconds)))
            text_ms = float(np.median([t for k, t in regions if k == "text"]))
            mixed_ms = float(np.median([t for k, t in regions if k == "mixed"]))
            # the pair kernel alone: forward passes of the pair objective on an otherwise idle GPU, the event pair on the launch itself
            m.profile_select("term_pair_loss"); m.profile_reset(); m.profile_enable(True)
            for _ in range(30):
                m.compute_cost_term_mixed(None, pb)
                m.synchronize()
            ms, launches = m.profile()["term_pair_loss"]
            m.profile_enable(False); m.profile_select(None)
            kernel_us = ms * 1e3 / launches
            moved = 2 * (2 * M * dw * 4)
            print(json.dumps(dict(
                shape=name, update_method=shape["update_method"], batch=B, pairs=M, mixture=list(weights),
                regions_ms=[dict(kind=k, ms_per_step=round(t, 5)) for k, t in regions],
                text_only_ms=round(text_ms, 5), mixed_ms=round(mixed_ms, 5), mixed_over_text=round(mixed_ms / text_ms, 4),
                pair_kernel_us=round(kernel_us, 2), pair_kernel_bytes=moved,
                pair_kernel_hbm_share=round(moved / (kernel_us * 1e-6) / HBM_BYTES_PER_S, 4),
                describe=m.describe(B))), flush=True)
        m.close()


if __name__ == "__main__":
    main()
