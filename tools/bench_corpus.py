#!/usr/bin/env python
"""Times a training step fed four ways, in alternating timed regions of ONE process and handle:
  (a) resident      nvsm_step on a batch already in HBM — the figure to aim at;
  (b) host_batch    nvsm_step on a page-locked host batch (132 B per window at window 10) — today's host path;
  (c) refs_host     nvsm_step_windows on page-locked window references (8 B per window) into the uploaded corpus;
  (d) refs_device   nvsm_step_windows on window references already in HBM.
All four train on the same windows (the batch of (a) and (b) is expand_windows of the references of (c) and (d)).

Shapes: the headline shape (|V| = 50 k, |D| = 100 k, 300 -> 256, window 10, 16 negatives, 51 200 windows, batch-norm + hard_tanh,
sparse Adam) and the LSE shape (|V| = 200 k, 128 -> 256, 4 096 windows, tanh, no batch-norm, full Adam); device sampler; a synthetic
Zipf corpus of about 40 tokens per document.
Per shape one JSON line: milliseconds per step and windows per second of every region, their medians, the region-to-region
spread of (a) (the margin the other figures are held against), the expansion kernel's own execution time alone on an idle GPU
and inside the steps of (d) (an event pair riding on the launch), its algorithmic bytes (8 + 8 + 4·w in, 12·w + 12 out per
window), and the share of a step of (d) that the copy stream spends in it.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "headline": dict(num_words=50000, num_entities=100000, word_repr_size=300, entity_repr_size=256, window_size=10, num_random_entities=16,
                     batch_normalization=1, nonlinearity="hard_tanh", bias_negative_samples=0, update_method="sparse_adam",
                     regularization_lambda=0.01, batch=51200, lr=1e-3),
    "lse": dict(num_words=200000, num_entities=100000, word_repr_size=128, entity_repr_size=256, window_size=10, num_random_entities=16,
                batch_normalization=0, nonlinearity="tanh", bias_negative_samples=1, update_method="full_adam",
                regularization_lambda=0.01, batch=4096, lr=1e-3),
}
KINDS = ("resident", "host_batch", "refs_host", "refs_device")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="headline,lse")
    ap.add_argument("--regions", type=int, default=3, help="rounds of the four timed regions per shape")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per region")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    from cunvsm_amd.model import pinned_copy
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_corpus.py needs a GPU (MI355X): the expansion kernel and the step have no CPU fallback")
    dev = torch.device("cuda", args.device)
    ca.bind_host_thread(args.device)

    for name in args.shapes.split(","):
        shape = dict(SHAPES[name])
        B, lr = shape.pop("batch"), shape.pop("lr")
        cfg = ca.default_config(max_batch_size=B, device=args.device, sampler=ca.SAMPLER_DEVICE, **shape)
        m = ca.Model(cfg)
        m.initialize(1)
        rs = np.random.RandomState(3)
        nV, nD, w = cfg.num_words, cfg.num_entities, cfg.window_size
        lengths = np.maximum(rs.poisson(40, nD), w)
        p = 1.0 / np.arange(1, nV + 1)
        tokens = rs.choice(nV, size=int(lengths.sum()), p=p / p.sum()).astype(np.int32)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        corpus = ca.Corpus(tokens, offsets, np.ones(nD, np.float32), rs.uniform(0.5, 2.0, nV).astype(np.float32))
        m.upload_corpus(corpus)
        doc = rs.randint(0, nD, B)
        refs = np.ascontiguousarray(np.stack([doc, (rs.uniform(0, 1, B) * (lengths[doc] - w + 1)).astype(np.int64)], axis=1), dtype=np.uint32)
        host = ca.expand_windows(corpus, refs, w)
        pins = [pinned_copy(a) for a in (host.features, host.labels, host.feature_weights, host.weights)]
        refs_pin = pinned_copy(refs)
        batches = {
            "resident": ca.Batch(*[torch.from_numpy(x.array).to(dev) for x in pins]),
            "host_batch": ca.Batch(*[x.array for x in pins]),
            "refs_host": ca.WindowBatch(refs_pin.array),
            "refs_device": ca.WindowBatch(torch.from_numpy(refs.view(np.int32)).to(dev)),
        }
        steps = {k: (lambda b=b: m.step(b, lr)) if k in ("resident", "host_batch") else (lambda b=b: m.step_windows(b, lr))
                 for k, b in batches.items()}

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

        regions = []
        for _ in range(args.regions):
            for kind in KINDS:
                regions.append((kind, run(steps[kind], args.seconds)))
        median = {k: float(np.median([t for kk, t in regions if kk == k])) for k in KINDS}
        resident = [t for k, t in regions if k == "resident"]

        def kernel_us(call):
            m.profile_select("window_expand"); m.profile_reset(); m.profile_enable(True)
            for _ in range(30):
                call()
            m.synchronize()
            ms, launches = m.profile()["window_expand"]
            m.profile_enable(False); m.profile_select(None)
            return ms * 1e3 / launches

        def alone():
            m.compute_cost_windows(batches["refs_device"])
            m.synchronize()

        alone_us, in_step_us = kernel_us(alone), kernel_us(steps["refs_device"])
        moved = B * (8 + 8 + 4 * w) + B * (12 * w + 12)
        print(json.dumps(dict(
            shape=name, update_method=shape["update_method"], batch=B, window=w, corpus_tokens=int(tokens.size),
            bytes_per_step=dict(host_batch=B * (12 * w + 12), refs=B * 8),
            regions_ms=[dict(kind=k, ms_per_step=round(t, 5)) for k, t in regions],
            ms_per_step={k: round(v, 5) for k, v in median.items()},
            windows_per_s={k: round(B / (v * 1e-3)) for k, v in median.items()},
            resident_region_spread=round((max(resident) - min(resident)) / median["resident"], 4),
            refs_host_over_host_batch=round(median["refs_host"] / median["host_batch"], 4),
            expand_kernel_us_alone=round(alone_us, 2), expand_kernel_us_in_step=round(in_step_us, 2), expand_kernel_bytes=moved,
            expand_kernel_GBps_alone=round(moved / (alone_us * 1e-6) / 1e9, 1),
            copy_stream_share_of_step=round(in_step_us * 1e-3 / median["refs_device"], 4),
            describe=m.describe(B))), flush=True)
        m.close()


if __name__ == "__main__":
    main()
