#!/usr/bin/env python
"""Times the fold-in step (nvsm_step_fold) against the full step (nvsm_step) of the SAME process, handle and batches, in alternating
timed regions.

Shape: the headline shape (|V| = 50 k, |D| = 100 k, 300 -> 256, window 10, 16 negatives, 51 200 windows, batch-norm + hard_tanh,
sparse Adam), first_document = 90 000 and 99 900: the positives of every window lie on the new documents (10 000 or 100 of them —
about 5 or 512 positives per new row and step), the negatives are drawn over all documents by the device sampler. Batches are
resident in HBM. Per first_document one JSON line: milliseconds per step of every region (step, fold, step, fold, ...), their
medians, the ratio, and the execution time of the fold kernels (events around fold.hip's launches) next to the full step's
documents pass. --design <file> also writes the figures between the bench_fold markers of that file's fold-in section.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = dict(num_words=50000, num_entities=100000, word_repr_size=300, entity_repr_size=256, window_size=10, num_random_entities=16,
             batch_normalization=1, nonlinearity="hard_tanh", bias_negative_samples=0, update_method="sparse_adam",
             regularization_lambda=0.01)
BEGIN, END = "<!-- bench_fold:begin -->", "<!-- bench_fold:end -->"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--first", default="90000,99900", help="first_document values")
    ap.add_argument("--batch", type=int, default=51200)
    ap.add_argument("--regions", type=int, default=3, help="pairs of timed regions (step, fold) per first_document")
    ap.add_argument("--seconds", type=float, default=0.5, help="timed work per region")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--design", default="", help="file whose bench_fold block is rewritten with the figures")
    args = ap.parse_args()

    import numpy as np
    import torch

    import cunvsm_amd as ca
    if not torch.cuda.is_available() or ca.device_count() < 1:
        sys.exit("bench_fold.py needs a GPU (MI355X): the fold kernels have no CPU fallback")
    dev = torch.device("cuda", args.device)
    ca.bind_host_thread(args.device)
    B, lr = args.batch, 1e-3
    cfg = ca.default_config(max_batch_size=B, device=args.device, sampler=ca.SAMPLER_DEVICE, **SHAPE)
    m = ca.Model(cfg)
    m.initialize(1)
    rs = np.random.RandomState(3)
    nV, nD, w = cfg.num_words, cfg.num_entities, cfg.window_size
    p = 1.0 / np.arange(1, nV + 1)
    p /= p.sum()
    words = torch.from_numpy(rs.choice(nV, size=B * w, p=p).astype(np.int64)).to(dev)

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

    def kernel_us(step, name):
        m.profile_select(name); m.profile_reset(); m.profile_enable(True)
        for _ in range(30):
            step()
            m.synchronize()
        ms, launches = m.profile()[name]
        m.profile_enable(False); m.profile_select(None)
        return ms * 1e3 / launches

    rows = []
    for n0 in [int(x) for x in args.first.split(",")]:
        labels = torch.from_numpy(rs.randint(n0, nD, B).astype(np.int64)).to(dev)
        batch = ca.Batch(words, labels)
        full_step = lambda: m.step(batch, lr)
        fold_step = lambda: m.step_fold(batch, lr, n0, want_cost=False)
        fold_step(); full_step(); m.synchronize()          # (the first fold step allocates its partial buffers)
        regions = []
        for _ in range(args.regions):
            regions.append(("step", run(full_step, args.seconds)))
            regions.append(("fold", run(fold_step, args.seconds)))
        step_ms = float(np.median([t for k, t in regions if k == "step"]))
        fold_ms = float(np.median([t for k, t in regions if k == "fold"]))
        fold_kernels = kernel_us(fold_step, "fold_update")
        docs_pass = kernel_us(full_step, "row_pass_entities")
        row = dict(shape="headline", update_method=SHAPE["update_method"], batch=B, num_entities=nD, first_document=n0,
                   regions_ms=[dict(kind=k, ms_per_step=round(t, 5)) for k, t in regions],
                   step_ms=round(step_ms, 5), fold_ms=round(fold_ms, 5), fold_over_step=round(fold_ms / step_ms, 4),
                   fold_kernels_us=round(fold_kernels, 2), step_documents_pass_us=round(docs_pass, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    m.close()

    if args.design:
        lines = ["| first_document | new rows | nvsm_step ms | nvsm_step_fold ms | fold / step | fold kernels µs | documents pass of the full step µs |",
                 "|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append("| %d | %d | %.4f | %.4f | %.3f | %.1f | %.1f |" % (
                r["first_document"], r["num_entities"] - r["first_document"], r["step_ms"], r["fold_ms"], r["fold_over_step"],
                r["fold_kernels_us"], r["step_documents_pass_us"]))
        block = BEGIN + "\n" + "\n".join(lines) + "\n" + END
        with open(args.design) as f:
            text = f.read()
        if BEGIN not in text or END not in text:
            sys.exit("%s has no bench_fold block" % args.design)
        text = re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda _: block, text, flags=re.S)
        with open(args.design, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
