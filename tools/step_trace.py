#!/usr/bin/env python
"""A fixed series of training calls for comparing the engine's HIP calls between two builds of the library:

    CUNVSM_AMD_LIB=<build> rocprofv3 --hip-runtime-trace --kernel-trace -f csv -d <dir> -- python tools/step_trace.py
    python tools/step_trace_diff.py <dir of build 1> <dir of build 2>

It runs tests/step_requests.SEQUENCE on both of its shapes — through the fused entry points on one handle, then as compute_cost*;
compute_gradients; update on a second one — and three fused text steps each at batches 4 096, 16 384 and 40 960 of the `large`
shape of tests/test_gpu_switches.py. Nothing is compared here (tests/test_gpu_step_requests.py does that): the point is that the
same calls reach the runtime in the same order, which the bit tests cannot see — a stream wait that moved may happen not to matter."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cunvsm_amd as ca  # noqa: E402
from tests.helpers import gpu_model  # noqa: E402
from tests.step_requests import Inputs, call  # noqa: E402

LARGE = dict(num_words=3000, num_entities=5000, word_dim=300, entity_dim=256, window=4, num_random=3, nonlinearity="hard_tanh",
             batch_norm=True, bias_negative_samples=False, update_method="sparse_adam", **{"lambda": 0.01})


def main():
    print("library: %s" % ca.library_path())
    for shape in ("a", "b"):
        inp = Inputs(shape)
        for fused in (True, False):
            m = inp.model()
            for kind, x in inp.calls:
                call(m, kind, x, inp.lr, fused)
                if kind == "no_corpus":
                    m.upload_corpus(inp.corpus)
            m.synchronize()
            m.close()
    rs = np.random.RandomState(5)
    for B in (4096, 16384, 40960):
        m = gpu_model(LARGE, B, sampler=ca.SAMPLER_DEVICE)
        m.initialize(7)
        w = LARGE["window"]
        for step in range(3):
            batch = ca.Batch((rs.zipf(1.3, B * w) % LARGE["num_words"]).astype(np.int64), rs.randint(0, LARGE["num_entities"], B).astype(np.int64),
                             rs.uniform(0.5, 1.5, B * w).astype(np.float32), rs.uniform(0.5, 1.5, B).astype(np.float32))
            m.step(batch, 0.001, want_cost=(step == 1))
        m.synchronize()
        m.close()
    print("step_trace done")


if __name__ == "__main__":
    main()
