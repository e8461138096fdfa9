#!/usr/bin/env python
"""A fixed series of retrieval calls for comparing the engine's HIP calls between two builds of the library — the retrieval twin of
tools/step_trace.py:

    CUNVSM_AMD_LIB=<build> rocprofv3 --hip-runtime-trace --kernel-trace -f csv -d <dir> -- python tools/rank_trace.py
    python tools/step_trace_diff.py <dir of build 1> <dir of build 2>

It runs the series of tests/retrieval_rounds.py (what tests/test_gpu_retrieval_rounds.py runs: nine entry points on one handle, three
slabs, two rounds), forwards and then in reverse, and prints behind every call a SHA-256 of each returned array, the handle's profile
names with their launch counts, and the device memory in use above what was in use before the handle was made. Two builds that do the
same work print the same lines; the traces say whether they reached the runtime through the same calls in the same order."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import retrieval_rounds as rr  # noqa: E402

os.environ["NVSM_RANK_SLAB_MB"] = rr.SLAB_MB      # (read when the handle is created)
import cunvsm_amd as ca  # noqa: E402


def main():
    import torch
    print("library: %s" % ca.library_path(), file=sys.stderr)
    in_use = lambda: torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]
    inp = rr.Inputs()
    base = in_use()
    m = inp.model()
    m.profile_enable(True)
    calls = inp.calls()
    for name, call in calls + calls[::-1]:
        for what, x in rr.arrays(call(m)):
            x = np.ascontiguousarray(x)
            print("%s %s %s%s %s" % (name, what, x.dtype, list(x.shape), hashlib.sha256(x.tobytes()).hexdigest()))
        print("%s profile %s" % (name, " ".join("%s=%d" % (n, c) for n, (_, c) in sorted(m.profile().items()))))
        print("%s memory %.1f MiB" % (name, (in_use() - base) / 2.0 ** 20))
    m.synchronize()
    m.close()
    print("rank_trace done")


if __name__ == "__main__":
    main()
