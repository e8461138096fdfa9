"""CPU test of the host layer's window references (cunvsm_amd/host/index_source.hpp: corpus_view, next_refs, hold_plan_in):
tests/cpp/corpus_tests.cpp draws two epochs as references, expands them on the CPU from the corpus view by the definition in
include/cunvsm_amd.h, and holds them against two epochs drawn as batches — same instances, weights, order and generator state —
for every order x feature weighting x instance weighting, on the Cranfield collection and on the reference's mock index. Built
here with g++, once plainly and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
CRANFIELD = os.path.join(ROOT, "tests", "golden", "cranfield", "cranfield.trectext")


@pytest.mark.parametrize("target", ["corpus_tests", "corpus_tests_san"])
def test_epochs_drawn_as_references_equal_epochs_drawn_as_batches(target):
    subprocess.check_call(["make", "-C", HOST_DIR, "build/" + target], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST_DIR, "build", target), CRANFIELD], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 failed")
    assert r.stdout.count("[ok]") == 24 and "FAIL" not in r.stdout           # 3 orders x 2 x 2, on two collections
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
