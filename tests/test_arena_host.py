"""CPU test of the factored arena builder (cunvsm_amd/host/token_arena.hpp), which IndexSource and cuNVSMQuery --qlm share:
tests/cpp/arena_tests.cpp builds the arena from the id mappings a checkpoint's meta file carries and holds it against
IndexSource::corpus_view() byte for byte, on the Cranfield collection and on the reference's mock index. Built here with g++, once
plainly and once as a stand-alone program under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
CRANFIELD = os.path.join(ROOT, "tests", "golden", "cranfield", "cranfield.trectext")


@pytest.mark.parametrize("target", ["arena_tests", "arena_tests_san"])
def test_the_arena_builder_gives_the_bytes_of_the_sources_corpus_view(target):
    subprocess.check_call(["make", "-C", HOST_DIR, "build/" + target], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST_DIR, "build", target), CRANFIELD], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("0 failed")
    assert r.stdout.count("[ok]") == 9 and "FAIL" not in r.stdout            # 2 collections x OoV or not x 2 orders, + the gaps
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
