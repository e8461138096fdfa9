"""CPU tests of the entity-entity pair source of the host layer (cunvsm_amd/host/pair_source.hpp): tests/cpp/pairs_tests.cpp
restates the reference's RepresentationSimilarityTest cases (cpp/data_tests.cpp:687-746) and adds the skip warning, repetition
across passes with a short last batch and a seed-pinned order; it is built by the host Makefile's `all` as build/pairs_tests,
and this file checks the verdict of every case."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
BIN = os.path.join(HOST_DIR, "build", "pairs_tests")

CASES = [
    "RepresentationSimilarityTest.LoadSimilarities", "RepresentationSimilarityTest.DataSource",
    "RepresentationSimilarityTest.LoadSimilarities_skips_unknown_documents",
    "RepresentationSimilarityTest.repetition_with_a_short_last_batch", "RepresentationSimilarityTest.seed_pinned_order",
]


@pytest.fixture(scope="module")
def pairs_tests():
    subprocess.check_call(["make", "-C", HOST_DIR, "build/pairs_tests"], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("case", CASES)
def test_pair_source_case(pairs_tests, case):
    r = subprocess.run([pairs_tests, case], capture_output=True, text=True, timeout=120)
    assert "[PASS] %s" % case in r.stdout, r.stdout + r.stderr
    assert r.returncode == 0


def test_every_case_is_listed(pairs_tests):
    r = subprocess.run([pairs_tests], capture_output=True, text=True, timeout=300)
    ran = re.findall(r"\[(?:PASS|FAIL)\] (\S+)", r.stdout)
    assert sorted(ran) == sorted(CASES)
    assert r.stdout.strip().endswith("0 failed")


def test_the_host_makefile_builds_it_by_default():
    with open(os.path.join(HOST_DIR, "Makefile")) as f:
        text = f.read()
    assert re.search(r"^all:.*build/pairs_tests", text, re.M)
