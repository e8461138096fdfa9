"""CPU tests of what cuNVSMTrainModel --fold_in does on the host (cunvsm_amd/host/index_source.hpp): tests/cpp/fold_tests.cpp holds
the cases, on the Cranfield fixture — which documents of an index (or of a document list) are new to a meta file and in what
order, the refusals, the fixed vocabulary, the label offset, and the term weights out of the meta file's frequencies. Built by the
host Makefile's `all` as build/fold_tests; this file checks the verdict of every case."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
BIN = os.path.join(HOST_DIR, "build", "fold_tests")
CRANFIELD = os.path.join(ROOT, "tests", "golden", "cranfield", "cranfield.trectext")

CASES = ["FoldIn.new_documents_in_index_order_and_refusals", "FoldIn.source_vocabulary_labels_and_weights",
         "FoldIn.existing_constructor_is_unchanged"]


@pytest.fixture(scope="module")
def fold_tests():
    subprocess.check_call(["make", "-C", HOST_DIR, "build/fold_tests"], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("case", CASES)
def test_fold_host_case(fold_tests, case):
    r = subprocess.run([fold_tests, CRANFIELD, case], capture_output=True, text=True, timeout=120)
    assert "[PASS] %s" % case in r.stdout, r.stdout + r.stderr
    assert r.returncode == 0


def test_every_case_is_listed(fold_tests):
    r = subprocess.run([fold_tests, CRANFIELD], capture_output=True, text=True, timeout=300)
    ran = re.findall(r"\[(?:PASS|FAIL)\] (\S+)", r.stdout)
    assert sorted(ran) == sorted(CASES)
    assert r.stdout.strip().endswith("0 failed")


def test_the_host_makefile_builds_the_fold_tests_by_default():
    with open(os.path.join(HOST_DIR, "Makefile")) as f:
        assert re.search(r"^all:.*build/fold_tests", f.read(), re.M)
