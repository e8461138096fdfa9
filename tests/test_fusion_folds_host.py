"""CPU tests of what cuNVSMQuery --ensemble_qrel decides on the host (cunvsm_amd/host/query_lib.hpp ensemble_folds and
ensemble_measure): tests/cpp/fusion_folds_tests.cpp holds the cases, built by the host Makefile's `all` as build/fusion_folds_tests;
this file checks every case's verdict and holds the program's folds against the restatement of the permutation that the GPU tests of
the tool rely on (tests/fusion_cv_reference.py shuffled_folds)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fusion_cv_reference as fr
from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
BIN = os.path.join(HOST_DIR, "build", "fusion_folds_tests")

CASES = ["Folds.topic_file_order", "Folds.seeded_permutation_by_hand", "Folds.seeded_permutation_against_its_rule", "Measure.names_and_map_cut"]


@pytest.fixture(scope="module")
def folds_tests():
    subprocess.check_call(["make", "-C", HOST_DIR, "build/fusion_folds_tests"], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("case", CASES)
def test_fusion_folds_case(folds_tests, case):
    r = subprocess.run([folds_tests, case], capture_output=True, text=True, timeout=120)
    assert "[PASS] %s" % case in r.stdout, r.stdout + r.stderr
    assert r.returncode == 0


def test_every_case_is_listed(folds_tests):
    r = subprocess.run([folds_tests], capture_output=True, text=True, timeout=120)
    assert sorted(re.findall(r"\[(?:PASS|FAIL)\] (\S+)", r.stdout)) == sorted(CASES)
    assert r.stdout.strip().endswith("0 failed")


def test_the_host_makefile_builds_it_by_default():
    with open(os.path.join(HOST_DIR, "Makefile")) as f:
        assert re.search(r"^all:.*build/fusion_folds_tests", f.read(), re.M)


def test_the_restated_permutation_by_hand():
    assert fr.shuffled_folds(5, 5, 0).tolist() == [0, 1, 2, 3, 4] and fr.shuffled_folds(7, 3, 0).tolist() == [0, 0, 0, 1, 1, 2, 2]
    # minstd_rand0(1): 16807, 282475249, ...: i = 2 takes j = 16807 % 3 = 1, i = 1 takes j = 282475249 % 2 = 1 -> order 0, 2, 1
    assert fr.shuffled_folds(3, 3, 1).tolist() == [0, 2, 1]
    assert fr.shuffled_folds(4, 2, 1).tolist() == [0, 1, 0, 1]
    shuffled = fr.shuffled_folds(23, 5, 1)
    assert np.bincount(shuffled).tolist() == [5, 5, 5, 4, 4] and shuffled.tolist() != fr.kfold(23, 5).tolist()


@pytest.mark.parametrize("n,num_folds,seed", [(5, 5, 1), (5, 2, 0), (5, 3, 7), (23, 5, 1), (225, 20, 1), (225, 20, 0), (225, 20, 2147483646), (224, 5, 12345)])
def test_the_tools_folds_are_the_restatements(folds_tests, n, num_folds, seed):
    r = subprocess.run([folds_tests, "--folds", str(n), str(num_folds), str(seed)], capture_output=True, text=True, timeout=60, check=True)
    assert [int(x) for x in r.stdout.split()] == fr.shuffled_folds(n, num_folds, seed).tolist()
