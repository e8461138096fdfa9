"""CPU tests of what cuNVSMQuery does on the host (cunvsm_amd/host/query_lib.hpp and read_hdf5 of hdf5_writer.hpp):
tests/cpp/query_tests.cpp holds the cases — the write_hdf5 -> read_hdf5 round trip bit for bit and the reader's refusals, where the
meta file of a checkpoint lies, the topic and qrel parsers, the meta file's mappings with their refusals, out-of-vocabulary
terms and --strict; it is built by the host Makefile's `all` as build/query_tests, and this file checks the verdict of every case
and the files its --make-model mode writes for tests/test_query_cli_gpu.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
BIN = os.path.join(HOST_DIR, "build", "query_tests")

CASES = [
    "Hdf5Reader.round_trip_is_bit_exact", "Hdf5Reader.refusals", "ModelPath.meta_file_and_batch_fallback", "Topics.parser",
    "Qrels.parser", "Meta.mappings_and_their_refusals", "Topics.terms_out_of_vocabulary_and_strict",
]


@pytest.fixture(scope="module")
def query_tests():
    subprocess.check_call(["make", "-C", HOST_DIR, "build/query_tests"], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("case", CASES)
def test_query_host_case(query_tests, case):
    r = subprocess.run([query_tests, case], capture_output=True, text=True, timeout=120)
    assert "[PASS] %s" % case in r.stdout, r.stdout + r.stderr
    assert r.returncode == 0


def test_every_case_is_listed(query_tests):
    r = subprocess.run([query_tests], capture_output=True, text=True, timeout=300)
    ran = re.findall(r"\[(?:PASS|FAIL)\] (\S+)", r.stdout)
    assert sorted(ran) == sorted(CASES)
    assert r.stdout.strip().endswith("0 failed")


def test_the_host_makefile_builds_the_tool_and_its_tests_by_default():
    with open(os.path.join(HOST_DIR, "Makefile")) as f:
        text = f.read()
    assert re.search(r"^all:.*build/query_tests", text, re.M) and re.search(r"^all:.*\.\./bin/cuNVSMQuery", text, re.M)


def read_mapping_dump(path):
    """<outbase>.map.txt of --make-model: (total_terms, {term: (index id, model id, tf)}, [(index object id, model id, docno)])"""
    total, terms, objects = None, {}, []
    with open(path) as f:
        for line in f:
            cols = line.split()
            if cols[0] == "total_terms":
                total = int(cols[1])
            elif cols[0] == "term":
                terms[cols[4]] = (int(cols[1]), int(cols[2]), int(cols[3]))
            else:
                objects.append((int(cols[1]), int(cols[2]), cols[3]))
    return total, terms, objects


def test_make_model_writes_a_checkpoint_with_every_7th_term_and_9th_document_left_out(query_tests, tmp_path):
    collection = tmp_path / "c.trectext"
    collection.write_text("".join("<DOC>\n<DOCNO> D%02d </DOCNO>\n<TEXT>\nword%d and common w%d\n</TEXT>\n</DOC>\n" % (i, i, i % 3)
                                  for i in range(1, 21)))
    stop = tmp_path / "stop.txt"
    stop.write_text("and\n")
    out = str(tmp_path / "m")
    r = subprocess.run([query_tests, "--make-model", str(collection), out, str(stop)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    total, terms, objects = read_mapping_dump(out + ".map.txt")
    assert total == 60                                       # 20 documents x 3 indexed terms ("and" is stopped)
    # index terms in order of first occurrence: word1 common w1 word2 w2 word3 w0 word4 ...: 24 of them, ids 7, 14, 21 left out
    assert len(terms) == 24 - 3 and "and" not in terms and "w0" not in terms
    assert terms["common"] == (2, 1, 20) and terms["word1"] == (1, 0, 1)
    assert sorted(m for _, m, _ in terms.values()) == list(range(21))
    assert [o[0] for o in objects] == [d for d in range(1, 21) if d % 9] and [o[1] for o in objects] == list(range(18))
    assert objects[8] == (10, 8, "D10")
    W = np.fromfile(out + ".W.f32", np.float32).reshape(21, 12)
    E = np.fromfile(out + ".E.f32", np.float32).reshape(18, 36)
    assert np.fromfile(out + ".T.f32", np.float32).size == 12 * 36 and np.fromfile(out + ".b.f32", np.float32).size == 36
    assert W[0, 0] == np.float32(np.sin(0.37)) and E[1, 2] == np.float32(np.cos(0.11 * 2 * 3 + 1.0))
    assert os.path.getsize(out + "_meta") > 0 and os.path.getsize(out + "_3.hdf5") > 4 * (W.size + E.size)
