"""-m gpu: cuNVSMTrainModel --fold_in on the Cranfield fixture: a model trained on the first 1 300 documents of the
collection, then the remaining documents folded in. The frozen datasets and the old documents' rows must come out byte for byte,
the new rows must start as cunvsm_amd.grow_documents draws them and train, the meta file must list the old objects first, the
query tool must take the result, two runs must agree, and every refused flag combination must say why."""
import os
import re
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.conftest import ROOT
from tests.helpers import PARAMS
from tests.test_host_layer import parse_metadata
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu

HOST_DIR = os.path.join(ROOT, "cunvsm_amd", "host")
FOLD_TESTS = os.path.join(HOST_DIR, "build", "fold_tests")
QUERY = os.path.join(ROOT, "cunvsm_amd", "bin", "cuNVSMQuery")
DW, DE, WINDOW = 32, 16, 10
MODEL_ARGS = ["--word_repr_size", str(DW), "--entity_repr_size", str(DE), "--window_size", str(WINDOW), "--num_random_entities", "4",
              "--seed", "1", "--update_method", "sparse_adam", "--batch_size", "1024", "--nonlinearity", "tanh", "--num_epochs", "1"]
OLD_DOCUMENTS = 1300


def documents():
    """(docno, text) of the collection, in file order — the index's order"""
    with open(CRANFIELD) as f:
        raw = f.read()
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"<DOCNO>(.*?)</DOCNO>(.*?)</DOC>", raw, re.S)]


def dump(checkpoint, outbase):
    """the four datasets of a checkpoint as float32 arrays (fold_tests --dump-hdf5: the host layer's own reader)"""
    subprocess.check_call(["make", "-C", HOST_DIR, "build/fold_tests"], stdout=subprocess.DEVNULL)
    out = subprocess.run([FOLD_TESTS, "--dump-hdf5", checkpoint, outbase], capture_output=True, text=True, check=True).stdout
    shapes = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in out.splitlines()}
    return {k: np.fromfile("%s.%s.f32" % (outbase, k), np.float32).reshape(shapes[k]) for k in "WETb"}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold")
    docs = documents()
    assert len(docs) == 1400
    listing = d / "first.txt"
    listing.write_text("".join(docno + "\n" for docno, _ in docs[:OLD_DOCUMENTS]))
    base, folded, again = str(d / "base"), str(d / "folded"), str(d / "again")
    r = run_trainer(MODEL_ARGS + ["--document_list", str(listing), "--output", base, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    logs = {}
    for out in (folded, again):
        r = run_trainer(MODEL_ARGS + ["--fold_in", base + "_1.hdf5", "--dump_initial_model", "--output", out, CRANFIELD])
        assert r.returncode == 0, r.stderr[-3000:]
        logs[out] = r.stderr
    return dict(dir=d, docs=docs, listing=str(listing), base=base, folded=folded, again=again, logs=logs)


def test_frozen_datasets_and_old_rows_are_byte_identical(runs):
    old, new = dump(runs["base"] + "_1.hdf5", str(runs["dir"] / "d_base")), dump(runs["folded"] + "_1.hdf5", str(runs["dir"] / "d_folded"))
    first = dump(runs["folded"] + "_0.hdf5", str(runs["dir"] / "d_first"))
    n_old = old["E"].shape[0]
    meta_old, meta_new = parse_metadata(runs["base"] + "_meta"), parse_metadata(runs["folded"] + "_meta")
    assert len(meta_old.object) == n_old and OLD_DOCUMENTS - 2 <= n_old <= OLD_DOCUMENTS      # (two documents of the collection are shorter than a window)
    n_all = new["E"].shape[0]
    assert n_all == 1398 and n_all - n_old >= 98
    for k in "WTb":
        assert old[k].tobytes() == new[k].tobytes() == first[k].tobytes(), k
    assert new["E"][:n_old].tobytes() == old["E"].tobytes() == first["E"][:n_old].tobytes()
    # the new rows: drawn as grow_documents draws them (the initial dump), and every one of them trained
    grown = ca.grow_documents({PARAMS[0]: old["W"], PARAMS[1]: old["E"], PARAMS[2]: old["T"], PARAMS[3]: old["b"]}, n_all - n_old, seed=1)
    np.testing.assert_array_equal(first["E"][n_old:].ravel(), grown[PARAMS[1]][n_old * DE:])
    assert np.all(np.any(new["E"][n_old:] != first["E"][n_old:], axis=1))
    # the meta file: the terms unchanged, the old objects first and as they were, the new ones behind them in index order
    assert [(t.index_term_id, t.model_term_id, t.term_frequency) for t in meta_new.term] == \
        [(t.index_term_id, t.model_term_id, t.term_frequency) for t in meta_old.term]
    assert meta_new.total_terms == meta_old.total_terms
    assert len(meta_new.object) == n_all
    assert [(o.index_object_id, o.model_object_id) for o in meta_new.object][:n_old] == [(o.index_object_id, o.model_object_id) for o in meta_old.object]
    fresh = meta_new.object[n_old:]
    assert [o.model_object_id for o in fresh] == list(range(n_old, n_all))
    assert [o.index_object_id for o in fresh] == sorted(o.index_object_id for o in fresh)
    assert not {o.index_object_id for o in fresh} & {o.index_object_id for o in meta_old.object}
    log = runs["logs"][runs["folded"]]
    assert "--max_vocabulary_size, --min_document_frequency and --max_document_frequency are ignored" in log
    assert "documents [0, %d) are frozen" % n_old in log


def test_two_fold_in_runs_write_the_same(runs):
    a, b = dump(runs["folded"] + "_1.hdf5", str(runs["dir"] / "r_a")), dump(runs["again"] + "_1.hdf5", str(runs["dir"] / "r_b"))
    for k in "WETb":
        assert a[k].tobytes() == b[k].tobytes(), k
    with open(runs["folded"] + "_meta", "rb") as f, open(runs["again"] + "_meta", "rb") as g:
        assert f.read() == g.read()


def test_the_query_tool_ranks_new_documents(runs):
    meta = parse_metadata(runs["folded"] + "_meta")
    n_old = len(parse_metadata(runs["base"] + "_meta").object)
    docs = runs["docs"]
    new_docnos = {docs[o.index_object_id - 1][0] for o in meta.object[n_old:]}      # index document ids count from 1 in file order
    assert new_docnos <= {docno for docno, _ in docs[OLD_DOCUMENTS:]}
    topics = runs["dir"] / "topics"
    lines = []
    for i, (docno, text) in enumerate([d for d in docs[OLD_DOCUMENTS:] if d[0] in new_docnos][:5]):
        words = re.findall(r"[a-z]+", text.lower())[:12]
        lines.append("%d;%s\n" % (i + 1, " ".join(words)))
    topics.write_text("".join(lines))
    run = str(runs["dir"] / "run")
    q = subprocess.run([QUERY, "--index", CRANFIELD, "--topics", str(topics), "--top_k", "100", runs["folded"] + "_1.hdf5", run],
                       capture_output=True, text=True, timeout=300)
    assert q.returncode == 0, q.stderr[-3000:]
    with open(run + "-topics") as f:
        ranked = [line.split()[2] for line in f]
    assert len(ranked) >= 100
    assert new_docnos & set(ranked)


@pytest.mark.parametrize("extra,message", [
    (["--device_corpus"], "--fold_in cannot be combined with --device_corpus"),
    (["--gpus", "2"], "--fold_in is not implemented under data parallelism"),
    (["--world_size", "2", "--rank", "0"], "--fold_in is not implemented under data parallelism"),
    (["--entity_similarity_weight", "0.3"], "--fold_in trains the text-entity objective only"),
    (["--term_similarity_weight", "0.3"], "--fold_in trains the text-entity objective only"),
    (["--l2_entity_normalization"], "--fold_in cannot be combined with --l2_entity_normalization"),
    (["--check_gradients"], "--fold_in cannot be combined with --check_gradients"),
])
def test_refused_flag_combinations(runs, extra, message):
    r = run_trainer(MODEL_ARGS + ["--fold_in", runs["base"] + "_1.hdf5"] + extra + [CRANFIELD])
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]


def test_a_model_description_that_disagrees_and_a_list_without_new_documents_are_fatal(runs):
    args = [a for a in MODEL_ARGS]
    args[args.index("--word_repr_size") + 1] = str(DW + 1)
    r = run_trainer(args + ["--fold_in", runs["base"] + "_1.hdf5", CRANFIELD])
    assert r.returncode != 0 and "--word_repr_size %d does not describe it" % (DW + 1) in r.stderr, r.stderr[-2000:]
    r = run_trainer(MODEL_ARGS + ["--fold_in", runs["base"] + "_1.hdf5", "--document_list", runs["listing"], CRANFIELD])
    assert r.returncode != 0 and "no new documents" in r.stderr, r.stderr[-2000:]
