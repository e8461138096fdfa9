"""-m gpu: cuNVSMQuery --qlm / --ensemble_alpha (cunvsm_amd/host/query_main.cpp) end to end. On the 70-document collection and the
checkpoint of tests/test_query_cli_gpu.py: the query-likelihood run file equals Model.lexical_rank on the same topics over the arena
this file builds from the mapping dump, the fused run file and the printed means equal Model.rank_ensemble's. On Cranfield, with the
collection's own topics and judgments: the whole last stage of the reference's demo, whose MAPs are printed for DESIGN.md §14 and
not asserted (tokenisation, stopping and the checkpoint differ from the reference's)."""
import os
import re

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import eval_reference as er
from tests.test_query_cli_gpu import (CUTOFFS, VOCAB, Corpus, assert_same_run, base_args, expected_rows, printed_metrics, read_run,
                                      run_query)
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.dirname(CRANFIELD)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = Corpus(tmp_path_factory.mktemp("query_lexical_cli"))
    # the collection as cuNVSMQuery uploads it: every document's words in the model's vocabulary (the stop words and the words the
    # model lacks are dropped: the model holds no out-of-vocabulary token), documents in model id order
    assert all(index_id != 0 for index_id, _, _ in c.terms.values())
    docs = {}
    for i in range(1, 71):
        words = [VOCAB[(i * j + j * j) % 30] for j in range(1, 12)]
        docs["DOC-%03d" % i] = [c.terms[w][1] for w in words if w in c.terms]
    by_model_id = [docs[c.docno_of[m]] for m in range(c.D)]
    tokens = np.array([t for d in by_model_id for t in d], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in by_model_id])]).astype(np.int64)
    c.model.upload_corpus(ca.Corpus(tokens, offsets))
    yield c
    c.model.close()


def kept_queries(corpus, name):
    kept, _, _, _ = corpus.expected(name)
    return kept, [t for _, t in kept]


@pytest.mark.parametrize("method,param", [("jm", "auto"), ("dirichlet", "auto"), ("jm", "0.3"), ("dirichlet", "25")])
def test_the_query_likelihood_run_is_lexical_ranks(corpus, tmp_path, method, param):
    out, qlm = str(tmp_path / "run"), str(tmp_path / "qlm")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    r = run_query(flags + ["--qlm", method, "--qlm_param", param, "--qlm_run_out", qlm] + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("topics_a", "topics_b"):
        kept, queries = kept_queries(corpus, name)
        ids, scores, counts = corpus.model.lexical_rank(queries, method=method, param=None if param == "auto" else float(param), top_k=corpus.D)
        assert (counts > 0).all() and (counts < corpus.D).any()               # only documents that hold a query word are retrieved
        assert_same_run(read_run("%s-%s" % (qlm, name)), expected_rows(corpus, kept, ids, scores, counts))
        # without --ensemble_alpha <run_out> is the NVSM run it always was
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, *corpus.expected(name)))
    assert r.stdout == ""


@pytest.mark.parametrize("alpha,normalizer,top_k", [("0.5", "standardize", None), ("0.3", "minmax", 5), ("1", "none", 20)])
def test_the_fused_run_and_the_printed_means_are_rank_ensembles(corpus, tmp_path, alpha, normalizer, top_k):
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    extra = ["--qlm", "jm", "--ensemble_alpha", alpha, "--score_normalizer", normalizer, "--qrels", corpus.qrel_path]
    if top_k:
        extra += ["--top_k", top_k]
    r = run_query(flags + extra + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = printed_metrics(r.stdout)
    assert len(blocks) == 2
    k = min(top_k or 1000, corpus.D)
    for name, block in zip(("topics_a", "topics_b"), blocks):
        kept, queries = kept_queries(corpus, name)
        judged = [corpus.judged_ids(t) for t, _ in kept]
        res, ids, scores, counts = corpus.model.rank_ensemble(queries, alpha=float(alpha), normalizer=normalizer, judgments=judged, top_k=k,
                                                              cutoffs=CUTOFFS, bias_coefficient=0.0, activation="tanh")
        assert ids.shape[1] == 2 * k and (counts >= k).all()
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, kept, ids, scores, counts))
        ref = er.evaluate(ids, counts, judged, CUTOFFS)
        evaluated = ref["num_rel"] > 0
        assert block["num_q"] == str(int(evaluated.sum()))
        for metric in er.names(CUTOFFS):
            np.testing.assert_allclose(res[metric], ref[metric], rtol=0, atol=1e-10, err_msg=metric)
            if metric in er.INTEGER:
                assert block[metric] == str(int(ref[metric][evaluated].sum())), metric
            else:
                assert re.fullmatch(r"\d\.\d{4}", block[metric]), block[metric]
                assert abs(float(block[metric]) - ref[metric][evaluated].mean()) <= 0.5e-4 + 1e-9, metric


def test_refusals_and_the_help_text(corpus, tmp_path):
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_b")
    for extra, word in ((["--qlm", "bm25", "--qlm_run_out", out], "--qlm"), (["--qlm", "jm"], "--qlm_run_out"),
                        (["--qlm", "jm", "--qlm_param", "1.5", "--qlm_run_out", out], "--qlm_param"),
                        (["--qlm", "dirichlet", "--qlm_param", "-3", "--qlm_run_out", out], "--qlm_param"),
                        (["--qlm", "jm", "--ensemble_alpha", "1.2"], "--ensemble_alpha"),
                        (["--qlm", "jm", "--ensemble_alpha", "0.5", "--score_normalizer", "zscore"], "--score_normalizer"),
                        (["--ensemble_alpha", "0.5"], "need --qlm"), (["--qlm_run_out", out], "need --qlm"),
                        (["--qlm", "jm", "--qlm_run_out", out, "--top_k", corpus.qrel_path], "--top_k")):
        r = run_query(flags + extra + positional)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics_b")
    r = run_query(["--help"])
    assert r.returncode == 0 and r.stdout.count("NOT OFFERED") == 3
    for flag in ("qlm", "qlm_param", "qlm_run_out", "ensemble_alpha", "score_normalizer"):
        assert "-%s (" % flag in r.stdout


def test_cranfield_the_demos_last_stage(tmp_path):
    """two epochs of LSE on Cranfield, then the NVSM run, the query-likelihood run and their fusion over the collection's 225 topics.
    The MAPs are printed for DESIGN.md §14 (next to the reference's 0.3900 for QLM and 0.4094 for NVSM + QLM), not asserted."""
    out = str(tmp_path / "lse")
    r = run_trainer(["--word_repr_size", "64", "--entity_repr_size", "64", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
                     "--update_method", "full_adam", "--nonlinearity", "tanh", "--batch_size", "1024", "--num_epochs", "2", "--output", out, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    topics, qrels = os.path.join(GOLDEN, "cranfield.topics"), os.path.join(GOLDEN, "cranfield.qrel")
    common = ["--index", CRANFIELD, "--topics", topics, "--qrels", qrels]
    maps = {}
    for label, extra in (("nvsm", []), ("ensemble", ["--qlm", "jm", "--ensemble_alpha", "0.5", "--qlm_run_out", str(tmp_path / "qlm")])):
        run = str(tmp_path / ("run_" + label))
        q = run_query(common + extra + [out + "_2.hdf5", run])
        assert q.returncode == 0, q.stderr[-3000:]
        block = printed_metrics(q.stdout)[0]
        maps[label] = float(block["map"])
        assert int(block["num_q"]) > 200 and os.path.exists(run + "-cranfield.topics")
    rows = read_run(str(tmp_path / "qlm") + "-cranfield.topics")
    by_topic = {}
    for topic, docno, rank, score in rows:
        by_topic.setdefault(topic, []).append((int(docno), rank, score))
    assert len(by_topic) > 200
    for mine in by_topic.values():
        assert [r for _, r, _ in mine] == list(range(1, len(mine) + 1)) and (np.diff([s for _, _, s in mine]) <= 0).all()
        assert len({d for d, _, _ in mine}) == len(mine) <= 1000
    # the fused run of a topic is the union of its two runs
    nvsm, fused = read_run(str(tmp_path / "run_nvsm") + "-cranfield.topics"), read_run(str(tmp_path / "run_ensemble") + "-cranfield.topics")
    assert {d for t, d, _, _ in fused if t == "1"} == {d for t, d, _, _ in nvsm if t == "1"} | {str(d) for d, _, _ in by_topic["1"]}
    # the query-likelihood run's own MAP, by nvsm_evaluate's formulas (Cranfield's docnos are numbers: they serve as ids here)
    judged = {}
    with open(qrels) as f:
        for line in f:
            topic, _, docno, grade = line.split()
            judged.setdefault(topic, []).append((int(docno), int(grade)))
    aps = [er.evaluate_query([d for d, _, _ in mine], judged[t])["map"] for t, mine in by_topic.items()
           if any(g >= 1 for _, g in judged.get(t, []))]
    print("cranfield-map (LSE, 2 epochs, d = 64, 225 topics): NVSM %.4f, QLM (jm, auto) %.4f over %d topics, NVSM + QLM (alpha 0.5, standardize) %.4f"
          % (maps["nvsm"], float(np.mean(aps)), len(aps), maps["ensemble"]))
