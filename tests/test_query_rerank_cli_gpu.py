"""-m gpu: cuNVSMQuery --rerank / --rerank_depth / --tfidf_run_out (cunvsm_amd/host/query_main.cpp) end to end, on the 70-document
collection, the checkpoint and the uploaded arena of tests/test_query_lexical_cli_gpu.py: the re-ranked run file and the printed
means equal Model.rerank's lists and metrics, the TF-IDF run file equals Model.tfidf_rank's, and the flag exclusions exit 1 with
their sentence."""
import os
import re

import numpy as np
import pytest

from tests import eval_reference as er
from tests.test_query_cli_gpu import CUTOFFS, assert_same_run, base_args, expected_rows, printed_metrics, read_run, run_query
from tests.test_query_lexical_cli_gpu import corpus, kept_queries  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STAGES = {"tfidf": dict(first_stage="tfidf", idf="robertson"), "okapi": dict(first_stage="tfidf", idf="okapi"),
          "jm": dict(first_stage="lexical", method="jm"), "dirichlet": dict(first_stage="lexical", method="dirichlet")}


@pytest.mark.parametrize("stage,depth,top_k", [("tfidf", 20, 5), ("okapi", 30, None), ("jm", 10, 10), ("dirichlet", None, 7)])
def test_the_reranked_run_and_the_printed_means_are_reranks(corpus, tmp_path, stage, depth, top_k):  # noqa: F811
    out, tfidf = str(tmp_path / "run"), str(tmp_path / "tfidf")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    extra = ["--rerank", stage, "--qrels", corpus.qrel_path, "--tfidf_run_out", tfidf]
    if depth:
        extra += ["--rerank_depth", str(depth)]
    if top_k:
        extra += ["--top_k", str(top_k)]
    r = run_query(flags + extra + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = printed_metrics(r.stdout)
    assert len(blocks) == 2
    d = min(depth or 1000, corpus.D)                                          # clipped to the collection, as --top_k is
    k = min(top_k or 1000, corpus.D, d)                                       # ... and a topic has no more results than candidates
    for name, block in zip(("topics_a", "topics_b"), blocks):
        kept, queries = kept_queries(corpus, name)
        judged = [corpus.judged_ids(t) for t, _ in kept]
        res, ids, scores, counts = corpus.model.rerank(queries, depth=d, top_k=k, judgments=judged, cutoffs=CUTOFFS, bias_coefficient=0.0,
                                                       activation="tanh", **STAGES[stage])
        assert ids.shape[1] == k and (counts > 0).all()
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, kept, ids, scores, counts))
        # the first stage's own run: TF-IDF at the depth (Okapi's idf with --rerank okapi)
        first = corpus.model.tfidf_rank(queries, idf="okapi" if stage == "okapi" else "robertson", top_k=d)
        assert (first[2] < corpus.D).any()                                    # only documents that hold a query word are retrieved
        assert_same_run(read_run("%s-%s" % (tfidf, name)), expected_rows(corpus, kept, *first))
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


def test_the_tfidf_run_alone_leaves_the_nvsm_run_as_it_was(corpus, tmp_path):  # noqa: F811
    out, tfidf = str(tmp_path / "run"), str(tmp_path / "tfidf")
    flags, positional = base_args(corpus, out, "topics_a")
    r = run_query(flags + ["--tfidf_run_out", tfidf, "--top_k", "12"] + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    kept, queries = kept_queries(corpus, "topics_a")
    assert_same_run(read_run(tfidf + "-topics_a"), expected_rows(corpus, kept, *corpus.model.tfidf_rank(queries, top_k=12)))
    ids, scores, counts = corpus.model.rank(queries, top_k=12, bias_coefficient=0.0, activation="tanh")
    assert_same_run(read_run(out + "-topics_a"), expected_rows(corpus, kept, ids, scores, counts))
    assert r.stdout == ""


def test_refusals_and_the_help_text(corpus, tmp_path):  # noqa: F811
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_b")
    for extra, word in ((["--rerank", "bm25"], "--rerank: 'bm25' is none of tfidf, okapi, jm, dirichlet"),
                        (["--rerank", "tfidf", "--qlm", "jm", "--ensemble_alpha", "0.5"], "--rerank and --ensemble_alpha / --ensemble_qrel are mutually exclusive"),
                        (["--rerank", "tfidf", "--qlm", "jm", "--ensemble_qrel", corpus.qrel_path],
                         "--rerank and --ensemble_alpha / --ensemble_qrel are mutually exclusive"),
                        (["--rerank", "tfidf", "--rerank_depth", "0"], "--rerank_depth must be in [1, 4096]"),
                        (["--rerank", "tfidf", "--rerank_depth", "4097"], "--rerank_depth must be in [1, 4096]"),
                        (["--rerank_depth", "50"], "--rerank_depth needs --rerank"),
                        (["--rerank", "tfidf", "--top_k", corpus.qrel_path], "--top_k"),
                        (["--tfidf_run_out", out, "--top_k", corpus.qrel_path], "--top_k"),
                        (["--rerank_exact_matching_documents"], "--rerank tfidf")):
        r = run_query(flags + extra + positional)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics_b")
    r = run_query(["--help"])
    assert r.returncode == 0 and r.stdout.count("NOT OFFERED") == 3
    for flag in ("rerank", "rerank_depth", "tfidf_run_out"):
        assert "-%s (" % flag in r.stdout
