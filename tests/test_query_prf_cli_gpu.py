"""-m gpu: cuNVSMQuery --qlm_prf (cunvsm_amd/host/query_main.cpp) end to end. On the 70-document collection and the checkpoint of
tests/test_query_lexical_cli_gpu.py: the query-likelihood run file written with --qlm_prf equals Model.lexical_rank_prf on the same
topics, the fused run file and the printed means equal Model.rank_ensemble(feedback=...)'s. On Cranfield, with the collection's own
topics and judgments: the MAPs of QLM, QLM with feedback and the fusion are printed for DESIGN.md §16 and not asserted (tokenisation,
stopping, the vocabulary cut and the relevance model's settings differ from the reference's Indri run)."""
import os
import re

import numpy as np
import pytest

from tests import eval_reference as er
from tests.test_query_cli_gpu import CUTOFFS, assert_same_run, base_args, expected_rows, printed_metrics, read_run, run_query
from tests.test_query_lexical_cli_gpu import GOLDEN, corpus, kept_queries      # noqa: F401  (corpus: the module's fixture)
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method,fb", [("jm", None), ("dirichlet", (3, 5, 0.7)), ("jm", (70, 4, 0.0))])
def test_the_feedback_run_is_lexical_rank_prfs(corpus, tmp_path, method, fb):      # noqa: F811
    out, qlm = str(tmp_path / "run"), str(tmp_path / "qlm")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    extra = ["--qlm", method, "--qlm_prf", "--qlm_run_out", qlm]
    if fb:
        extra += ["--qlm_fb_docs", str(fb[0]), "--qlm_fb_terms", str(fb[1]), "--qlm_fb_orig_weight", str(fb[2])]
    fb_docs, fb_terms, orig_weight = fb or (10, 10, 0.5)
    r = run_query(flags + extra + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("topics_a", "topics_b"):
        kept, queries = kept_queries(corpus, name)
        ids, scores, counts = corpus.model.lexical_rank_prf(queries, fb_docs=min(fb_docs, corpus.D), fb_terms=fb_terms, orig_weight=orig_weight,
                                                            method=method, top_k=corpus.D)
        assert (counts > 0).all()
        assert_same_run(read_run("%s-%s" % (qlm, name)), expected_rows(corpus, kept, ids, scores, counts))
        plain = corpus.model.lexical_rank(queries, method=method, top_k=corpus.D)
        assert not np.array_equal(scores, plain[1])
        if orig_weight > 0:                                                   # the original terms stay: at least what the query retrieved
            assert (counts >= plain[2]).all()
        # without --ensemble_alpha <run_out> is the NVSM run it always was
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, *corpus.expected(name)))
    assert r.stdout == ""


def test_the_fused_run_and_the_printed_means_use_the_feedback_list(corpus, tmp_path):      # noqa: F811
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    r = run_query(flags + ["--qlm", "jm", "--qlm_prf", "--qlm_fb_docs", "5", "--ensemble_alpha", "0.4", "--qrels", corpus.qrel_path, "--top_k", "20"]
                  + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = printed_metrics(r.stdout)
    assert len(blocks) == 2
    for name, block in zip(("topics_a", "topics_b"), blocks):
        kept, queries = kept_queries(corpus, name)
        judged = [corpus.judged_ids(t) for t, _ in kept]
        res, ids, scores, counts = corpus.model.rank_ensemble(queries, alpha=0.4, judgments=judged, top_k=20, cutoffs=CUTOFFS, bias_coefficient=0.0,
                                                              activation="tanh", feedback=dict(fb_docs=5))
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, kept, ids, scores, counts))
        ref = er.evaluate(ids, counts, judged, CUTOFFS)
        evaluated = ref["num_rel"] > 0
        assert block["num_q"] == str(int(evaluated.sum()))
        for metric in er.names(CUTOFFS):
            if metric in er.INTEGER:
                assert block[metric] == str(int(ref[metric][evaluated].sum())), metric
            else:
                assert re.fullmatch(r"\d\.\d{4}", block[metric]), block[metric]
                assert abs(float(block[metric]) - ref[metric][evaluated].mean()) <= 0.5e-4 + 1e-9, metric


def test_refusals_and_the_help_text(corpus, tmp_path):      # noqa: F811
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_b")
    for extra, word in ((["--qlm_prf"], "--qlm_prf needs --qlm"), (["--qlm", "jm", "--qlm_run_out", out, "--qlm_fb_docs", "3"], "need --qlm_prf"),
                        (["--qlm", "jm", "--qlm_run_out", out, "--qlm_fb_terms", "3"], "need --qlm_prf"),
                        (["--qlm", "jm", "--qlm_run_out", out, "--qlm_fb_orig_weight", "0.3"], "need --qlm_prf"),
                        (["--qlm", "jm", "--qlm_prf", "--qlm_run_out", out, "--qlm_fb_docs", "0"], "--qlm_fb_docs"),
                        (["--qlm", "jm", "--qlm_prf", "--qlm_run_out", out, "--qlm_fb_docs", "1025"], "--qlm_fb_docs"),
                        (["--qlm", "jm", "--qlm_prf", "--qlm_run_out", out, "--qlm_fb_terms", "0"], "--qlm_fb_terms"),
                        (["--qlm", "jm", "--qlm_prf", "--qlm_run_out", out, "--qlm_fb_orig_weight", "1.5"], "--qlm_fb_orig_weight")):
        r = run_query(flags + extra + positional)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics_b")
    r = run_query(["--help"])
    assert r.returncode == 0
    for flag in ("qlm_prf", "qlm_fb_docs", "qlm_fb_terms", "qlm_fb_orig_weight"):
        assert "-%s (" % flag in r.stdout


def test_cranfield_query_likelihood_with_feedback(tmp_path):
    """two epochs of LSE on Cranfield, then the query-likelihood run without and with feedback and the fusion of the NVSM run with the
    feedback run over the collection's 225 topics. The MAPs are printed for DESIGN.md §16 (next to the reference tutorial's 0.3900 ->
    0.4163 for QLM with Jelinek-Mercer smoothing and 0.4345 for the fusion), not asserted."""
    out = str(tmp_path / "lse")
    r = run_trainer(["--word_repr_size", "64", "--entity_repr_size", "64", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
                     "--update_method", "full_adam", "--nonlinearity", "tanh", "--batch_size", "1024", "--num_epochs", "2", "--output", out, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    topics, qrels = os.path.join(GOLDEN, "cranfield.topics"), os.path.join(GOLDEN, "cranfield.qrel")
    common = ["--index", CRANFIELD, "--topics", topics, "--qrels", qrels]
    q = run_query(common + ["--qlm", "jm", "--qlm_run_out", str(tmp_path / "qlm"), out + "_2.hdf5", str(tmp_path / "run_nvsm")])
    assert q.returncode == 0, q.stderr[-3000:]
    q = run_query(common + ["--qlm", "jm", "--qlm_prf", "--qlm_run_out", str(tmp_path / "prf"), "--ensemble_alpha", "0.5", out + "_2.hdf5",
                            str(tmp_path / "run_fused")])
    assert q.returncode == 0, q.stderr[-3000:]
    fused = printed_metrics(q.stdout)[0]
    assert int(fused["num_q"]) > 200
    judged = {}
    with open(qrels) as f:
        for line in f:
            topic, _, docno, grade = line.split()
            judged.setdefault(topic, []).append((int(docno), int(grade)))
    maps = {}
    for label in ("qlm", "prf"):
        by_topic = {}
        for topic, docno, rank, score in read_run(str(tmp_path / label) + "-cranfield.topics"):
            by_topic.setdefault(topic, []).append((int(docno), rank, score))
        assert len(by_topic) > 200
        for mine in by_topic.values():
            assert [r for _, r, _ in mine] == list(range(1, len(mine) + 1)) and (np.diff([s for _, _, s in mine]) <= 0).all()
            assert len({d for d, _, _ in mine}) == len(mine) <= 1000
        aps = [er.evaluate_query([d for d, _, _ in mine], judged[t])["map"] for t, mine in by_topic.items()
               if any(g >= 1 for _, g in judged.get(t, []))]
        maps[label] = float(np.mean(aps))
    print("cranfield-map (LSE, 2 epochs, d = 64, 225 topics; jm, auto; feedback 10 documents, 10 terms, original weight 0.5): QLM %.4f, "
          "QLM + PRF %.4f, NVSM + QLM + PRF (alpha 0.5, standardize) %.4f" % (maps["qlm"], maps["prf"], float(fused["map"])))
