"""The fp64 restatement of weighted query likelihood, the relevance model and the RM3 expansion (tests/prf_reference.py) against a
hand-computed example and its own invariances, and — from the restatement alone — the share of positions whose order the contract
leaves open on the inputs tests/test_gpu_prf.py uses: at most 1 %, so that a GPU failure there is never an input problem."""
import numpy as np
import pytest

from tests import lexical_reference as lr
from tests import prf_reference as pr

_collections = {}


def case(documents, queries):
    if (documents, queries) not in _collections:
        _collections.clear()
        tokens, offsets, qs = lr.case_inputs(documents, queries)
        _collections[(documents, queries)] = (lr.Collection(tokens, offsets, pr.NUM_WORDS), qs)
    return _collections[(documents, queries)]


def test_a_hand_computed_three_document_example():
    """Documents d0 = [0 0 1], d1 = [0 2], d2 = [3]: N = 6, cf = (3, 1, 1, 1), p = (1/2, 1/6, 1/6, 1/6). Query [0], Jelinek-Mercer, auto
    (lambda 1/2):
      s(d0) = log(1/2 · 2/3 + 1/2 · 1/2) = log(7/12),  s(d1) = log(1/2 · 1/2 + 1/4) = log(1/2),  d2 does not hold word 0.
    Feedback documents (fb_docs 2): d0, d1 with w0 = 1, w1 = exp(s1 − s0) = (1/2) / (7/12) = 6/7, sum 13/7:
      pi(0) = (2/3 + 6/7 · 1/2) / (13/7) = 23/39,  pi(1) = (1/3) / (13/7) = 7/39,  pi(2) = (6/7 · 1/2) / (13/7) = 9/39.
    Expansion terms (fb_terms 2): word 0 (23/39), word 2 (9/39); S = 32/39. With orig_weight 1/2 and L = 1 the expanded query is
      [0, 0, 2] with weights [1/2, 1/2 · 23/32, 1/2 · 9/32] = [32/64, 23/64, 9/64].
    Its scores: word 2 has tf 0 in d0 — log(1/2 · 1/6) = log(1/12) — and tf 1 in d1 — log(1/2 · 1/2 + 1/12) = log(1/3):
      s(d0) = 55/64 · log(7/12) + 9/64 · log(1/12) = −0.813,  s(d1) = 55/64 · log(1/2) + 9/64 · log(1/3) = −0.750;  d2 holds neither
    word. Feedback turns the order round: d1 holds the expansion term 2, d0 does not."""
    coll = lr.Collection([0, 0, 1, 0, 2, 3], [0, 3, 5, 6], 6)
    ids, sc = pr.first_pass(coll, [0], "jm", None, 2)
    assert list(ids) == [0, 1] and sc.dtype == np.float32
    np.testing.assert_allclose(sc, [np.log(7 / 12), np.log(1 / 2)], rtol=2e-7)
    terms, pi, bound = pr.relevance_model(coll, ids, sc, 2)
    assert list(terms) == [0, 2]
    np.testing.assert_allclose(pi, [23 / 39, 7 / 39, 9 / 39, 0, 0, 0], rtol=1e-6)        # (w1 comes from float32 scores)
    assert abs(pi.sum() - 1.0) < 1e-15
    words, weights = pr.expand(coll, [0], terms, pi[terms].astype(np.float32), 0.5)
    assert words == [0, 0, 2] and weights.dtype == np.float32
    np.testing.assert_allclose(weights, [32 / 64, 23 / 64, 9 / 64], rtol=1e-6)
    assert weights[0] == np.float32(0.5)
    order, scores, bound = pr.weighted_rank_query(coll, words, weights, "jm", None)
    assert list(order) == [1, 0]
    np.testing.assert_allclose(scores[:2], [55 / 64 * np.log(7 / 12) + 9 / 64 * np.log(1 / 12), 55 / 64 * np.log(1 / 2) + 9 / 64 * np.log(1 / 3)],
                               rtol=1e-6)
    np.testing.assert_array_equal(bound, lr.EPS * np.abs(scores))
    # Dirichlet, mu = 3: s(d0) = log((2 + 3/2) / 6) = log(7/12) and s(d1) = log((1 + 3/2) / 5) = log(1/2) as well
    ids, sc = pr.first_pass(coll, [0], "dirichlet", 3.0, 2)
    np.testing.assert_allclose(sc, [np.log(7 / 12), np.log(1 / 2)], rtol=2e-7)


def test_weights_all_one_are_the_unweighted_restatement():
    coll, qs = case(1000, 300)
    for method, param in (("jm", None), ("dirichlet", None), ("jm", lr.EXPLICIT["jm"]), ("dirichlet", lr.EXPLICIT["dirichlet"])):
        for q in qs[:60]:
            plain, matched, _ = lr.score_query(coll, q, method, param)
            scores, also, bound = pr.weighted_score_query(coll, q, [1.0] * len(q), method, param)
            np.testing.assert_array_equal(scores, plain)
            np.testing.assert_array_equal(also, matched)
            halves, _, _ = pr.weighted_score_query(coll, q, [0.5] * len(q), method, param)
            np.testing.assert_array_equal(halves, 0.5 * plain)
            # the weighted bound is the tighter one
            assert (bound[matched] <= lr.score_query(coll, q, method, param)[2][matched]).all()
    # a weight 0 drops the term, from the score and from the retrieved set
    q = next(q for q in qs if len(pr.remaining(coll, q)) >= 2 and len(set(q)) == len(q))
    a = pr.weighted_rank_query(coll, q, [0.0] + [1.0] * (len(q) - 1), "jm", None)
    b = lr.rank_query(coll, q[1:], "jm", None)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert pr.weighted_rank_query(coll, q, [0.0] * len(q), "jm", None)[0].size == 0


def test_one_feedback_document_gives_tf_over_len():
    coll, qs = case(1000, 300)
    seen = 0
    for q in qs[:80]:
        ids, sc = pr.first_pass(coll, q, "jm", None, 1)
        terms, pi, _ = pr.relevance_model(coll, ids, sc, 5)
        if ids.size == 0:
            assert terms.size == 0 and not pi.any()
            continue
        d = int(ids[0])
        doc = coll.tokens[coll.offsets[d]:coll.offsets[d + 1]]
        np.testing.assert_array_equal(pi, np.bincount(doc, minlength=coll.num_words) / float(doc.size))
        assert terms.size == min(5, np.unique(doc).size) and (np.diff(pi[terms]) <= 0).all()
        tied = pi[terms][:-1] == pi[terms][1:]
        assert (terms[:-1][tied] < terms[1:][tied]).all()
        seen += 1
    assert seen > 50


def test_orig_weight_0_and_1_drop_the_other_group():
    coll, qs = case(1000, 300)
    for q in qs[:40]:
        kept = pr.remaining(coll, q)
        ids, sc = pr.first_pass(coll, q, "jm", None, 10)
        terms, pi, _ = pr.relevance_model(coll, ids, sc, 10)
        probs = pi[terms].astype(np.float32)
        words, w = pr.expand(coll, q, terms, probs, 1.0)
        assert words == kept + list(terms) and (w[len(kept):] == 0).all() and (w[:len(kept)] == np.float32(1.0 / len(kept))).all()
        np.testing.assert_array_equal(pr.weighted_score_query(coll, words, w, "jm", None)[0],
                                      pr.weighted_score_query(coll, kept, w[:len(kept)], "jm", None)[0])
        words, w = pr.expand(coll, q, terms, probs, 0.0)
        assert (w[:len(kept)] == 0).all() and abs(float(w[len(kept):].astype(np.float64).sum()) - 1.0) < 1e-6
        np.testing.assert_array_equal(pr.weighted_score_query(coll, words, w, "jm", None)[0],
                                      pr.weighted_score_query(coll, list(terms), w[len(kept):], "jm", None)[0])
        words, w = pr.expand(coll, q, terms, probs, 0.5)
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6        # o + (1 - o)
    absent = int(np.flatnonzero(coll.cf == 0)[0])
    assert pr.expand(coll, [absent, -4, pr.NUM_WORDS], [], [], 0.5)[0] == []      # nothing remains: the query stays empty


@pytest.mark.parametrize("documents,queries", pr.CASES)
def test_the_gpu_tests_inputs_leave_at_most_one_percent_open(documents, queries):
    """the first pass simulated by the restatement's scores narrowed to float32; auto parameters, orig_weight 0.5"""
    coll, qs = case(documents, queries)
    assert pr.SHARE == 0.01
    for method, param in pr.METHODS:
        for fb in pr.FEEDBACK:
            fb_docs, fb_terms = pr.fb_of(documents, fb)
            (left, total), deep = pr.open_shares(coll, qs, method, param, fb_docs, fb_terms, pr.ORIG_WEIGHT, pr.TOP_KS)
            assert left <= pr.SHARE * total, ("A", method, fb, left, total)
            for k, (b_left, b_total) in deep.items():
                assert b_left <= pr.SHARE * b_total, ("B", method, fb, k, b_left, b_total)
            print("D=%d Q=%d %s fb=%s: A %d of %d open, B %s" % (documents, queries, method, fb, left, total, deep))
    if documents >= 1000:       # the premises of the GPU tests: queries that retrieve fewer documents than fb_docs, and none
        found = [lr.rank_query(coll, q, "jm", None)[0].size for q in qs]
        assert min(found) < 10 and max(found) > 100
