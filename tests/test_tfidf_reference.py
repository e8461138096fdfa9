"""tests/tfidf_reference.py, the numpy restatement the GPU tests of nvsm_tfidf_rank are held against, held itself against a pure-Python
loop over documents written independently from the header's contract; and the share of (query, rank) slots whose order the
restatement alone leaves open on the collection the GPU tests rank (they allow 1 %)."""
import math

import numpy as np
import pytest

from tests import tfidf_reference as tr

# a dozen documents: an empty one, a one-token one, word 0 in every document that has words
DOCS = [[0, 3, 4, 3], [], [0], [5, 0, 5, 5, 6], [0, 1], [2, 0, 2], [0, 7, 8, 9, 1], [1, 0], [0, 0, 3], [9, 0, 4, 4, 4, 4], [0, 6], [3, 0, 1, 2]]
V = 12                                     # words 10 and 11 occur nowhere
QUERIES = [[0], [3], [3, 3], [4, 10, 1], [10, 11], [], [0, 5, 9, 0], [2, 1, 3]]
WEIGHTS = [[1.5], [0.0], [0.5, 2.0], [1.0, 3.0, 0.25], [1.0, 1.0], [], [0.0, 1.0, 0.0, 4.0], [1.0, 1.0, 1.0]]


def arena(docs):
    tokens = np.array([t for d in docs for t in d], np.int32)
    return tokens, np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)


def loop_ranking(docs, num_words, query, weights, k1, b, idf):
    """[(id, score)] of every matching document, best first: plain Python, one document at a time"""
    D, N = len(docs), sum(len(d) for d in docs)
    df = [sum(1 for d in docs if t in d) for t in range(num_words)]
    out = []
    for i, doc in enumerate(docs):
        score, hit = 0.0, False
        for j, t in enumerate(query):
            w = 1.0 if weights is None else float(np.float32(weights[j]))
            if not 0 <= t < num_words or df[t] == 0 or w == 0.0:
                continue
            tf = doc.count(t)
            if tf == 0:
                continue
            hit = True
            val = math.log((D + 1.0) / (df[t] + 0.5)) if idf == "robertson" else math.log((D - df[t] + 0.5) / (df[t] + 0.5))
            score += w * (val * tf * (k1 + 1.0) / (tf + k1 * (1.0 - b + b * len(doc) / (N / D))))
        if hit:
            out.append((i, score))
    return sorted(out, key=lambda e: (-e[1], e[0])), df


@pytest.mark.parametrize("idf", tr.IDFS)
@pytest.mark.parametrize("k1,b", [(None, None), (0.9, 0.4), (2.0, 1.0)])
@pytest.mark.parametrize("weighted", [False, True])
def test_the_restatement_equals_a_loop_over_documents(idf, k1, b, weighted):
    tokens, offsets = arena(DOCS)
    coll = tr.Collection(tokens, offsets, V)
    k1v, bv = tr.parameters(k1, b)
    for i, q in enumerate(QUERIES):
        w = WEIGHTS[i] if weighted else None
        want, df = loop_ranking(DOCS, V, q, w, k1v, bv, idf)
        np.testing.assert_array_equal(coll.df, df)
        order, scores, bound = tr.rank_query(coll, q, w, k1, b, idf)
        assert len(want) == order.size, (i, want, order)
        for (d, s), got in zip(want, order):
            # (two documents the loop ties exactly could only swap if the restatement did not tie them: ids are compared)
            assert d == got and abs(scores[got] - s) <= 1e-12 * max(1.0, abs(s)), (i, d, got, s, scores[got])
            assert bound[got] >= 0.0
    assert coll.df[0] == len(DOCS) - 1 and coll.df[10] == coll.df[11] == 0
    assert tr.idf_values(coll.df[0], len(DOCS), "okapi") < 0 < tr.idf_values(coll.df[0], len(DOCS), "robertson")


def test_the_gpu_collection_holds_what_the_gpu_tests_rely_on():
    tokens, offsets = tr.gpu_corpus()
    lens = offsets[1:] - offsets[:-1]
    D = lens.size
    coll = tr.Collection(tokens, offsets, tr.NUM_WORDS)
    assert (lens == 0).sum() == 1 and (lens == 1).sum() >= 1 and lens.max() > 2 * 256
    assert coll.df[tr.W_ALL] == D - 1 and D / 2 < coll.df[tr.W_HALF] < D - 1 and coll.df[tr.W_ABSENT] == 0
    long_doc = tokens[offsets[int(lens.argmax())]:offsets[int(lens.argmax()) + 1]]
    assert long_doc[0] == long_doc[-1] == tr.W_EDGE and (long_doc[1:-1] != tr.W_EDGE).all()
    assert tr.idf_values(coll.df[tr.W_ALL], D, "okapi") < 0 and tr.idf_values(coll.df[tr.W_HALF], D, "okapi") < 0
    queries = tr.gpu_queries(tokens)
    weights = tr.gpu_weights(queries)
    for idf in tr.IDFS:
        for w in (None, weights):
            for params in ({}, tr.EXPLICIT):
                for k in (1, 10, D):
                    left, total = tr.open_share(coll, queries, w, k, idf=idf, **params)
                    print("tfidf reference %s weighted=%s %s k=%d: %d of %d slots open" % (idf, w is not None, params, k, left, total))
                    assert total > 0 and left <= tr.SHARE * total, (idf, k, left, total)
