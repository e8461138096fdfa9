"""The core check of the inverted index: through every entry point that runs lexical rounds, ids, scores (compared as
uint32) and counts with the slabs filled from postings (use = "always") equal those of the arena scan (use = "never") bit for bit;
the profiler shows which fill ran; "auto" returns the same bits; and the hand-built collection of tests/test_gpu_lexical.py matches
the fp64 restatement directly through the postings."""
import numpy as np
import pytest

from tests import lexical_reference as lr
from tests.test_gpu_lexical import HAND_QUERIES, METHODS, check_ranking, hand_built, lexical_model
from tests.test_gpu_rank import bits

pytestmark = pytest.mark.gpu

SCAN = {"lex_score", "lex_score_weighted", "tfidf_score"}
POSTINGS = {"lex_postings", "lex_postings_weighted", "tfidf_postings"}


def flat(result):
    """a call's arrays, a metrics dict in front unfolded by name"""
    out = []
    for r in result:
        out += [r[k] for k in sorted(r)] if isinstance(r, dict) else [r]
    return out


def assert_same_bits(a, b, what):
    a, b = flat(a), flat(b)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=what)


def under(m, use, call):
    """the call's result with the index used as `use`, and the fill groups the profiler saw meanwhile"""
    m.index_corpus(use)
    m.profile_reset()
    result = call(m)
    return result, {n for n, (_, launches) in m.profile().items() if n in SCAN | POSTINGS and launches > 0}


def check_calls(m, calls, auto=True):
    for what, call, groups in calls:
        scan, seen = under(m, "never", call)
        assert seen and seen <= SCAN and seen == {g.replace("postings", "score") for g in groups}, (what, seen)
        post, seen = under(m, "always", call)
        assert seen == set(groups), (what, seen)
        assert_same_bits(scan, post, what)
        if auto:
            assert_same_bits(scan, under(m, "auto", call)[0], what + " (auto)")


# ---- about 3 000 documents, V = 2 000 of which the last ten words occur nowhere, 40 queries of 1 to 8 words ---------------------------
V, SEEN = 2000, 1990


def collection_a():
    tokens, offsets = lr.zipf_corpus(101, 3000, SEEN, max_len=60)
    rs = np.random.RandomState(102)
    present = np.flatnonzero(lr.collection_frequencies(tokens, V) > 0)
    queries = []
    for i in range(40):
        n = 1 + i % 8
        q = [int(t) for t in (tokens[rs.randint(0, tokens.size, n)] if i % 3 == 0 else present[rs.randint(0, present.size, n)])]
        queries.append(q)
    queries[5] = queries[5] + [queries[5][0]]                  # a repeated word
    queries[6] = [queries[6][0], SEEN + 3] + queries[6][1:]   # a word of cf = 0 among others
    queries[7] = []                                            # no words
    queries[8] = [SEEN, V - 1, SEEN + 1]                       # every word unseen
    queries[9] = [int(tokens[0]), int(tokens[0]), int(tokens[1]), int(tokens[0])]
    assert all(len(q) <= 9 for q in queries)
    return tokens, offsets, queries


def weights_for(queries, seed):
    rs = np.random.RandomState(seed)
    ws = [list(rs.uniform(0.25, 2.0, len(q)).astype(np.float32)) for q in queries]
    for w in ws[::4]:
        if len(w) > 1:
            w[1] = np.float32(0.0)                             # a term of weight 0 is dropped
    return ws


@pytest.fixture(scope="module")
def model_a():
    tokens, offsets, queries = collection_a()
    m = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    m.profile_enable(True)
    return m, tokens, offsets, queries


def test_lexical_and_tfidf_rank(model_a):
    m, tokens, offsets, queries = model_a
    ws = weights_for(queries, 103)
    assert any(0.0 in w for w in ws)
    calls = []
    for method, param in METHODS:
        calls.append(("lexical %s %s" % (method, param), lambda m, a=method, p=param: m.lexical_rank(queries, method=a, param=p, top_k=100), ["lex_postings"]))
        calls.append(("weighted %s %s" % (method, param), lambda m, a=method, p=param: m.lexical_rank(queries, method=a, param=p, top_k=100, weights=ws),
                      ["lex_postings_weighted"]))
    for idf in ("robertson", "okapi"):
        calls.append(("tfidf " + idf, lambda m, i=idf: m.tfidf_rank(queries, idf=i, top_k=100), ["tfidf_postings"]))
        calls.append(("weighted tfidf " + idf, lambda m, i=idf: m.tfidf_rank(queries, idf=i, k1=0.9, b=0.4, top_k=100, weights=ws), ["tfidf_postings"]))
    check_calls(m, calls)
    ids, scores, counts = m.lexical_rank(queries, top_k=3000)
    assert counts[7] == 0 and counts[8] == 0 and counts.max() > 100       # wordless, unseen; frequent words match many documents
    # ... and the postings fill alone against the fp64 restatement
    m.index_corpus("always")
    check_ranking(m.lexical_rank(queries, top_k=50), tokens, offsets, queries, "jm", None, 50, num_words=V)


def test_feedback_rerank_and_ensemble(model_a):
    m, tokens, offsets, queries = model_a
    rs = np.random.RandomState(104)
    judged = [[(int(d), int(g)) for d, g in zip(rs.choice(3000, 6, replace=False), rs.randint(0, 3, 6))] for _ in queries]
    calls = [
        ("relevance_model", lambda m: m.relevance_model(queries, fb_docs=8, fb_terms=12), ["lex_postings"]),
        ("lexical_rank_prf", lambda m: m.lexical_rank_prf(queries, fb_docs=8, fb_terms=12, top_k=100), ["lex_postings", "lex_postings_weighted"]),
        ("rerank tfidf", lambda m: m.rerank(queries, first_stage="tfidf", depth=64, top_k=20, judgments=judged, cutoffs=(5, 10)), ["tfidf_postings"]),
        ("rerank lexical", lambda m: m.rerank(queries, first_stage="lexical", method="dirichlet", depth=64, top_k=20, judgments=judged, cutoffs=(5, 10)),
         ["lex_postings"]),
        ("rank_ensemble", lambda m: m.rank_ensemble(queries, alpha=0.3, top_k=50), ["lex_postings"]),
        ("rank_ensemble_prf", lambda m: m.rank_ensemble(queries, alpha=0.3, top_k=50, feedback=dict(fb_docs=5, fb_terms=7, orig_weight=0.6)),
         ["lex_postings", "lex_postings_weighted"]),
    ]
    check_calls(m, calls)


# ---- 9 001 documents, 256 queries, three slabs of 4 096: postings straddle the slab edges ------------------------------------------
def test_three_slabs(monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")
    tokens, offsets = lr.zipf_corpus(9001, 9001, lr.NUM_WORDS)
    queries = lr.zipf_queries(9257, 256, lr.NUM_WORDS, tokens)
    edges = [0, 4095, 4096, 8191, 8192, 9000]                   # every slab's first and last column
    for i, d in enumerate(edges):
        queries[10 + i] = [int(tokens[offsets[d]])] + queries[10 + i][:2]
    queries[20] = [int(tokens[offsets[d]]) for d in edges]      # one query whose lists cross every edge
    for d in edges:
        assert set(tokens[offsets[d]:offsets[d + 1]]) & set(queries[20])
    m = lexical_model(9001, corpus=(tokens, offsets))
    m.profile_enable(True)
    check_calls(m, [("lexical", lambda m: m.lexical_rank(queries, top_k=9001), ["lex_postings"]),
                    ("tfidf", lambda m: m.tfidf_rank(queries, top_k=1000), ["tfidf_postings"])])
    (ids, scores, counts), _ = under(m, "always", lambda m: m.lexical_rank(queries, top_k=9001))
    for d in edges:
        assert d in ids[20, :counts[20]]
    groups = m.profile()["lex_postings"][1]
    assert groups >= 3 and groups % 3 == 0                      # one group per slab and round


def test_a_round_with_more_distinct_terms_than_slots_splits():
    tokens, offsets = lr.zipf_corpus(77, 1000, lr.NUM_WORDS)
    present = np.flatnonzero(lr.collection_frequencies(tokens, lr.NUM_WORDS) > 0)
    rs = np.random.RandomState(78)
    qs = [list(present[rs.randint(0, present.size, 5)]) for _ in range(300)]
    assert np.unique(np.concatenate(qs[:256])).size > 1024
    m = lexical_model(1000, corpus=(tokens, offsets))
    m.profile_enable(True)
    check_calls(m, [("lexical", lambda m: m.lexical_rank(qs, top_k=20), ["lex_postings"]),
                    ("tfidf", lambda m: m.tfidf_rank(qs, top_k=20), ["tfidf_postings"])], auto=False)
    assert m.profile()["tfidf_postings"][1] >= 2                # (the first round ends where its terms run out, not at 256 queries)


@pytest.mark.parametrize("method,param", METHODS)
def test_hand_built_collection_through_the_postings(method, param):
    tokens, offsets = hand_built()
    m = lexical_model(offsets.size - 1, corpus=(tokens, offsets))
    m.index_corpus("always")
    m.profile_enable(True)
    for k in (1, 3, offsets.size - 1):
        res = m.lexical_rank(HAND_QUERIES, method=method, param=param, top_k=k)
        check_ranking(res, tokens, offsets, HAND_QUERIES, method, param, k)
    ids, scores, counts = res
    assert counts[3] == 0 and counts[4] == 0
    assert list(ids[5]).index(5) + 1 == list(ids[5]).index(7) and not np.isin(ids, [0, 6]).any()
    np.testing.assert_array_equal(scores[1][:counts[1]], 2 * scores[0][:counts[0]])
    names = set(m.profile())
    assert "lex_postings" in names and not names & SCAN
