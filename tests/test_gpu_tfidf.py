"""nvsm_tfidf_rank on the GPU against the fp64 restatement of its contract (tests/tfidf_reference.py): the df table exactly (through
the hook, at slabs of 32, 33 and more documents than there are), counts equal, every score within 2^-23 sum |w a| of the
restatement, every list ordered by (float32 score descending, id ascending), ids equal except where the restatement's own
neighbouring scores are closer than twice the bound (at most 1 % of the slots; tests/test_tfidf_reference.py checks on the CPU that
the restatement alone stays under that), the identities of the contract, training and nvsm_lexical_rank undisturbed, every refusal."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import lexical_reference as lr
from tests import tfidf_reference as tr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu

V = tr.NUM_WORDS
TOKENS, OFFSETS = tr.gpu_corpus()
D = OFFSETS.size - 1
QUERIES = tr.gpu_queries(TOKENS)
WEIGHTS = tr.gpu_weights(QUERIES)
_COLL = tr.Collection(TOKENS, OFFSETS, V)
_references = {}


def reference(i, weighted, idf, params):
    """a query's restatement ranking: computed once, shared among the top_k values and the tests, never changed"""
    key = (i, weighted, idf, tuple(sorted(params.items())))
    if key not in _references:
        _references[key] = tr.rank_query(_COLL, QUERIES[i], WEIGHTS[i] if weighted else None, idf=idf, **params)
    return _references[key]


def check_ranking(result, weighted, idf, params, top_k):
    ids, scores, counts = result
    assert ids.shape == scores.shape == (len(QUERIES), top_k) and counts.shape == (len(QUERIES),)
    left = total = 0
    worst = 0.0
    for i in range(len(QUERIES)):
        order, ref, bound = reference(i, weighted, idf, params)
        n = min(top_k, order.size)
        assert counts[i] == n, (i, counts[i], n)
        assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
        if n == 0:
            continue
        got = ids[i, :n]
        assert got.min() >= 0 and np.unique(got).size == n
        err = np.abs(scores[i, :n].astype(np.float64) - ref[got])
        assert (err <= bound[got]).all(), (i, float((err / bound[got]).max()))
        worst = max(worst, float((err / bound[got]).max()))
        sc = scores[i, :n]                                                    # ordered by (float32 score descending, id ascending)
        assert (sc[:-1] >= sc[1:]).all() and (got[:-1][sc[:-1] == sc[1:]] < got[1:][sc[:-1] == sc[1:]]).all()
        open_ = lr.excused(ref[order], bound[order])[:n]
        differ = got != order[:n]
        assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
        left += int(open_.sum())
        total += n
    print("tfidf %s weighted=%s %s k=%d: %d of %d slots left out, worst error %.3g of the bound" % (idf, weighted, params, top_k, left, total, worst))
    assert left <= tr.SHARE * total, (left, total)


@pytest.fixture(scope="module")
def model():
    return lexical_model(D, num_words=V, corpus=(TOKENS, OFFSETS))


# ---- df ---------------------------------------------------------------------------------------------------------------------------------
def debug_df(tokens, offsets, num_words, slab):
    df = np.full(num_words, -7, np.int64)
    tokens, offsets = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(offsets, np.int64)
    st = ca.lib().nvsm_debug_lex_df(tokens.ctypes.data, tokens.size, offsets.ctypes.data, offsets.size - 1, num_words, slab, df.ctypes.data)
    return st, df


@pytest.mark.parametrize("slab", [32, 33, D + 126])
def test_the_df_table_is_exact_at_every_slab(slab):
    """32: one bit word per row and three slabs; 33: the second word of a row begins, and the slabs do not divide the documents; more
    than the corpus: one slab. The long document's edge word lies in two chunks of its wave's loop and counts once."""
    st, df = debug_df(TOKENS, OFFSETS, V, slab)
    assert st == 0, ca.lib().nvsm_last_error()
    np.testing.assert_array_equal(df, _COLL.df)
    assert df[tr.W_EDGE] == 2 and df[tr.W_ALL] == D - 1 and df[tr.W_ABSENT] == 0


def test_the_df_hook_refuses_a_broken_corpus():
    for tokens, offsets, slab in ((TOKENS, OFFSETS[::-1], 32), (np.array([V], np.int32), np.array([0, 1]), 32), (TOKENS, OFFSETS, 0)):
        st, df = debug_df(tokens, offsets, V, slab)
        assert st == 1 and (df == -7).all()


# ---- scores, retrieved set, order -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idf", tr.IDFS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("params", [{}, tr.EXPLICIT], ids=["auto", "explicit"])
def test_scores_sets_and_order(model, idf, weighted, params):
    for k in (1, 10, D):                                                       # D: more than any query matches (a document is empty)
        res = model.tfidf_rank(QUERIES, idf=idf, top_k=k, weights=WEIGHTS if weighted else None, **params)
        check_ranking(res, weighted, idf, params, k)
    ids, scores, counts = res
    assert (counts < D).all()
    by = {tuple(q): i for i, q in enumerate(QUERIES)}
    assert counts[by[(tr.W_ABSENT,)]] == 0 and counts[by[()]] == 0            # only absent terms; no words
    if not weighted:
        assert counts[by[(tr.W_ALL,)]] == D - 1                                # the empty document is never retrieved
        assert counts[by[(tr.W_EDGE,)]] == 2
        if idf == "okapi":
            assert (scores[by[(tr.W_ALL,)], :D - 1] < 0).all()                 # df > D_c / 2: a negative idf, reproduced as it is


def test_identities(model):
    for idf in tr.IDFS:
        plain = model.tfidf_rank(QUERIES, idf=idf, top_k=D)
        same_bits(plain, model.tfidf_rank(QUERIES, idf=idf, top_k=D))         # a repeated call
        ones = [np.ones(len(q), np.float32) for q in QUERIES]
        same_bits(plain, model.tfidf_rank(QUERIES, idf=idf, top_k=D, weights=ones))
        for scale in (4.0, 0.125):
            # a power of two on every term: every product and every partial sum scales exactly, and so does the narrowed score
            ids, scores, counts = model.tfidf_rank(QUERIES, idf=idf, top_k=D, weights=[scale * w for w in ones])
            np.testing.assert_array_equal(ids, plain[0])
            np.testing.assert_array_equal(counts, plain[2])
            np.testing.assert_array_equal(scores, np.float32(scale) * plain[1])
    # a repeated word counts once per occurrence: a + a is exact, so [e, e] scores twice [e], bit for bit
    one, two = model.tfidf_rank([[tr.W_EDGE]], top_k=5), model.tfidf_rank([[tr.W_EDGE, tr.W_EDGE]], top_k=5)
    np.testing.assert_array_equal(two[0], one[0])
    np.testing.assert_array_equal(two[1][0, :2], 2 * one[1][0, :2])


def test_lexical_rank_is_the_same_before_and_after_and_an_upload_renews_the_table(model):
    fresh = lexical_model(D, num_words=V, corpus=(TOKENS, OFFSETS))
    before = fresh.lexical_rank(QUERIES, top_k=10)
    res = fresh.tfidf_rank(QUERIES, top_k=10)
    same_bits(before, fresh.lexical_rank(QUERIES, top_k=10))
    same_bits(res, model.tfidf_rank(QUERIES, top_k=10))
    assert fresh.describe() == lexical_model(D, num_words=V, corpus=(TOKENS, OFFSETS)).describe()      # what the call allocated is not in the text
    other = ((TOKENS[::-1].astype(np.int64) + 7) % tr.ZIPF_WORDS).astype(np.int32)
    fresh.upload_corpus(ca.Corpus(other, OFFSETS))
    coll = tr.Collection(other, OFFSETS, V)
    assert (coll.df != _COLL.df).any()
    ids, scores, counts = fresh.tfidf_rank([[5, 9]], top_k=D)
    order, ref, bound = tr.rank_query(coll, [5, 9])
    assert counts[0] == order.size and set(ids[0, :counts[0]].tolist()) == set(order.tolist())
    assert (np.abs(scores[0, :counts[0]] - ref[ids[0, :counts[0]]]) <= bound[ids[0, :counts[0]]]).all()
    fresh.upload_corpus(None)
    with pytest.raises(ca.NvsmError) as e:
        fresh.tfidf_rank([[5]], top_k=5)
    assert e.value.status == 1 and "corpus" in str(e.value)


def test_a_tfidf_call_between_steps_never_disturbs_training():
    spec = dict(num_words=V, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    models = []
    for _ in range(2):
        m = gpu_model(spec, 64)
        load_params(m, random_params(spec, np.random.RandomState(9)), True)
        m.upload_corpus(ca.Corpus(TOKENS, OFFSETS))
        models.append(m)
    a, b = models
    rs = np.random.RandomState(10)
    first = None
    for words, ww, labels, iw, ids in [random_batch(spec, rs, 64, zipf=True) for _ in range(4)]:
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        res = a.tfidf_rank(QUERIES, top_k=20)                                  # straight behind nvsm_step
        if first is None:
            first = res
        same_bits(first, res)                                                  # a function of corpus and query, not of the parameters
    check_ranking(res, False, "robertson", {}, 20)
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def raw_tfidf(m, k1=0.0, b=0.0, idf=0, top_k=5, words=(1, 2, 3), word_offsets=(0, 2, 3), weights=None, null=None):
    w, off = np.asarray(words, np.int64), np.asarray(word_offsets, np.int64)
    wt = None if weights is None else np.asarray(weights, np.float32)
    Q = off.size - 1
    q = ca.NvsmQueries(w.ctypes.data, None if wt is None else wt.ctypes.data, None if null == "offsets" else off.ctypes.data, Q)
    o = ca.NvsmTfidfOptions()
    ca.lib().nvsm_tfidf_options_default(C.byref(o))
    o.k1, o.b, o.idf, o.top_k = k1, b, idf, top_k
    ids = np.full((Q, max(top_k, 1)), -7, np.int64)
    scores = np.full((Q, max(top_k, 1)), -7.0, np.float32)
    counts = np.full(Q, -7, np.int64)
    ptr = lambda name, a: None if null == name else a.ctypes.data
    st = ca.lib().nvsm_tfidf_rank(m._h, None if null == "queries" else C.byref(q), None if null == "opt" else C.byref(o),
                                  ptr("doc_ids", ids), ptr("scores", scores), ptr("counts", counts))
    return st, (ids, scores, counts)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    m = lexical_model(D, num_words=V)
    L = ca.lib()
    st, _ = raw_tfidf(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()          # no corpus uploaded
    m.upload_corpus(ca.Corpus(TOKENS, OFFSETS))
    nan, inf = float("nan"), float("inf")
    bad = [
        (dict(idf=2), b"idf"), (dict(idf=-1), b"idf"),
        (dict(k1=-0.5), b"k1"), (dict(k1=nan), b"k1"), (dict(k1=inf), b"k1"),
        (dict(b=-0.1), b"b must"), (dict(b=1.5), b"b must"), (dict(b=nan), b"b must"),
        (dict(top_k=0), b"top_k"), (dict(top_k=D + 1), b"top_k"),
        (dict(weights=(1.0, -1.0, 1.0)), b"weight is negative"), (dict(weights=(1.0, nan, 1.0)), b"weight is not finite"),
        (dict(word_offsets=(0, 3, 2)), b"queries->offsets decrease"), (dict(word_offsets=(1, 2, 3)), b"offsets[0]"),
        (dict(null="queries"), b"null argument: queries"), (dict(null="opt"), b"null argument: opt"),
        (dict(null="doc_ids"), b"null argument: doc_ids"), (dict(null="scores"), b"null argument: scores"),
        (dict(null="counts"), b"null argument: counts"), (dict(null="offsets"), b"null argument: queries->offsets"),
    ]
    for kwargs, word in bad:
        st, out = raw_tfidf(m, **kwargs)
        assert st == 1 and word in L.nvsm_last_error(), (kwargs, L.nvsm_last_error())
        assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_tfidf(m)
        assert st == 0 and (out[2] >= 0).all()
    # a word id out of range matches nothing, and the call says so
    st, out = raw_tfidf(m, words=(1, V, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error()
    same_bits(out, raw_tfidf(m, words=(1, 3), word_offsets=(0, 1, 2))[1])
    # more distinct terms than a round has counters for
    wide = np.arange(ca._lib.LEXICAL_MAX_QUERY_TERMS + 1) % V
    m2 = lexical_model(D, num_words=2000, corpus=(TOKENS, OFFSETS))
    st, out = raw_tfidf(m2, words=np.arange(ca._lib.LEXICAL_MAX_QUERY_TERMS + 1), word_offsets=(0, ca._lib.LEXICAL_MAX_QUERY_TERMS + 1))
    assert st == 2 and b"distinct terms" in L.nvsm_last_error() and all((a == -7).all() for a in out)
    assert raw_tfidf(m, words=wide, word_offsets=(0, wide.size))[0] == 0     # ... distinct ones: repeats do not count
    assert raw_tfidf(m, k1=2.0, b=1.0, idf=1)[0] == 0                        # b = 1 is inside its range
    for kwargs in (dict(idf="bm25"), dict(k1=-1.0), dict(b=1.5), dict(top_k=0)):
        with pytest.raises(ValueError):
            m.tfidf_rank([[1]], **kwargs)
