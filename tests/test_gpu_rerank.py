"""nvsm_rerank on the GPU against its definition: bit for bit what nvsm_rank returns with `candidates` set to the ids the first stage
returns at top_k = depth — for both first stages, both similarities, depths below, at and above the number of matches, queries
without candidates, weighted neural queries, more queries than one chunk holds — and nvsm_evaluate's metrics for those candidates;
the cap NVSM_RERANK_MAX_DEPTH; lazily decayed tables read through their view; every refusal by name."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import tfidf_reference as tr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu

V = tr.NUM_WORDS
TOKENS, OFFSETS = tr.gpu_corpus()
D = OFFSETS.size - 1
QUERIES = tr.gpu_queries(TOKENS)
STAGES = {"tfidf": dict(idf="okapi", k1=0.9, b=0.4), "lexical": dict(method="dirichlet", param=30.0)}


def first_stage(m, stage, queries, depth):
    if stage == "tfidf":
        return m.tfidf_rank(queries, top_k=depth, **STAGES[stage])
    return m.lexical_rank(queries, top_k=depth, **STAGES[stage])


def candidates_of(first):
    ids, _, counts = first
    return [ids[i, :counts[i]] for i in range(ids.shape[0])]


@pytest.fixture(scope="module")
def model():
    return lexical_model(D, num_words=V, corpus=(TOKENS, OFFSETS))


@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("similarity", ["cosine", "dot"])
def test_rerank_is_rank_over_the_first_stage_ids(model, stage, similarity):
    matches = first_stage(model, stage, QUERIES, D)[2]
    assert matches.min() == 0 and 2 in matches and matches.max() == D - 1    # no candidates; depth 2 = the matches; most documents
    for depth, top_k in ((1, 1), (2, 2), (30, 7), (30, 30), (D, 10), (D, D)):
        for Q in (1, 7, 40, len(QUERIES)):                                    # ragged lengths, repeated and absent words among them
            qs = QUERIES[-Q:]
            first = first_stage(model, stage, qs, depth)
            want = model.rank(qs, top_k=top_k, candidates=candidates_of(first), similarity=similarity, bias_coefficient=0.0)
            got = model.rerank(qs, first_stage=stage, depth=depth, top_k=top_k, similarity=similarity, bias_coefficient=0.0, **STAGES[stage])
            same_bits(want, got)
            np.testing.assert_array_equal(got[2], np.minimum(top_k, first[2]))
    same_bits(got, model.rerank(qs, first_stage=stage, depth=depth, top_k=top_k, similarity=similarity, bias_coefficient=0.0, **STAGES[stage]))


def test_the_first_stage_is_unweighted_and_the_weights_shape_the_neural_query(model):
    rs = np.random.RandomState(3)
    weights = [rs.uniform(0.5, 2.0, len(q)).astype(np.float32) for q in QUERIES]
    first = model.tfidf_rank(QUERIES, top_k=20)                               # unweighted, at the defaults
    want = model.rank(QUERIES, top_k=10, weights=weights, candidates=candidates_of(first))
    got = model.rerank(QUERIES, depth=20, top_k=10, weights=weights)
    same_bits(want, got)
    assert (got[1] != model.rerank(QUERIES, depth=20, top_k=10)[1]).any()


def test_metrics_are_evaluates_for_those_candidates(model):
    rs = np.random.RandomState(4)
    judged = [[(int(d), int(rs.randint(0, 3))) for d in rs.choice(D, rs.randint(0, 12), replace=False)] + [(-1, 1)] for _ in QUERIES]
    for stage in sorted(STAGES):
        first = first_stage(model, stage, QUERIES, 25)
        want = model.evaluate(QUERIES, judged, top_k=10, cutoffs=(1, 5, 10), candidates=candidates_of(first), return_ranking=True)
        got = model.rerank(QUERIES, first_stage=stage, depth=25, top_k=10, judgments=judged, cutoffs=(1, 5, 10), **STAGES[stage])
        assert sorted(want[0]) == sorted(got[0])
        for name in want[0]:
            np.testing.assert_array_equal(want[0][name].view(np.int64), got[0][name].view(np.int64), err_msg=name)
        same_bits(want[1:], got[1:])
        assert want[0]["num_rel_ret"].sum() > 0


def test_more_queries_than_a_chunk_and_many_first_stage_rounds(model):
    """4100 queries: two chunks of the hand-over, seventeen first-stage rounds in the first, candidate offsets that run across them"""
    rs = np.random.RandomState(5)
    present = np.flatnonzero(tr.document_frequencies(TOKENS, OFFSETS, V) > 0)
    qs = [list(present[rs.randint(0, present.size, rs.randint(1, 4))]) for _ in range(4100)]
    qs[4095], qs[4096] = [tr.W_ABSENT], [tr.W_ALL]
    first = model.tfidf_rank(qs, top_k=6)
    want = model.rank(qs, top_k=3, candidates=candidates_of(first))
    same_bits(want, model.rerank(qs, depth=6, top_k=3))


def test_the_cap():
    """4100 one-token documents over three words; word 0 is in all but two of them: every depth up to the cap is filled"""
    n = 4100
    tokens = np.zeros(n, np.int32)
    tokens[[17, 4000]] = [1, 2]
    offsets = np.arange(n + 1, dtype=np.int64)
    m = lexical_model(n, num_words=5, corpus=(tokens, offsets))
    cap = ca._lib.RERANK_MAX_DEPTH
    assert cap == 4096
    queries = [[0], [1], [3], [0, 2]]
    for stage in ("tfidf", "lexical"):
        first = m.tfidf_rank(queries, top_k=cap) if stage == "tfidf" else m.lexical_rank(queries, top_k=cap)
        np.testing.assert_array_equal(first[2], [cap, 1, 0, cap])
        want = m.rank(queries, top_k=50, candidates=candidates_of(first))
        same_bits(want, m.rerank(queries, first_stage=stage, depth=cap, top_k=50))
        with pytest.raises(ca.NvsmError) as e:
            m.rerank(queries, first_stage=stage, depth=cap + 1, top_k=50)
        assert e.value.status == 2 and "NVSM_RERANK_MAX_DEPTH" in str(e.value)
        with pytest.raises(ca.NvsmError) as e:                                # past the documents: a wrong argument, whatever the cap
            m.rerank(queries, first_stage=stage, depth=n + 1, top_k=50)
        assert e.value.status == 1 and "depth" in str(e.value)


def test_lazy_tables_are_read_through_their_view(monkeypatch):
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(num_words=V, num_entities=500, word_dim=12, entity_dim=16, window=3, num_random=2, nonlinearity="tanh",
                batch_norm=False, update_method="sparse_adam")
    spec["lambda"] = 0.02
    rs = np.random.RandomState(12)
    params = random_params(spec, rs)
    a, b = gpu_model(spec, 40), gpu_model(spec, 40)
    for m in (a, b):
        load_params(m, params, True)
        m.upload_corpus(ca.Corpus(TOKENS, OFFSETS))
    batches = [random_batch(spec, rs, 40, zipf=True) for _ in range(20)]

    def ten(lo):
        for words, ww, labels, iw, ids in batches[lo:lo + 10]:
            for m in (a, b):
                m.step(ca.Batch(words, labels, ww, iw), 2e-2, entity_ids=ids)
    ten(0)
    got = a.rerank(QUERIES, depth=30, top_k=10)                               # rows that sat out updates carry pending factors
    first = a.tfidf_rank(QUERIES, top_k=30)
    same_bits(a.rank(QUERIES, top_k=10, candidates=candidates_of(first)), got)
    ten(10)                                                                   # ... and nothing was flushed: the twin did nothing there
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.profile_enable(True)
    words, ww, labels, iw, ids = batches[0]
    a.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids)
    assert {"lazy_stamp_words", "lazy_stamp_entities"} <= set(a.profile()), "the handle's tables do decay lazily"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def raw_rerank(m, depth=5, top_k=3, stage=0, similarity=0, tfidf=None, lexical=None, candidates=False, judgments=False, metrics=False,
               words=(1, 2, 3), word_offsets=(0, 2, 3), null=None):
    w, off = np.asarray(words, np.int64), np.asarray(word_offsets, np.int64)
    Q = off.size - 1
    q = ca.NvsmQueries(w.ctypes.data, None, off.ctypes.data, Q)
    ro = ca.NvsmRankOptions()
    ca.lib().nvsm_rank_options_default(C.byref(ro))
    ro.top_k, ro.similarity = top_k, similarity
    cand, cand_off = np.zeros(1, np.int64), np.zeros(Q + 1, np.int64)
    if candidates:
        ro.candidates, ro.candidate_offsets = cand.ctypes.data, cand_off.ctypes.data
    rr = ca.NvsmRerankOptions()
    ca.lib().nvsm_rerank_options_default(C.byref(rr))
    rr.first_stage, rr.depth = stage, depth
    to, lo = ca.NvsmTfidfOptions(), ca.NvsmLexicalOptions()
    ca.lib().nvsm_tfidf_options_default(C.byref(to))
    ca.lib().nvsm_lexical_options_default(C.byref(lo))
    if tfidf:
        for name, value in tfidf.items():
            setattr(to, name, value)
        rr.tfidf = C.pointer(to)
    if lexical:
        for name, value in lexical.items():
            setattr(lo, name, value)
        rr.lexical = C.pointer(lo)
    joff, cut = np.zeros(Q + 1, np.int64), np.array([1], np.int32)
    js = ca.NvsmJudgments(None, None, joff.ctypes.data, cut.ctypes.data, 1)
    met = np.full((Q, 10), -7.0, np.float64)
    ids = np.full((Q, max(top_k, 1)), -7, np.int64)
    scores = np.full((Q, max(top_k, 1)), -7.0, np.float32)
    counts = np.full(Q, -7, np.int64)
    ptr = lambda name, a: None if null == name else a.ctypes.data
    st = ca.lib().nvsm_rerank(m._h, None if null == "queries" else C.byref(q), None if null == "rank_opt" else C.byref(ro),
                              None if null == "rr" else C.byref(rr), C.byref(js) if judgments else None, met.ctypes.data if metrics else None,
                              ptr("doc_ids", ids), ptr("scores", scores), ptr("counts", counts))
    return st, (ids, scores, counts, met)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    m = lexical_model(D, num_words=V)
    L = ca.lib()
    st, _ = raw_rerank(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()          # no corpus uploaded
    m.upload_corpus(ca.Corpus(TOKENS, OFFSETS))
    defaults = ca.NvsmRerankOptions()
    L.nvsm_rerank_options_default(C.byref(defaults))
    assert (defaults.first_stage, defaults.depth, bool(defaults.tfidf), bool(defaults.lexical)) == (ca.STAGE_TFIDF, 1000, False, False)
    nan = float("nan")
    bad = [
        (dict(candidates=True), b"rank_opt->candidates must be NULL"),
        (dict(stage=2), b"unknown first stage"), (dict(stage=-1), b"unknown first stage"),
        (dict(depth=0), b"depth must be in"), (dict(depth=D + 1), b"depth must be in"),
        (dict(depth=2, top_k=3), b"depth must not be smaller than rank_opt->top_k"),
        (dict(tfidf=dict(k1=-1.0)), b"k1"), (dict(tfidf=dict(b=nan)), b"b must"), (dict(tfidf=dict(idf=7)), b"unknown idf"),
        (dict(stage=1, lexical=dict(method=9)), b"unknown lexical method"), (dict(stage=1, lexical=dict(param=1.5)), b"lambda"),
        (dict(similarity=5), b"unknown similarity"), (dict(top_k=0), b"top_k"),
        (dict(word_offsets=(0, 3, 2)), b"queries->offsets decrease"),
        (dict(null="queries"), b"null argument: queries"), (dict(null="rank_opt"), b"null argument: rank_opt"),
        (dict(null="rr"), b"null argument: rr"), (dict(judgments=True), b"null argument: metrics"),
        (dict(metrics=True), b"null argument: judgments"), (dict(null="doc_ids"), b"null argument: doc_ids"),
        (dict(null="scores"), b"null argument: scores"), (dict(null="counts"), b"null argument: counts"),
    ]
    for kwargs, word in bad:
        st, out = raw_rerank(m, **kwargs)
        assert st == 1 and word in L.nvsm_last_error(), (kwargs, L.nvsm_last_error())
        assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_rerank(m)
        assert st == 0 and (out[2] >= 0).all()
    # the stage's own top_k is not looked at, the other stage's options neither; with metrics the lists may stay away
    assert raw_rerank(m, tfidf=dict(top_k=-3), lexical=dict(method=9))[0] == 0
    assert raw_rerank(m, stage=1, lexical=dict(top_k=10 ** 6), tfidf=dict(idf=7))[0] == 0
    st, out = raw_rerank(m, judgments=True, metrics=True, null="doc_ids")
    assert st == 0 and (out[3][:, :8] != -7).all() and (out[0] == -7).all() and (out[2] >= 0).all()
    # a word id out of range follows the index contract
    st, out = raw_rerank(m, words=(1, V, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error()
    with pytest.raises(ValueError):
        m.rerank([[1]], first_stage="bm25")
