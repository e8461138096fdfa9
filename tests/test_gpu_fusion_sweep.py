"""nvsm_ensemble_sweep on the GPU: every row against the row nvsm_rank_ensemble(_prf) returns for that alpha, bit for bit, wherever
the depth does not cut; cut rows against the restatement (tests/fusion_cv_reference.py) of the GPU's own two lists; the strip, round
and LDS boundaries of fuse_sweep_kernel; and what the call must leave alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import eval_reference as er
from tests import lexical_reference as lr
from tests.conftest import ROOT
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_ensemble import CUTOFFS, METRIC_BOUND, NUM_WORDS, REL, ensemble_model, queries_for
from tests.test_gpu_eval import judged_list
from tests.test_gpu_rank import ADAM_STATE

pytestmark = pytest.mark.gpu

ALPHAS = np.array([0.0, 0.25, np.float32(0.3), 0.5, 1.0], np.float32)
NAMES = er.names(CUTOFFS)
with open(os.path.join(ROOT, "cunvsm_amd", "csrc", "kernels.h")) as f:
    _KERNELS_H = f.read()
STRIP = int(re.search(r"constexpr int kFuseSweepStrip = (\d+);", _KERNELS_H).group(1))
RANK_CHUNK = 256                            # ranking.cpp kRankChunk: the queries of one round of fusion

_MODELS = {}


def model(D=300, **kw):
    key = (D, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = ensemble_model(D, **kw)
    return _MODELS[key]


def same_rows(got, want, what=""):
    """two metric dicts of equal shapes, as bits"""
    assert list(got) == list(want) == NAMES
    for name in NAMES:
        np.testing.assert_array_equal(got[name].view(np.uint64), want[name].view(np.uint64), err_msg="%s %s" % (what, name))


def nine_queries(m, tokens, offsets, D, k_max):
    """Q = 9: one query without words, one whose lexical list is empty, one whose two lists share no document at top_k <= k_max"""
    qs = queries_for(tokens, 9, 21)
    cf = lr.collection_frequencies(tokens, NUM_WORDS)
    doc_of = np.repeat(np.arange(D), np.diff(offsets))
    for w in np.flatnonzero((cf >= 1) & (cf <= 2)):
        holders = np.unique(doc_of[tokens == w])
        ids, _, n = m.rank([[int(w)]], top_k=k_max)
        if not np.isin(holders, ids[0, :n[0]]).any():
            qs[5] = [int(w)]
            return qs
    raise AssertionError("no rare word whose documents all lie outside rank()'s list")


def judgments_for(Q, D, seed):
    rs = np.random.RandomState(seed)
    return [judged_list(rs, D, (0, 1, 9, 65)[q % 4]) for q in range(Q)]


def ensemble_rows(m, qs, judged, alphas, **kw):
    """the loop a caller writes without the sweep: rank_ensemble's metrics per alpha, stacked [A, Q]"""
    rows = [m.rank_ensemble(qs, alpha=float(a), judgments=judged, cutoffs=CUTOFFS, **kw)[0] for a in alphas]
    return {name: np.stack([r[name] for r in rows]) for name in NAMES}


@pytest.mark.parametrize("top_k", [1, 5, 64, 150])
@pytest.mark.parametrize("normalizer", ["standardize", "minmax", "none"])
def test_rows_are_rank_ensembles_bits(normalizer, top_k):
    D = 300
    m, tokens, offsets = model(D)
    qs = nine_queries(m, tokens, offsets, D, 150)
    judged = judgments_for(9, D, top_k)
    kw = dict(normalizer=normalizer, top_k=top_k)
    a_ids, _, a_n = m.rank(qs, top_k=top_k)
    b_ids, _, b_n = m.lexical_rank(qs, top_k=top_k)
    assert a_n[1] == b_n[1] == 0 and b_n[2] == 0 and a_n[2] == top_k      # the premises: no words; an empty lexical list;
    assert b_n[5] > 0 and not np.isin(b_ids[5, :b_n[5]], a_ids[5, :a_n[5]]).any()      # ... lists without a common document
    want = ensemble_rows(m, qs, judged, ALPHAS, **kw)
    got = m.ensemble_sweep(qs, judged, ALPHAS, depth=0, cutoffs=CUTOFFS, **kw)
    assert got["map"].shape == (ALPHAS.size, 9) and got["map"].dtype == np.float64
    same_rows(got, want, "depth 0")
    assert all((got[name][:, 1] == 0.0).all() for name in NAMES)             # the query without words: all zeros
    for depth in (2 * top_k, 2 * top_k + 1):
        same_rows(m.ensemble_sweep(qs, judged, ALPHAS, depth=depth, cutoffs=CUTOFFS, **kw), want, "depth %d" % depth)
    want = ensemble_rows(m, qs, judged, ALPHAS, feedback=True, **kw)
    same_rows(m.ensemble_sweep(qs, judged, ALPHAS, feedback=True, cutoffs=CUTOFFS, **kw), want, "feedback")


@pytest.mark.parametrize("depth", [1, 7, 64, 65, 129])
def test_rows_of_a_cut_list_follow_the_restatement(depth):
    D, k = 300, 150
    m, tokens, offsets = model(D)
    qs = nine_queries(m, tokens, offsets, D, k)
    judged = judgments_for(9, D, 77)
    a_ids, a_sc, a_n = m.rank(qs, top_k=k)
    b_ids, b_sc, b_n = m.lexical_rank(qs, top_k=k)
    alphas = ALPHAS[1:4]
    got = m.ensemble_sweep(qs, judged, alphas, depth=depth, top_k=k, cutoffs=CUTOFFS)
    left = total = 0
    for ai, alpha in enumerate(alphas):
        ids, _, counts = m.rank_ensemble(qs, alpha=float(alpha), top_k=k)
        for i in range(9):
            r_ids, r_sc = lr.fuse_query(a_ids[i, :a_n[i]], a_sc[i, :a_n[i]], b_ids[i, :b_n[i]], b_sc[i, :b_n[i]], alpha, "standardize")
            n = r_ids.size
            assert counts[i] == n
            # check_fusion's treatment of the order: where the restatement decides it, it is the restatement's
            open_ = lr.excused(r_sc, REL * np.abs(r_sc)) if n else np.zeros(0, bool)
            differ = ids[i, :n] != r_ids
            assert not (differ & ~open_).any(), (alpha, i)
            left += int(open_.sum())
            total += n
            ref = er.evaluate_query(ids[i, :min(n, depth)], judged[i], CUTOFFS, has_words=len(qs[i]) > 0)
            for name in NAMES:
                value = got[name][ai, i]
                if name in er.INTEGER:
                    assert value == ref[name], (name, alpha, i)
                else:
                    assert abs(value - ref[name]) <= METRIC_BOUND, (name, alpha, i, value, ref[name])
            if len(qs[i]):
                assert got["num_ret"][ai, i] == min(n, depth)
    assert left <= lr.SHARE * total, (left, total)


def test_strip_boundaries():
    D, k = 300, 5
    m, tokens, offsets = model(D)
    qs = nine_queries(m, tokens, offsets, D, 150)
    judged = judgments_for(9, D, 5)
    grid = np.concatenate([ca.alpha_grid(0.01), [1.0]]).astype(np.float32)
    assert grid.size == 101 and STRIP >= 2
    full = m.ensemble_sweep(qs, judged, grid, top_k=k, cutoffs=CUTOFFS)
    at = np.array([0, STRIP - 1, STRIP, 100])
    same_rows({n: v[at] for n, v in full.items()}, ensemble_rows(m, qs, judged, grid[at], top_k=k), "101 alphas")
    for count in (1, STRIP, STRIP + 1):
        part = m.ensemble_sweep(qs, judged, grid[:count], top_k=k, cutoffs=CUTOFFS)
        same_rows(part, {n: v[:count] for n, v in full.items()}, "%d alphas" % count)


def test_a_round_boundary():
    D, k, Q = 300, 5, RANK_CHUNK + 3
    m, tokens, offsets = model(D)
    qs = queries_for(tokens, Q, 9)
    judged = judgments_for(Q, D, 6)
    alphas = np.array([0.75, 0.125], np.float32)
    same_rows(m.ensemble_sweep(qs, judged, alphas, top_k=k, cutoffs=CUTOFFS), ensemble_rows(m, qs, judged, alphas, top_k=k), "two rounds")


def test_the_largest_list():
    D, k = 2000, 1000
    m, tokens, offsets = model(D, seed=2)
    qs = queries_for(tokens, 3, 11) + [[int(t) for t in tokens[:40]]]     # the last one matches most documents: 1000 + 1000 entries
    rs = np.random.RandomState(4)
    judged = [judged_list(rs, D, 65) for _ in qs]
    alphas = np.array([0.0, 0.5, np.float32(0.7)], np.float32)
    want = ensemble_rows(m, qs, judged, alphas, top_k=k)
    assert want["num_ret"][0, -1] > 1000
    same_rows(m.ensemble_sweep(qs, judged, alphas, top_k=k, cutoffs=CUTOFFS), want, "top_k 1000")
    same_rows(m.ensemble_sweep(qs, judged, alphas, top_k=k, depth=2 * k, cutoffs=CUTOFFS), want, "top_k 1000, depth 2000")


@pytest.mark.parametrize("normalizer", ["standardize", "minmax"])
def test_a_constant_list_normalises_to_zero(normalizer):
    D, k = 200, 10
    m, tokens, offsets = model(D, seed=1, constant_documents=True)
    qs = queries_for(tokens, 12, 3)
    judged = judgments_for(12, D, 8)
    a_ids, a_sc, a_n = m.rank(qs, top_k=k)
    assert all(np.unique(a_sc[i, :a_n[i]]).size == 1 for i in range(12) if a_n[i])       # the premise: list A is one constant per query
    assert m.lexical_rank(qs, top_k=k)[2][2] == 0                         # ... and query 2 has list A alone
    alphas = np.array([0.0, 0.2, 0.9, 1.0], np.float32)
    got = m.ensemble_sweep(qs, judged, alphas, normalizer=normalizer, top_k=k, cutoffs=CUTOFFS)
    same_rows(got, ensemble_rows(m, qs, judged, alphas, normalizer=normalizer, top_k=k), "constant list A")
    for name in NAMES:                      # every fused score of query 2 is alpha·0: the order is the ids', whatever alpha
        assert (got[name][:, 2].view(np.uint64) == got[name][0, 2].view(np.uint64)).all(), name


def test_repeated_and_unordered_alphas_and_repeated_calls():
    D, k = 300, 64
    m, tokens, offsets = model(D)
    qs = nine_queries(m, tokens, offsets, D, 150)
    judged = judgments_for(9, D, 12)
    alphas = np.array([0.5, 0.0, 1.0, 0.5, 0.25, 0.0, 0.5, 1.0, 0.25, 0.5], np.float32)      # a second strip begins inside the repeats
    got = m.ensemble_sweep(qs, judged, alphas, top_k=k, depth=65, cutoffs=CUTOFFS)
    for name in NAMES:
        for value in np.unique(alphas):
            rows = got[name][alphas == value].view(np.uint64)
            assert (rows == rows[0]).all(), (name, value)
    ordered = m.ensemble_sweep(qs, judged, np.unique(alphas), top_k=k, depth=65, cutoffs=CUTOFFS)
    same_rows({n: v[[1, 4, 0, 2]] for n, v in got.items()}, ordered, "order")      # the rows of 0, 0.25, 0.5 and 1
    same_rows(m.ensemble_sweep(qs, judged, alphas, top_k=k, depth=65, cutoffs=CUTOFFS), got, "a second call")


def test_a_sweep_between_steps_never_disturbs_training():
    spec = dict(num_words=2000, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    tokens, offsets = lr.zipf_corpus(3, 600, 2000)
    queries = lr.zipf_queries(4, 20, 2000, tokens)
    judged = judgments_for(20, 600, 2)
    models = []
    for _ in range(2):
        m = gpu_model(spec, 64)
        load_params(m, random_params(spec, np.random.RandomState(9)), True)
        m.upload_corpus(ca.Corpus(tokens, offsets))
        models.append(m)
    a, b = models
    rs = np.random.RandomState(10)
    for words, ww, labels, iw, ids in [random_batch(spec, rs, 64, zipf=True) for _ in range(3)]:
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        a.ensemble_sweep(queries, judged, ALPHAS, top_k=50)                 # straight behind nvsm_step
        a.rank_ensemble_cv(queries, judged, stepsize=0.25, num_folds=4, top_k=50, feedback=True)
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    assert a.describe() == b.describe()                     # what the calls allocated is not in the text


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_sweep(m, top_k=5, lex_top_k=None, alphas=(0.5, 0.25), num_alphas=None, null_alphas=False, normalizer=0, depth=0, method=0,
              param=0.0, candidates=False, similarity=0, cv=None, fb_docs=None):
    """nvsm_ensemble_sweep, or with cv = dict(measure, num_folds, fold_of) nvsm_rank_ensemble_cv, on three two-word queries"""
    words, off = np.asarray([1, 2, 3, 4, 5, 6], np.int64), np.asarray([0, 2, 4, 6], np.int64)
    q = ca.NvsmQueries(words.ctypes.data, None, off.ctypes.data, 3)
    ro, lo, so, fo = ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmSweepOptions(), ca.NvsmFeedbackOptions()
    L = ca.lib()
    L.nvsm_rank_options_default(C.byref(ro))
    L.nvsm_lexical_options_default(C.byref(lo))
    L.nvsm_sweep_options_default(C.byref(so))
    L.nvsm_feedback_options_default(C.byref(fo))
    ro.top_k, ro.similarity = top_k, similarity
    lo.top_k, lo.method, lo.param = top_k if lex_top_k is None else lex_top_k, method, param
    grid = np.asarray(alphas, np.float32)
    so.alphas = None if null_alphas else grid.ctypes.data
    so.num_alphas, so.normalizer, so.depth = grid.size if num_alphas is None else num_alphas, normalizer, depth
    cand, coff = np.asarray([0, 1, 2], np.int64), np.asarray([0, 1, 2, 3], np.int64)
    if candidates:
        ro.candidates, ro.candidate_offsets = cand.ctypes.data, coff.ctypes.data
    fb = None
    if fb_docs is not None:
        fo.fb_docs = fb_docs
        fb = C.byref(fo)
    jd, jg, jo = np.asarray([0, 3], np.int64), np.asarray([1, 2], np.int32), np.asarray([0, 1, 2, 2], np.int64)
    j = ca.NvsmJudgments(jd.ctypes.data, jg.ctypes.data, jo.ctypes.data, None, 0)
    table = np.full((max(grid.size, 1), 3, 7), -7.0, np.float64)
    if cv is None:
        st = L.nvsm_ensemble_sweep(m._h, C.byref(q), C.byref(ro), C.byref(lo), fb, C.byref(so), C.byref(j), table.ctypes.data)
        return st, (table,)
    co = ca.NvsmCvOptions()
    L.nvsm_cv_options_default(C.byref(co))
    co.measure, co.num_folds = cv.get("measure", 3), cv.get("num_folds", 3)
    folds = np.asarray(cv["fold_of"], np.int32) if "fold_of" in cv else None
    if folds is not None:
        co.fold_of = folds.ctypes.data
    F = max(co.num_folds, 1)
    width = 2 * max(top_k, 1)
    out = (np.full(F, -7.0, np.float32), np.full(F, -7.0, np.float64), np.full((3, width), -7, np.int64), np.full((3, width), -7.0, np.float32),
           np.full(3, -7, np.int64), np.full((3, 7), -7.0, np.float64), table)
    st = L.nvsm_rank_ensemble_cv(m._h, C.byref(q), C.byref(ro), C.byref(lo), fb, C.byref(so), C.byref(co), C.byref(j),
                                 *[x.ctypes.data for x in out])
    return st, out


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    D = 1100
    m, tokens, offsets = model(D, seed=5)
    L = ca.lib()
    bad = [
        (dict(normalizer=3), 1, b"normalizer"), (dict(alphas=(0.5, 1.5)), 1, b"alpha"), (dict(alphas=(-0.01,)), 1, b"alpha"),
        (dict(alphas=(0.5, float("nan"))), 1, b"alpha"), (dict(alphas=(float("inf"),)), 1, b"alpha"),
        (dict(null_alphas=True), 1, b"null argument: sweep->alphas"), (dict(num_alphas=0), 1, b"num_alphas"),
        (dict(num_alphas=1025), 1, b"num_alphas"), (dict(depth=-1), 1, b"depth"),
        (dict(method=7), 1, b"method"), (dict(param=1.0), 1, b"lambda"), (dict(method=1, param=-2.0), 1, b"mu"),
        (dict(top_k=0), 1, b"top_k"), (dict(top_k=D + 1), 1, b"top_k"), (dict(lex_top_k=4), 1, b"equal"),
        (dict(candidates=True), 1, b"candidates"), (dict(similarity=9), 1, b"similarity"), (dict(fb_docs=0), 1, b"fb_docs"),
        (dict(top_k=1025), 2, b"NVSM_ENSEMBLE_MAX_TOP_K"),
        (dict(cv=dict(num_folds=1)), 1, b"num_folds"), (dict(cv=dict(num_folds=4)), 1, b"num_folds"),
        (dict(cv=dict(fold_of=[0, 3, 1])), 1, b"fold_of"), (dict(cv=dict(fold_of=[0, -1, 1])), 1, b"fold_of"),
        (dict(cv=dict(fold_of=[1, 1, 1])), 1, b"training set"),
        (dict(cv=dict(measure=7)), 1, b"measure"), (dict(cv=dict(measure=-1)), 1, b"measure"),
        (dict(cv=dict(measure=0)), 1, b"measure"), (dict(cv=dict(measure=1)), 1, b"measure"), (dict(cv=dict(measure=2)), 1, b"measure"),
        (dict(cv=dict(), depth=-2), 1, b"depth"), (dict(cv=dict(), alphas=(2.0,)), 1, b"alpha"),
    ]
    for kwargs, status, word in bad:
        st, out = raw_sweep(m, **kwargs)
        assert st == status and word in L.nvsm_last_error(), (kwargs, st, L.nvsm_last_error())
        assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_sweep(m)
        assert st == 0 and (out[0][:, :, 0] >= 5).all()                   # num_ret of every row
    assert raw_sweep(m, top_k=1024)[0] == 0                               # the limit itself is served
    st, out = raw_sweep(m, cv=dict(fold_of=[0, 2, 2]))                    # an empty fold is served: (NaN, 0)
    assert st == 0 and np.isnan(out[0][1]) and out[1][1] == 0.0 and not np.isnan(out[0][[0, 2]]).any()
    m.upload_corpus(None)
    st, out = raw_sweep(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error() and all((a == -7).all() for a in out)
    del _MODELS[(D, (("seed", 5),))]                                      # (the cached model has lost its corpus)
    for call in (lambda: m.ensemble_sweep([[1]], [[(0, 1)]], [2.0]), lambda: m.ensemble_sweep([[1]], [[(0, 1)]], []),
                 lambda: m.ensemble_sweep([[1]], [[(0, 1)]], [0.5], depth=-1), lambda: m.ensemble_sweep([[1]], None, [0.5]),
                 lambda: m.ensemble_sweep([[1]], [[(0, 1)]], [0.5], normalizer="zscore"),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=3),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=2, measure="num_ret"),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=2, measure="bpref"),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=2, fold_of=[0, 2]),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=2, fold_of=[1, 1]),
                 lambda: m.rank_ensemble_cv([[1], [2]], [[(0, 1)], []], num_folds=2, stepsize=0.0005)):
        with pytest.raises(ValueError):
            call()
