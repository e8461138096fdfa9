"""-m gpu: query inference and top-k document ranking (nvsm_infer / nvsm_rank, csrc/rank.hip) against fp64 numpy.

The reference values are fp64 restatements, written here, of the formulas the header pins (include/cunvsm_amd.h):
  representation  Σ wᵢ·W[idᵢ] / Σ wᵢ                         (np.average, py/nvsm/base.py:305-307)
  projection      f(T·x + c·b), no batch normalisation        (cpp/model.cu:105-133)
  score           cosine similarity (inverse norm 0 for a zero vector) or the dot product
  ranking         top k by score descending, ties by ascending document id

RANK CORRECTNESS RULE (rule 2 of the issue). s64 = the fp64 scores, err32 = the largest |s32 − s64| of a float32 numpy
evaluation of the same formula on the same inputs, tol = 4·err32 (the factor allows for another summation order over the
d_e terms and for norms accumulated beside the dot products). A result is correct when per query (a) every returned score
is within tol of s64 of the returned id; (b) every document with s64 > s64_k + 2·tol is returned and none with
s64 < s64_k − 2·tol (s64_k: the k-th largest); (c) returned scores do not increase, equal scores come in ascending id order,
ids are distinct; (d) along the returned order s64 never rises by more than 2·tol. The band |s64 − s64_k| ≤ 2·tol may hold
at most max(2, k/100) documents besides the k-th: asserted about the inputs BEFORE the GPU result is looked at.

In the shape sweep the projection is made exact in every arithmetic (one word per query, d_w = d_e, T = I, c = 0, identity
activation: the projected query IS the word row, bit for bit), so that the scoring formula's inputs are known to the test
and err32 is the error of the scoring formula alone — the figures the issue quotes for these two kinds of input. The tests
of lazily decayed tables, candidates and training in between run the whole chain (multi-word queries, a trained T, tanh)
in fp64 and in float32, parameters as nvsm_get_param returns them.

Every case prints `rank-error` lines: err32 and the observed max|s − s64| / err32 (DESIGN.md §9 quotes them)."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params, rel_err

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS


# ---- fp64 / float32 restatements ---------------------------------------------------------------------------------------------
def ref_infer(params, spec, queries, weights=None, c=1.0, act="tanh", dtype=np.float64):
    dw, de = spec["word_dim"], spec["entity_dim"]
    W = params[W_NAME].reshape(-1, dw).astype(dtype)
    T = params[T_NAME].reshape(dw, de).astype(dtype)          # stored T[r + de·c]: [c][r]
    b = params[B_NAME].astype(dtype)
    X = np.zeros((len(queries), dw), dtype)
    for i, q in enumerate(queries):
        rows = W[np.asarray(q, np.int64)]
        w = np.ones(len(q), dtype) if weights is None else np.asarray(weights[i], dtype)
        X[i] = (w[:, None] * rows).sum(0, dtype=dtype) / w.sum(dtype=dtype)
    pre = X @ T + dtype(c) * b
    if act == "tanh":
        return np.tanh(pre)
    if act == "hard_tanh":
        return np.clip(pre, -1, 1)
    return pre


def ref_scores(P, E, sim, dtype=np.float64, chunk=100000):
    """[Q][D] scores of the projected queries P against the rows of E, everything in `dtype`."""
    P = P.astype(dtype)
    out = np.empty((P.shape[0], E.shape[0]), dtype)
    if sim == "cosine":
        pn = np.sqrt((P * P).sum(1, dtype=dtype))
        pinv = np.where(pn > 0, dtype(1) / np.where(pn > 0, pn, 1), dtype(0)).astype(dtype)
    for d0 in range(0, E.shape[0], chunk):
        Ec = E[d0:d0 + chunk].astype(dtype)
        s = P @ Ec.T
        if sim == "cosine":
            en = np.sqrt((Ec * Ec).sum(1, dtype=dtype))
            einv = np.where(en > 0, dtype(1) / np.where(en > 0, en, 1), dtype(0)).astype(dtype)
            s = s * einv[None, :] * pinv[:, None]
        out[:, d0:d0 + chunk] = s
    return out


def tolerance(P, E, sim):
    s64 = ref_scores(P, E, sim, np.float64)
    s32 = ref_scores(P, E, sim, np.float32)
    err32 = float(np.abs(s32.astype(np.float64) - s64).max())
    return s64, err32, 4.0 * max(err32, 1e-45)


def band_is_narrow(s64q, universe, k, tol):
    su = s64q[universe]
    n = min(k, su.size)
    kth = np.partition(su, su.size - n)[su.size - n]
    others = int((np.abs(su - kth) <= 2 * tol).sum()) - 1
    assert others <= max(2, k / 100), "the test's own inputs: %d documents within 2 tol of the k-th score" % others
    return kth


def check_query(ids, scores, count, s64q, k, tol, universe=None):
    """rule 2 (a)-(d) for one query; returns the largest |s − s64| over the returned documents"""
    D = s64q.size
    universe = np.arange(D) if universe is None else np.unique(np.asarray(universe, np.int64))
    n = min(k, universe.size)
    assert count == n, (count, n)
    assert (ids[n:] == -1).all() and np.isneginf(scores[n:]).all(), "padding is (-1, -inf)"
    if n == 0:
        return 0.0
    kth = band_is_narrow(s64q, universe, k, tol)
    got, sc = ids[:n], scores[:n]
    assert np.isin(got, universe).all()
    assert np.unique(got).size == n, "(c) ids distinct"
    err = float(np.abs(sc.astype(np.float64) - s64q[got]).max())
    assert err <= tol, "(a) score error %g > tol %g" % (err, tol)
    d = np.diff(sc)
    assert (d <= 0).all(), "(c) scores increase"
    assert (np.diff(got)[d == 0] > 0).all(), "(c) equal scores not in ascending id order"
    su = s64q[universe]
    must = universe[su > kth + 2 * tol]
    assert np.isin(must, got).all(), "(b) a document above the band is missing"
    assert (s64q[got] >= kth - 2 * tol).all(), "(b) a document below the band was returned"
    assert (np.diff(s64q[got]) <= 2 * tol).all(), "(d) fp64 scores rise along the returned order"
    return err


def check_result(res, s64, k, tol, universes=None):
    ids, scores, counts = res
    worst = 0.0
    for q in range(s64.shape[0]):
        worst = max(worst, check_query(ids[q], scores[q], counts[q], s64[q], k, tol, None if universes is None else universes[q]))
    return worst


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_rows(kind, rs, D, de, Q):
    """documents [D][de] and queries [Q][de], float32: uniform rows, or 64 Gaussian clusters with the queries near documents"""
    if kind == "uniform":
        E = rs.random_sample((D, de)).astype(np.float32)
        P = rs.random_sample((Q, de)).astype(np.float32)
    else:
        centres = rs.standard_normal((64, de))
        E = (centres[rs.randint(0, 64, D)] + 0.3 * rs.standard_normal((D, de))).astype(np.float32)
        P = (E[rs.randint(0, D, Q)] + 0.1 * rs.standard_normal((Q, de))).astype(np.float32)
    return E, P


def exact_projection_model(E, P, **extra):
    """a handle whose projected query q is P[q] bit for bit: one word per query, d_w = d_e, T = I, c = 0, identity activation"""
    D, de = E.shape
    spec = dict(num_words=P.shape[0], num_entities=D, word_dim=de, entity_dim=de, window=1, num_random=1, update_method="sgd")
    m = gpu_model(spec, 8, **extra)
    m.set_param(W_NAME, P)
    m.set_param(E_NAME, E)
    m.set_param(T_NAME, np.eye(de, dtype=np.float32))
    m.set_param(B_NAME, np.zeros(de, np.float32))
    return m


EXACT = dict(bias_coefficient=0.0, activation="identity")


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same_bits(r1, r2):
    for x, y in zip(r1, r2):
        np.testing.assert_array_equal(bits(x), bits(y))


# ---- 1. infer parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonlin,bn", [("tanh", False), ("hard_tanh", True)])
@pytest.mark.parametrize("dw,de", [(300, 256), (8, 8), (100, 36), (64, 1024)])
def test_infer_matches_fp64(dw, de, nonlin, bn):
    spec = dict(num_words=2000, num_entities=50, word_dim=dw, entity_dim=de, window=5, num_random=2, nonlinearity=nonlin,
                batch_norm=bn, update_method="sgd")
    rs = np.random.RandomState(dw * 7 + de)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 4).astype(np.float32)         # some units leave hard_tanh's linear region
    m = gpu_model(spec, 64)
    load_params(m, params, True)
    other = "hard_tanh" if nonlin == "tanh" else "tanh"
    for Q in (1, 7, 300, 5000):
        lengths = rs.randint(1, 41, Q)
        lengths[:min(Q, 3)] = (1, 40, 17)[:min(Q, 3)]
        queries = [rs.randint(0, spec["num_words"], n) for n in lengths]
        weights = [rs.uniform(0.1, 3.0, n).astype(np.float32) for n in lengths]
        for c, act, wts in ((1.0, "model", None), (0.0, "model", weights), (0.5, "identity", weights), (0.5, other, None),
                            (1.0, nonlin, weights)):
            got = m.infer(queries, wts, bias_coefficient=c, activation=act)
            assert got.shape == (Q, de) and got.dtype == np.float32
            ref = ref_infer(params, spec, queries, wts, c, nonlin if act == "model" else act)
            assert rel_err(got, ref) < 2e-5, (Q, c, act, wts is not None, rel_err(got, ref))
    clipped = np.abs(ref_infer(params, spec, queries, None, 1.0, "identity")) > 1
    assert 0.005 < clipped.mean() < 0.995


@pytest.mark.parametrize("nonlin", ["tanh", "hard_tanh"])
def test_infer_equals_the_forward_projection_of_a_handle_without_batch_norm(nonlin):
    """lengths = window, c = 1, the handle's nonlinearity: Model::infer is compute_cost's "proj" when nothing normalises"""
    spec = dict(num_words=3000, num_entities=400, word_dim=300, entity_dim=256, window=10, num_random=4, nonlinearity=nonlin,
                batch_norm=False, update_method="sgd")
    rs = np.random.RandomState(11)
    params = random_params(spec, rs)
    params[T_NAME] = (params[T_NAME] * 30).astype(np.float32)
    B = 777
    m = gpu_model(spec, B)
    load_params(m, params, True)
    words, _, labels, iw, ids = random_batch(spec, rs, B, weighted=False)
    m.compute_cost(ca.Batch(words, labels, None, iw), ids)
    proj = m.get_tensor("proj").reshape(B, 256)
    got = m.infer(list(words.reshape(B, 10)))
    assert rel_err(got, proj) < 2e-5, rel_err(got, proj)
    assert rel_err(got, ref_infer(params, spec, list(words.reshape(B, 10)), None, 1.0, nonlin)) < 2e-5


# ---- 2, 3. the rule over shapes and dispatch paths ------------------------------------------------------------------------------
#         D       de    Q    k       similarity  rows         slab MB (None: the default 256)
CASES = [(1,      256,  1,   1,      "cosine",   "uniform",   None),
         (37,     36,   5,   10,     "dot",      "uniform",   None),
         (37,     256,  5,   37,     "cosine",   "clustered", None),
         (1000,   256,  64,  10,     "cosine",   "uniform",   None),
         (1000,   36,   300, 1000,   "cosine",   "clustered", None),
         (1000,   1024, 5,   10,     "dot",      "uniform",   None),
         (20000,  1024, 64,  1000,   "cosine",   "clustered", None),
         (20000,  36,   5,   20000,  "dot",      "clustered", None),
         (200000, 256,  64,  1000,   "cosine",   "uniform",   None),
         (200000, 256,  64,  10,     "cosine",   "clustered", None),
         (200000, 256,  300, 1000,   "dot",      "clustered", None),
         (200000, 256,  1,   200000, "cosine",   "uniform",   None),
         (200000, 256,  64,  1000,   "cosine",   "clustered", 1),
         (200000, 256,  5,   10,     "dot",      "uniform",   1),
         (200000, 36,   5,   1,      "cosine",   "uniform",   None)]


def expected_paths(D, de, Q, k, slab_mb, candidates=False):
    """what ranking.cpp's dispatch takes for a shape (the rank_ profile names)"""
    if candidates:
        return {"rank_scan_candidates"}
    qn = min(Q, 256)
    S = min(D, max(4096, ((slab_mb or 256) << 18) // qn // 4096 * 4096))
    slabs = [min(S, D - d0) for d0 in range(0, D, S)]
    n = sum(min(k, s) for s in slabs)
    names = {"rank_scan_mfma" if de % 64 == 0 else "rank_scan_plain"}
    names |= {"rank_select_radix" if k < s else "rank_select_all" for s in slabs}
    names.add("rank_sort_global" if n > 8192 else "rank_sort_lds")
    return names


VISITED = set()


@pytest.mark.parametrize("D,de,Q,k,sim,kind,slab_mb", CASES)
def test_rank_rule(D, de, Q, k, sim, kind, slab_mb, monkeypatch):
    if slab_mb:
        monkeypatch.setenv("NVSM_RANK_SLAB_MB", str(slab_mb))
    rs = np.random.RandomState(D % 1000 + de + Q + k % 997)
    E, P = make_rows(kind, rs, D, de, Q)
    s64, err32, tol = tolerance(P, E, sim)
    for q in range(Q):
        band_is_narrow(s64[q], np.arange(D), k, tol)
    m = exact_projection_model(E, P)
    np.testing.assert_array_equal(m.infer([[q] for q in range(Q)], **EXACT), P)      # the scan's inputs are the test's
    m.profile_enable(True)
    res = m.rank([[q] for q in range(Q)], top_k=k, similarity=sim, **EXACT)
    names = {n for n in m.profile() if n.startswith("rank_")}
    worst = check_result(res, s64, k, tol)
    print("rank-error D=%d de=%d Q=%d k=%d %s %s slab=%s: err32 %.3g, max|s-s64|/err32 %.2f (of the returned documents)"
          % (D, de, Q, k, sim, kind, slab_mb, err32, worst / max(err32, 1e-45)))
    assert expected_paths(D, de, Q, k, slab_mb) <= names, names
    VISITED.update(names)


def test_every_dispatch_path_was_taken():
    """the cases above visit every scan, selection and sort route (candidates: their own test below)"""
    want = set()
    for D, de, Q, k, sim, kind, slab_mb in CASES:
        want |= expected_paths(D, de, Q, k, slab_mb)
    assert want == {"rank_scan_mfma", "rank_scan_plain", "rank_select_radix", "rank_select_all", "rank_sort_lds", "rank_sort_global"}
    if VISITED:                                                    # (empty when this test is selected on its own)
        assert want <= VISITED, want - VISITED


def test_profile_names_appear_only_after_a_rank_call():
    rs = np.random.RandomState(5)
    E, P = make_rows("uniform", rs, 300, 64, 3)
    m = exact_projection_model(E, P)
    m.profile_enable(True)
    m.synchronize()
    assert not any(n.startswith("rank_") for n in m.profile())
    m.infer([[0]])
    assert {n for n in m.profile() if n.startswith("rank_")} == {"rank_query", "rank_infer"}


# ---- full size -------------------------------------------------------------------------------------------------------------------
FULL_D, FULL_DE = 2_000_000, 256


@pytest.fixture(scope="module")
def full_size():
    """an SGD handle (no optimiser state beside the 2 GB documents table) at |D| = 2 M, d_e = 256, with 256 one-word queries"""
    rng = np.random.default_rng(77)
    E = rng.random((FULL_D, FULL_DE), dtype=np.float32)
    P = rng.random((256, FULL_DE), dtype=np.float32)
    m = exact_projection_model(E, P)
    yield m, E, P
    m.close()


def test_memory_growth_at_full_size_stays_under_1_gib(full_size):
    """|D| = 2 M, Q = 256, k = 1000: the score matrix alone would take 2 GB; the call may grow device memory by < 1 GiB"""
    import torch
    m, E, P = full_size
    m.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ids, scores, counts = m.rank([[q] for q in range(256)], top_k=1000, **EXACT)
    free1, _ = torch.cuda.mem_get_info()
    print("rank-memory: device memory in use grew by %.1f MiB" % ((free0 - free1) / 2**20))
    assert (counts == 1000).all() and (ids >= 0).all() and np.isfinite(scores).all()
    assert free0 - free1 < 2**30, (free0 - free1) / 2**20


def test_rank_rule_at_full_size(full_size):
    m, E, P = full_size
    Q, k = 16, 1000
    s64, err32, tol = tolerance(P[:Q], E, "cosine")                # (document chunks of 100 000 rows on the host)
    res = m.rank([[q] for q in range(Q)], top_k=k, **EXACT)
    worst = check_result(res, s64, k, tol)
    print("rank-error D=%d de=%d Q=%d k=%d cosine uniform: err32 %.3g, max|s-s64|/err32 %.2f" % (FULL_D, FULL_DE, Q, k, err32, worst / err32))


# ---- 4. ties and degenerate rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("de,slab_mb", [(256, None), (36, None), (64, 1)])
def test_ties_zero_rows_and_the_zero_query(de, slab_mb, monkeypatch):
    if slab_mb:
        monkeypatch.setenv("NVSM_RANK_SLAB_MB", str(slab_mb))
    rs = np.random.RandomState(de)
    D = 9000
    distinct = rs.standard_normal((50, de)).astype(np.float32)
    E = rs.standard_normal((D, de)).astype(np.float32)
    copies = rs.choice(D, 5200, replace=False)
    E[copies[:5000]] = distinct[rs.randint(0, 50, 5000)]
    E[copies[5000:]] = 0.0
    nq = 64 if slab_mb else 4                                # (64 queries x 1 MB: slabs of 4 096 documents, three of them)
    P = (distinct[np.arange(nq) % 50] + 0.05 * rs.standard_normal((nq, de))).astype(np.float32)
    groups = [np.flatnonzero((E == distinct[j]).all(1)) for j in range(50)]
    assert sum(g.size for g in groups) == 5000
    spec = dict(num_words=nq, num_entities=D, word_dim=de, entity_dim=de, window=1, num_random=1, nonlinearity="hard_tanh",
                update_method="sgd")
    m = gpu_model(spec, 8)
    for name, v in ((W_NAME, P), (E_NAME, E), (T_NAME, np.eye(de, dtype=np.float32)), (B_NAME, np.full(de, 0.25, np.float32))):
        m.set_param(name, v)
    queries = [[q] for q in range(nq)]
    for sim in ("cosine", "dot"):
        ids, sc, cnt = m.rank(queries, top_k=D, similarity=sim, **EXACT)
        s64, s32 = ref_scores(P, E, sim), ref_scores(P, E, sim, np.float32)
        assert (cnt == D).all() and not np.isnan(sc).any()
        for q in range(nq):
            assert np.array_equal(np.sort(ids[q]), np.arange(D))
            by_id = np.empty(D, np.float32)
            by_id[ids[q]] = sc[q]
            assert (by_id[copies[5000:]] == 0).all() and not np.signbit(by_id[copies[5000:]]).any(), "zero rows score exactly +0"
            for rows in groups:                                      # copies of a row: one score, bit for bit
                assert np.unique(by_id[rows].view(np.uint32)).size == 1
            d = np.diff(sc[q])
            assert (d <= 0).all() and (np.diff(ids[q])[d == 0] > 0).all(), "equal scores in ascending id order"
            assert np.abs(by_id.astype(np.float64) - s64[q]).max() <= 4 * np.abs(s32.astype(np.float64) - s64).max()
        # a smaller k is a prefix of the full order, wherever it cuts a group of equal scores
        for k in (1, 7, 100, 1000, 5203):
            ids_k, sc_k, cnt_k = m.rank(queries, top_k=k, similarity=sim, **EXACT)
            assert (cnt_k == k).all()
            np.testing.assert_array_equal(ids_k, ids[:, :k])
            np.testing.assert_array_equal(sc_k.view(np.uint32), sc[:, :k].view(np.uint32))
    # T = 0, c = 0 on a hard-tanh handle: every projected query is exactly 0 — all scores 0, so the ids are 0 .. k − 1
    m.set_param(T_NAME, np.zeros(de * de, np.float32))
    assert not m.infer(queries, bias_coefficient=0.0).any()
    for sim in ("cosine", "dot"):
        for k in (1, 10, 1000, D):
            ids, sc, cnt = m.rank(queries, top_k=k, similarity=sim, bias_coefficient=0.0)
            assert (cnt == k).all() and (sc == 0).all() and not np.signbit(sc).any()
            np.testing.assert_array_equal(ids, np.tile(np.arange(k), (nq, 1)))


# ---- 5. candidates -------------------------------------------------------------------------------------------------------------------
def trained_like_model(rs, de=256, dw=300, D=6000, nonlin="tanh", **extra):
    spec = dict(num_words=2000, num_entities=D, word_dim=dw, entity_dim=de, window=4, num_random=3, nonlinearity=nonlin,
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    m = gpu_model(spec, 64, **extra)
    load_params(m, params, True)
    return spec, params, m


def chain_tolerance(params, spec, queries, weights, sim, c=1.0, act="tanh"):
    """s64 and tol = 4·err32 of the WHOLE chain (mean, projection, activation, score) in fp64 and in float32"""
    E = params[E_NAME].reshape(-1, spec["entity_dim"])
    s64 = ref_scores(ref_infer(params, spec, queries, weights, c, act, np.float64), E, sim, np.float64)
    s32 = ref_scores(ref_infer(params, spec, queries, weights, c, act, np.float32), E, sim, np.float32)
    err32 = float(np.abs(s32.astype(np.float64) - s64).max())
    return s64, err32, 4 * err32


@pytest.mark.parametrize("de", [256, 36])
def test_candidate_lists(de):
    rs = np.random.RandomState(31 + de)
    spec, params, m = trained_like_model(rs, de=de)
    D = spec["num_entities"]
    lengths = [0, 1, 1000, 1000, 5, 3000]
    queries = [rs.randint(0, 2000, rs.randint(1, 9)) for _ in lengths]
    weights = [rs.uniform(0.5, 2, len(q)).astype(np.float32) for q in queries]
    cands = [rs.randint(0, D, n) for n in lengths]                      # unsorted, with duplicates
    cands[3] = np.concatenate([cands[3][:500], cands[3][:500]])         # ... half of them twice
    m.profile_enable(True)
    for sim in ("cosine", "dot"):
        s64, err32, tol = chain_tolerance(params, spec, queries, weights, sim)
        for k in (1, 10, 1000):
            res = m.rank(queries, top_k=k, weights=weights, candidates=cands, similarity=sim)
            worst = check_result(res, s64, k, tol, universes=cands)
            assert list(res[2]) == [min(k, np.unique(c).size) for c in cands]
        print("rank-error candidates de=%d %s: err32 %.3g, max|s-s64|/err32 %.2f" % (de, sim, err32, worst / err32))
    assert "rank_scan_candidates" in m.profile()
    with pytest.raises(ValueError):
        m.rank(queries, top_k=10, candidates=cands[:-1])
    with pytest.raises(ValueError):
        m.rank(queries, top_k=10, candidates=[[D]] * len(queries))


def test_a_query_without_words_retrieves_nothing():
    rs = np.random.RandomState(8)
    spec, params, m = trained_like_model(rs, de=64, dw=16, D=500)
    ids, sc, cnt = m.rank([[3, 4], [], [7]], top_k=5)
    assert list(cnt) == [5, 0, 5] and (ids[1] == -1).all() and np.isneginf(sc[1]).all()
    s64, err32, tol = chain_tolerance(params, spec, [[3, 4], [7]], None, "cosine")
    check_result((ids[[0, 2]], sc[[0, 2]], cnt[[0, 2]]), s64, 5, tol)


# ---- 6. reproducibility and isolation --------------------------------------------------------------------------------------------
ADAM_STATE = ["word_representations/m", "word_representations/v", "entity_representations/m", "entity_representations/v"]


def test_same_call_same_bits_on_two_handles():
    rs = np.random.RandomState(3)
    spec, params, a = trained_like_model(rs)
    _, _, b = trained_like_model(np.random.RandomState(3))
    queries = [rs.randint(0, 2000, rs.randint(1, 30)) for _ in range(70)]
    r1 = a.rank(queries, top_k=100)
    r2 = a.rank(queries, top_k=100)
    r3 = b.rank(queries, top_k=100)
    same_bits(r1, r2)
    same_bits(r1, r3)


def test_ranking_never_disturbs_training_and_sees_finished_updates():
    rs = np.random.RandomState(17)
    spec, params, a = trained_like_model(rs)
    _, _, b = trained_like_model(np.random.RandomState(17))
    _, _, c = trained_like_model(np.random.RandomState(17))
    queries = [rs.randint(0, 2000, rs.randint(1, 12)) for _ in range(20)]
    batches = [random_batch(spec, rs, 64, zipf=True) for _ in range(20)]
    for words, ww, labels, iw, ids in batches:
        for m in (a, b, c):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        ra = a.rank(queries, top_k=50)                      # straight behind nvsm_step: its side-stream tails are still running
        c.synchronize()
        rc = c.rank(queries, top_k=50)
        same_bits(ra, rc)
    after = {n: a.get_param(n) for n in PARAMS}
    s64, err32, tol = chain_tolerance(after, spec, queries, None, "cosine")
    check_result(ra, s64, 50, tol)                            # the scan saw the finished updates of the last step
    for n in list(PARAMS) + ADAM_STATE:                       # b never ranked
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    assert np.abs(after[E_NAME] - params[E_NAME]).max() > 0


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def raw_rank(m, ids, offsets, top_k, similarity=ca.SIM_COSINE, activation=ca.ACT_MODEL):
    ids, offsets = np.asarray(ids, np.int64), np.asarray(offsets, np.int64)
    Q = offsets.size - 1
    q = ca.NvsmQueries(ids.ctypes.data, None, offsets.ctypes.data, Q)
    o = ca.NvsmRankOptions()
    ca.lib().nvsm_rank_options_default(C.byref(o))
    o.top_k, o.similarity, o.activation = top_k, similarity, activation
    k = max(top_k, 1)
    out_ids, out_sc, out_cnt = np.zeros((Q, k), np.int64), np.zeros((Q, k), np.float32), np.zeros(Q, np.int64)
    return ca.lib().nvsm_rank(m._h, C.byref(q), C.byref(o), out_ids.ctypes.data, out_sc.ctypes.data, out_cnt.ctypes.data)


def test_bad_arguments_are_status_codes_and_the_handle_still_trains():
    rs = np.random.RandomState(2)
    spec, params, m = trained_like_model(rs, de=64, dw=16, D=500)
    D = spec["num_entities"]
    assert raw_rank(m, [1, 2, 3], [0, 2, 1, 3], 5) == 1 and b"offsets" in ca.lib().nvsm_last_error()
    assert raw_rank(m, [1, 2, 3], [1, 2, 3], 5) == 1
    assert raw_rank(m, [1, 2, 3], [0, 3], 0) == 1 and b"top_k" in ca.lib().nvsm_last_error()
    assert raw_rank(m, [1, 2, 3], [0, 3], D + 1) == 1
    assert raw_rank(m, [1, 2, 3], [0, 3], 5, similarity=7) == 1
    assert raw_rank(m, [1, 2, 3], [0, 3], 5, activation=9) == 1
    assert raw_rank(m, [1, 2, 3], [0, 3], D) == 0
    for bad in (spec["num_words"], -1):                      # the index contract: row 0 is read, the wait reports it once
        assert raw_rank(m, [1, bad, 3], [0, 3], 5) == 1 and b"word id" in ca.lib().nvsm_last_error()
        assert raw_rank(m, [1, 2, 3], [0, 3], 5) == 0
    with pytest.raises(ValueError):
        m.rank([[1]], top_k=0)
    with pytest.raises(ValueError):
        m.rank([[1]], top_k=D + 1)
    words, ww, labels, iw, ids = random_batch(spec, rs, 64)
    cost = m.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids, want_cost=True)
    assert np.isfinite(cost)
    m.synchronize()
    now = {n: m.get_param(n) for n in PARAMS}
    s64, err32, tol = chain_tolerance(now, spec, [[5, 6, 7]], None, "cosine")
    check_result(m.rank([[5, 6, 7]], top_k=10), s64, 10, tol)


# ---- 9. lazily decayed tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,lam,dims", [("sparse_adam", 0.02, (12, 16)), ("sgd", 0.05, (64, 64)), ("adagrad", 0.05, (300, 256))])
def test_lazy_tables_are_ranked_at_their_logical_values(method, lam, dims, monkeypatch):
    """ranking reads through the LazyView (no flush): the scores are those of the parameters nvsm_get_param returns, and the handle
    trains on, bit for bit, like a twin that did nothing where this one ranked"""
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(num_words=3000, num_entities=5000, word_dim=dims[0], entity_dim=dims[1], window=3, num_random=2,
                nonlinearity="tanh", batch_norm=False, update_method=method)
    spec["lambda"] = lam
    rs = np.random.RandomState(dims[0])
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    a, b = gpu_model(spec, 40), gpu_model(spec, 40)
    for m in (a, b):
        load_params(m, params, True)
    batches = [random_batch(spec, rs, 40, zipf=True) for _ in range(20)]
    # rare words and documents: rows that sit out all ten updates carry ten pending factors when they are ranked
    queries = [rs.randint(0, 3000, rs.randint(2, 9)) for _ in range(40)]
    weights = [rs.uniform(0.5, 2, len(q)).astype(np.float32) for q in queries]

    def ten(lo):
        for words, ww, labels, iw, ids in batches[lo:lo + 10]:
            for m in (a, b):
                m.step(ca.Batch(words, labels, ww, iw), 2e-2, entity_ids=ids)
    ten(0)
    a.profile_enable(True)
    got = {sim: a.rank(queries, top_k=25, weights=weights, similarity=sim) for sim in ("cosine", "dot")}
    a.profile_enable(False)
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0
    for sim in ("cosine", "dot"):
        s64, err32, tol = chain_tolerance(logical, spec, queries, weights, sim)
        worst = check_result(got[sim], s64, 25, tol)
        print("rank-error lazy %s de=%d %s: err32 %.3g, max|s-s64|/err32 %.2f" % (method, dims[1], sim, err32, worst / err32))
    ten(10)
    state = {"sgd": [], "adagrad": ["word_representations/a", "entity_representations/a"], "sparse_adam": ADAM_STATE}[method]
    for n in list(PARAMS) + state:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.profile_enable(True)
    words, ww, labels, iw, ids = batches[0]
    a.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids)
    assert {"lazy_stamp_words", "lazy_stamp_entities"} <= set(a.profile()), "the handle's tables do decay lazily"
