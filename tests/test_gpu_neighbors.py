"""-m gpu: nearest-neighbour search in word, projected-word and document space (nvsm_neighbors / nvsm_similarity, csrc/rank.hip)
against fp64 numpy.

The reference values are fp64 restatements, written here, of the formulas the header pins (include/cunvsm_amd.h):
  words            the rows of W                                    (related_terms / term_similarity, py/nvsm/base.py:325-353)
  projected words  row w = f(T·W[w] + c·b), no batch normalisation  (TermBruteforcer, base.py:106-162)
  entities         the rows of E                                    (query_using_projected_query, base.py:362-430)
  score            cosine similarity (inverse norm 0 for a zero vector) or the dot product
  result           top k by score descending, ties by ascending id; exclude_self leaves the query's own row out

The RANK CORRECTNESS RULE of tests/test_gpu_rank.py is reused unchanged (its functions are imported): tol = 4·err32 with err32
the float32 numpy error of the same formula on the same inputs, computed per case and never from the GPU result; conditions
(a)-(d); the universe excludes the query's own row when exclude_self; at most max(2, k/100) other rows within 2·tol of the
k-th, asserted about the inputs BEFORE the GPU result is read.

Shape sweep: numpy's float32 error differs between hosts (2.2e-7 against 1.0e-6 for one input), and the k = 30
cases sit next to the cap, so every case carries a seed offset for which the cap still holds with the tolerance DOUBLED
(8·err32), checked on the CPU when the cases were written; the test itself asserts the cap at the rule's 4·err32.

Every case prints `nbr-error` lines: err32 and the observed max|s − s64| / err32 (DESIGN.md §10 quotes them)."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import (ADAM_STATE, band_is_narrow, check_query, check_result, make_rows, ref_scores, same_bits,
                                 tolerance)

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS


# ---- fp64 / float32 restatements -----------------------------------------------------------------------------------------------
def project_vocab(params, spec, c=1.0, act="tanh", dtype=np.float64):
    """[num_words][d_e]: f(T·W[w] + c·b) for every word, everything in `dtype`"""
    dw, de = spec["word_dim"], spec["entity_dim"]
    W = params[W_NAME].reshape(-1, dw).astype(dtype)
    T = params[T_NAME].reshape(dw, de).astype(dtype)          # stored T[r + de·c]: [c][r]
    pre = W @ T + dtype(c) * params[B_NAME].astype(dtype)
    if act == "tanh":
        return np.tanh(pre)
    if act == "hard_tanh":
        return np.clip(pre, -1, 1)
    return pre


def space_rows(params, spec, space, dtype, c=1.0, act="tanh"):
    if space == "words":
        return params[W_NAME].reshape(-1, spec["word_dim"]).astype(dtype)
    if space == "entities":
        return params[E_NAME].reshape(-1, spec["entity_dim"]).astype(dtype)
    return project_vocab(params, spec, c, act, dtype)


def chain_tolerance(P64, X64, P32, X32, sim):
    """s64 and tol = 4·err32 of a whole chain evaluated in fp64 (P64, X64) and in float32 (P32, X32)"""
    s64 = ref_scores(P64, X64, sim, np.float64)
    s32 = ref_scores(P32, X32, sim, np.float32)
    err32 = float(np.abs(s32.astype(np.float64) - s64).max())
    return s64, err32, 4.0 * max(err32, 1e-45)


def bands_are_narrow(s64, k, tol, universes=None):
    for q in range(s64.shape[0]):
        band_is_narrow(s64[q], np.arange(s64.shape[1]) if universes is None else universes[q], k, tol)


def all_but(V, ids):
    return [np.delete(np.arange(V), i) for i in ids]


def ref_pairs(A, B, sim, dtype):
    A, B = A.astype(dtype), B.astype(dtype)
    d = (A * B).sum(1, dtype=dtype)
    if sim == "dot":
        return d
    out = d
    for X in (A, B):
        n = np.sqrt((X * X).sum(1, dtype=dtype))
        out = out * np.where(n > 0, dtype(1) / np.where(n > 0, n, 1), dtype(0)).astype(dtype)
    return out


# ---- models ----------------------------------------------------------------------------------------------------------------------
def table_model(space, rows):
    """a handle whose searched table (`space`: "words" or "entities") holds `rows`; the other table is as small as can be"""
    V, d = rows.shape
    if space == "words":
        spec = dict(num_words=V, num_entities=8, word_dim=d, entity_dim=64, window=1, num_random=1, update_method="sgd")
    else:
        spec = dict(num_words=8, num_entities=V, word_dim=64, entity_dim=d, window=1, num_random=1, update_method="sgd")
    m = gpu_model(spec, 8)
    m.set_param(W_NAME if space == "words" else E_NAME, rows)
    return m


def trained_like(rs, de=256, dw=300, D=6000, V=2000, nonlin="tanh", **extra):
    """as tests/test_gpu_rank.py trained_like_model builds one, with the vocabulary's size a parameter"""
    spec = dict(num_words=V, num_entities=D, word_dim=dw, entity_dim=de, window=4, num_random=3, nonlinearity=nonlin,
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    m = gpu_model(spec, 64, **extra)
    load_params(m, params, True)
    return spec, params, m


# ---- 1. the rule over shapes and dispatch paths: by-id queries in the searched table, self excluded ------------------------------
#        V       d    Q    k      rows         space       seed offset  slab MB (None: the default 256)
CASES = [(37,     300, 5,   36,    "uniform",   "words",    0,    None),      # takes every other row
         (37,     300, 5,   37,    "uniform",   "words",    0,    None),      # k = rows: the whole slab survives, one slot fewer is written
         (1000,   300, 64,  30,    "clustered", "words",    1000, None),
         (1000,   36,  300, 999,   "clustered", "entities", 0,    None),      # one chunk plus a tail of 4; Q > 256: two rounds
         (1000,   30,  5,   30,    "uniform",   "words",    0,    None),      # d % 4 != 0: the plain scan
         (50000,  300, 64,  30,    "uniform",   "words",    2000, None),
         (50000,  300, 64,  30,    "clustered", "words",    5000, None),
         (50000,  300, 300, 1000,  "clustered", "words",    0,    None),
         (50000,  128, 64,  30,    "clustered", "entities", 2000, None),      # no tail
         (200000, 300, 5,   1000,  "uniform",   "words",    3000, None),
         (200000, 300, 16,  30,    "clustered", "words",    4000, None),
         (200000, 300, 16,  30,    "clustered", "words",    4000, 1),         # thirteen slabs contribute
         (20000,  300, 1,   19999, "uniform",   "words",    0,    None)]      # global sort


def sweep_inputs(V, d, Q, k, kind, offset):
    rs = np.random.RandomState(V % 1000 + d + Q + k % 997 + offset)
    rows, _ = make_rows(kind, rs, V, d, Q)
    ids = rs.choice(V, Q, replace=False).astype(np.int64)
    return rows, ids


def expected_paths(V, d, Q, k, slab_mb):
    """what ranking.cpp's neighbour dispatch takes for a shape (profile names)"""
    qn = min(Q, 256)
    S = min(V, max(4096, ((slab_mb or 256) << 18) // qn // 4096 * 4096))
    slabs = [min(S, V - d0) for d0 in range(0, V, S)]
    n = sum(min(k, s) for s in slabs)
    names = {"nbr_scan_mfma" if d % 4 == 0 and d >= 32 else "nbr_scan_plain"}
    names |= {"rank_select_radix" if k < s else "rank_select_all" for s in slabs}
    names.add("rank_sort_global" if n > 8192 else "rank_sort_lds")
    return names


ROUTES = {"nbr_scan_mfma", "nbr_scan_plain", "rank_select_radix", "rank_select_all", "rank_sort_lds", "rank_sort_global"}
VISITED = set()


@pytest.mark.parametrize("V,d,Q,k,kind,space,offset,slab_mb", CASES)
def test_neighbor_rule(V, d, Q, k, kind, space, offset, slab_mb, monkeypatch):
    if slab_mb:
        monkeypatch.setenv("NVSM_RANK_SLAB_MB", str(slab_mb))
    rows, ids = sweep_inputs(V, d, Q, k, kind, offset)
    universes = all_but(V, ids)
    checked = {}
    for sim in ("cosine", "dot"):
        s64, err32, tol = tolerance(rows[ids], rows, sim)
        bands_are_narrow(s64, k, tol, universes)               # the test's own inputs, before the GPU result is read
        checked[sim] = (s64, err32, tol)
    m = table_model(space, rows)
    m.profile_enable(True)
    for sim in ("cosine", "dot"):
        s64, err32, tol = checked[sim]
        res = m.neighbors(space, ids=ids, top_k=k, exclude_self=True, similarity=sim)
        assert (res[2] == min(k, V - 1)).all()
        for q in range(Q):
            assert ids[q] not in res[0][q], "the query's own row was returned"
        worst = check_result(res, s64, k, tol, universes=universes)
        print("nbr-error %s V=%d d=%d Q=%d k=%d %s %s slab=%s: err32 %.3g, max|s-s64|/err32 %.2f (of the returned rows)"
              % (space, V, d, Q, k, sim, kind, slab_mb, err32, worst / max(err32, 1e-45)))
    names = {n for n in m.profile() if n in ROUTES}
    assert names == expected_paths(V, d, Q, k, slab_mb), names
    VISITED.update(names)
    m.close()


def test_every_dispatch_path_was_taken():
    want = set()
    for V, d, Q, k, kind, space, offset, slab_mb in CASES:
        want |= expected_paths(V, d, Q, k, slab_mb)
    assert want == ROUTES
    if VISITED:                                                    # (empty when this test is selected on its own)
        assert want <= VISITED, want - VISITED


# ---- 2. the projected vocabulary ---------------------------------------------------------------------------------------------------
PROJ_SLAB_BYTES, PROJ_CHUNK = 64 << 20, 16384                    # ranking.cpp: one projected slab, words projected per launch group


def projected_slabs(V, de, Q):
    S = min(V, max(4096, (256 << 18) // min(Q, 256) // 4096 * 4096), max(4096, PROJ_SLAB_BYTES // (de * 4) // 4096 * 4096))
    return [min(S, V - d0) for d0 in range(0, V, S)]


#                                         (the last: more words than one projected slab of 64 MB / (4·256) = 65 536 rows holds)
@pytest.mark.parametrize("de,nonlin,c,V", [(256, "tanh", 1.0, 2000), (256, "hard_tanh", 0.0, 2000), (36, "tanh", 0.0, 2000),
                                           (36, "hard_tanh", 1.0, 2000), (256, "tanh", 1.0, 70000)])
def test_nearest_terms_in_the_projected_vocabulary(de, nonlin, c, V):
    rs = np.random.RandomState(100 + de + V % 97 + int(c))
    spec, params, m = trained_like(rs, de=de, V=V, nonlin=nonlin)
    D, Q = spec["num_entities"], 7
    ent_ids = rs.choice(D, Q, replace=False).astype(np.int64)
    vectors = rs.standard_normal((Q, de)).astype(np.float32)
    X64, X32 = project_vocab(params, spec, c, nonlin, np.float64), project_vocab(params, spec, c, nonlin, np.float32)
    E = params[E_NAME].reshape(D, de)
    if V > 2000:
        assert len(projected_slabs(V, de, Q)) >= 2
    for what, P in (("entity ids", E[ent_ids]), ("vectors", vectors)):
        for sim in ("cosine", "dot"):
            s64, err32, tol = chain_tolerance(P, X64, P, X32, sim)
            for k in (1, 20, V):
                bands_are_narrow(s64, k, tol)
                m.profile_reset()
                m.profile_enable(True)
                if what == "entity ids":
                    res = m.nearest_terms(entity_ids=ent_ids, top_k=k, similarity=sim, bias_coefficient=c)
                else:
                    res = m.nearest_terms(vectors=vectors, top_k=k, similarity=sim, bias_coefficient=c)
                prof = m.profile()
                m.profile_enable(False)
                worst = check_result(res, s64, k, tol)
                # every slab of the vocabulary was projected, in launch groups of PROJ_CHUNK words, and never more than a slab at once
                assert prof["nbr_project"][1] == sum(-(-s // PROJ_CHUNK) for s in projected_slabs(V, de, Q)), prof["nbr_project"]
                assert "nbr_scan_mfma" in prof and not any(n in prof for n in ("rank_query", "rank_scan", "rank_infer"))
            print("nbr-error projected_words V=%d de=%d %s c=%g %s by %s: err32 %.3g, max|s-s64|/err32 %.2f"
                  % (V, de, nonlin, c, sim, what, err32, worst / max(err32, 1e-45)))
    # the activation and the coefficient are options of the call, as they are nvsm_rank's
    other = "hard_tanh" if nonlin == "tanh" else "tanh"
    Y64, Y32 = project_vocab(params, spec, 0.5, other, np.float64), project_vocab(params, spec, 0.5, other, np.float32)
    s64, err32, tol = chain_tolerance(vectors, Y64, vectors, Y32, "cosine")
    bands_are_narrow(s64, 20, tol)
    check_result(m.nearest_terms(vectors=vectors, top_k=20, bias_coefficient=0.5, activation=other), s64, 20, tol)
    m.close()


# ---- 3. documents near documents ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("de", [256, 36])
def test_related_documents(de):
    rs = np.random.RandomState(41 + de)
    spec, params, m = trained_like(rs, de=de)
    D = spec["num_entities"]
    E = params[E_NAME].reshape(D, de)
    ids = rs.choice(D, 40, replace=False).astype(np.int64)
    for sim in ("cosine", "dot"):
        s64, err32, tol = tolerance(E[ids], E, sim)
        for k, exclude in ((10, False), (10, True), (D, True), (D, False)):
            universes = all_but(D, ids) if exclude else None
            bands_are_narrow(s64, k, tol, universes)
            res = m.neighbors("entities", ids=ids, top_k=k, exclude_self=exclude, similarity=sim)
            if sim == "cosine":
                same_bits(res, m.related_documents(ids, top_k=k, exclude_self=exclude))
            worst = check_result(res, s64, k, tol, universes=universes)
            if not exclude and sim == "cosine":
                assert (res[0][:, 0] == ids).all(), "a document is its own nearest neighbour"
        print("nbr-error entities de=%d %s: err32 %.3g, max|s-s64|/err32 %.2f" % (de, sim, err32, worst / err32))
    m.close()


@pytest.mark.parametrize("de", [256, 64])
def test_projected_single_word_queries_return_what_nvsm_rank_returns(de):
    """queries = projected words, searched space = documents: nvsm_rank of one-word queries, id for id and bit for bit"""
    rs = np.random.RandomState(43 + de)
    spec, params, m = trained_like(rs, de=de)
    words = rs.randint(0, spec["num_words"], 300).astype(np.int64)           # two rounds
    for opts in (dict(), dict(bias_coefficient=0.0, activation="hard_tanh"), dict(similarity="dot", activation="identity")):
        for k in (1, 50, spec["num_entities"]):
            want = m.rank([[w] for w in words], top_k=k, **opts)
            got = m.neighbors("entities", ids=words, source="projected_words", top_k=k, **opts)
            same_bits(want, got)
    m.close()


# ---- 4. nvsm_similarity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("de", [256, 36])
def test_similarity_of_pairs(de):
    rs = np.random.RandomState(51 + de)
    spec, params, m = trained_like(rs, de=de)
    params[W_NAME].reshape(-1, spec["word_dim"])[5] = 0.0
    params[E_NAME].reshape(-1, de)[5] = 0.0
    load_params(m, params, True)
    n = 5000                                                      # more than one round of pairs
    for space in ("words", "projected_words", "entities"):
        X64 = space_rows(params, spec, space, np.float64, 1.0, "tanh")
        X32 = space_rows(params, spec, space, np.float32, 1.0, "tanh")
        R = X64.shape[0]
        a, b = rs.randint(0, R, n).astype(np.int64), rs.randint(0, R, n).astype(np.int64)
        a[:3], b[:3] = (5, 7, 5), (9, 5, 5)                       # the zero row (zero only in the two tables) on either side
        for sim in ("cosine", "dot"):
            s64, s32 = ref_pairs(X64[a], X64[b], sim, np.float64), ref_pairs(X32[a], X32[b], sim, np.float32)
            err32 = float(np.abs(s32.astype(np.float64) - s64).max())
            got = m.similarity(space, a, b, similarity=sim)
            assert got.dtype == np.float32 and got.shape == (n,) and not np.isnan(got).any()
            err = float(np.abs(got.astype(np.float64) - s64).max())
            print("nbr-error similarity %s de=%d %s: err32 %.3g, max|s-s64|/err32 %.2f" % (space, de, sim, err32, err / err32))
            assert err <= 4 * err32, (space, sim, err, err32)
            if space != "projected_words":
                assert (got[:3] == 0).all() and not np.signbit(got[:3]).any(), "a zero row scores exactly +0"
            same = m.similarity(space, a, a, similarity="cosine")
            ones = ref_pairs(X64[a], X64[a], "cosine", np.float64)
            e32 = float(np.abs(ref_pairs(X32[a], X32[a], "cosine", np.float32).astype(np.float64) - ones).max())
            assert np.abs(same.astype(np.float64) - ones).max() <= 4 * e32
    ws = rs.randint(6, spec["num_words"], 50)
    X64, X32 = space_rows(params, spec, "words", np.float64), space_rows(params, spec, "words", np.float32)
    e32 = float(np.abs(ref_pairs(X32[ws], X32[ws], "cosine", np.float32).astype(np.float64) - 1).max())
    assert np.abs(m.term_similarity(ws, ws).astype(np.float64) - 1).max() <= 4 * e32, "term_similarity(a, a) is 1 within tol"
    assert isinstance(m.term_similarity(7, 9), float) and m.term_similarity(5, 9) == 0.0
    m.close()


# ---- 5. ties and zeros ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,slab_mb", [(300, None), (30, None), (64, 1)])
def test_ties_zero_rows_and_the_zero_query(d, slab_mb, monkeypatch):
    if slab_mb:
        monkeypatch.setenv("NVSM_RANK_SLAB_MB", str(slab_mb))
    rs = np.random.RandomState(d)
    V = 9000
    distinct = rs.standard_normal((50, d)).astype(np.float32)
    W = rs.standard_normal((V, d)).astype(np.float32)
    copies = rs.choice(V, 5200, replace=False)
    W[copies[:5000]] = distinct[rs.randint(0, 50, 5000)]
    W[copies[5000:]] = 0.0
    groups = [np.flatnonzero((W == distinct[j]).all(1)) for j in range(50)]
    assert sum(g.size for g in groups) == 5000
    plain = np.setdiff1d(np.arange(V), copies)
    nq = 64 if slab_mb else 4                                     # (64 queries x 1 MB: slabs of 4 096 rows, three of them)
    ids = np.concatenate([plain[:nq - 2], copies[:1], copies[5000:5001]]).astype(np.int64)      # ..., a copied row, a zero row
    m = table_model("words", W)
    for sim in ("cosine", "dot"):
        s64, s32 = ref_scores(W[ids], W, sim), ref_scores(W[ids], W, sim, np.float32)
        tol = 4 * np.abs(s32.astype(np.float64) - s64).max()
        got, sc, cnt = m.neighbors("words", ids=ids, top_k=V, similarity=sim)
        assert (cnt == V).all() and not np.isnan(sc).any()
        for q in range(nq):
            assert np.array_equal(np.sort(got[q]), np.arange(V))
            by_id = np.empty(V, np.float32)
            by_id[got[q]] = sc[q]
            assert (by_id[copies[5000:]] == 0).all() and not np.signbit(by_id[copies[5000:]]).any(), "zero rows score exactly +0"
            for rows in groups:                                      # copies of a row: one score, bit for bit
                assert np.unique(by_id[rows].view(np.uint32)).size == 1
            dd = np.diff(sc[q])
            assert (dd <= 0).all() and (np.diff(got[q])[dd == 0] > 0).all(), "equal scores in ascending id order"
            assert np.abs(by_id.astype(np.float64) - s64[q]).max() <= tol
        # a smaller k is a prefix of the full order; with exclude_self the same order without the own row
        for k in (1, 7, 100, 5203):
            g_k, s_k, c_k = m.neighbors("words", ids=ids, top_k=k, similarity=sim)
            assert (c_k == k).all()
            np.testing.assert_array_equal(g_k, got[:, :k])
            np.testing.assert_array_equal(s_k.view(np.uint32), sc[:, :k].view(np.uint32))
        for k in (7, 5203, V):
            g_x, s_x, c_x = m.neighbors("words", ids=ids, top_k=k, similarity=sim, exclude_self=True)
            n = min(k, V - 1)
            assert (c_x == n).all()
            for q in range(nq):
                keep = got[q] != ids[q]
                np.testing.assert_array_equal(g_x[q, :n], got[q][keep][:n])
                np.testing.assert_array_equal(s_x[q, :n].view(np.uint32), sc[q][keep][:n].view(np.uint32))
                assert (g_x[q, n:] == -1).all() and np.isneginf(s_x[q, n:]).all()
        # the zero query row: every score 0, so the ids are 0 .. k − 1 — minus its own id when that is left out
        zero = int(ids[-1])
        for k in (1, 10, 1000, V):
            g0, s0, c0 = m.neighbors("words", ids=[zero], top_k=k, similarity=sim)
            assert c0[0] == k and (s0 == 0).all() and not np.signbit(s0).any()
            np.testing.assert_array_equal(g0[0], np.arange(k))
            g1, s1, c1 = m.neighbors("words", ids=[zero], top_k=k, similarity=sim, exclude_self=True)
            n = min(k, V - 1)
            assert c1[0] == n and (s1[0, :n] == 0).all()
            np.testing.assert_array_equal(g1[0, :n], np.delete(np.arange(V), zero)[:n])
    m.close()


# ---- 6. lazily decayed tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,lam,dims", [("sparse_adam", 0.02, (12, 16)), ("sgd", 0.05, (64, 64)), ("adagrad", 0.05, (300, 256))])
def test_lazy_tables_are_searched_at_their_logical_values(method, lam, dims, monkeypatch):
    """the constructions of test_lazy_tables_are_ranked_at_their_logical_values: neighbours read through the LazyView (no flush),
    and the handle trains on, bit for bit, like a twin that did nothing where this one searched"""
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
    # rare words and documents: rows that sit out all ten updates carry ten pending factors when they are searched
    wids = rs.choice(3000, 30, replace=False).astype(np.int64)
    eids = rs.choice(5000, 30, replace=False).astype(np.int64)
    pa, pb = rs.randint(0, 3000, 200).astype(np.int64), rs.randint(0, 3000, 200).astype(np.int64)
    k = 25

    def ten(lo):
        for words, ww, labels, iw, ids in batches[lo:lo + 10]:
            for m in (a, b):
                m.step(ca.Batch(words, labels, ww, iw), 2e-2, entity_ids=ids)
    ten(0)
    got = {}
    for sim in ("cosine", "dot"):                            # straight behind nvsm_step: its side-stream tails are still running
        got["words", sim] = a.neighbors("words", ids=wids, top_k=k, exclude_self=True, similarity=sim)
        got["entities", sim] = a.neighbors("entities", ids=eids, top_k=k, exclude_self=True, similarity=sim)
        got["projected_words", sim] = a.nearest_terms(entity_ids=eids, top_k=k, similarity=sim)
        got["pairs words", sim] = a.similarity("words", pa, pb, similarity=sim)
        got["pairs entities", sim] = a.similarity("entities", pa, pb, similarity=sim)
        got["pairs projected_words", sim] = a.similarity("projected_words", pa, pb, similarity=sim)
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0 and np.abs(logical[W_NAME] - params[W_NAME]).max() > 0
    for sim in ("cosine", "dot"):
        for space, qspace, ids in (("words", "words", wids), ("entities", "entities", eids), ("projected_words", "entities", eids)):
            X64, X32 = space_rows(logical, spec, space, np.float64), space_rows(logical, spec, space, np.float32)
            P = space_rows(logical, spec, qspace, np.float32)[ids]
            s64, err32, tol = chain_tolerance(P, X64, P, X32, sim)
            universes = all_but(X64.shape[0], ids) if space == qspace else None
            worst = check_result(got[space, sim], s64, k, tol, universes=universes)
            print("nbr-error lazy %s %s d=%d %s: err32 %.3g, max|s-s64|/err32 %.2f" % (method, space, X64.shape[1], sim, err32, worst / err32))
            s64p, s32p = ref_pairs(X64[pa], X64[pb], sim, np.float64), ref_pairs(X32[pa], X32[pb], sim, np.float32)
            e32 = float(np.abs(s32p.astype(np.float64) - s64p).max())
            assert np.abs(got["pairs " + space, sim].astype(np.float64) - s64p).max() <= 4 * e32
    ten(10)
    state = {"sgd": [], "adagrad": ["word_representations/a", "entity_representations/a"], "sparse_adam": ADAM_STATE}[method]
    for n in list(PARAMS) + state:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.profile_enable(True)
    words, ww, labels, iw, ids = batches[0]
    a.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids)
    assert {"lazy_stamp_words", "lazy_stamp_entities"} <= set(a.profile()), "the handle's tables do decay lazily"


def test_searching_in_the_middle_of_training_leaves_the_handle_bit_equal_to_a_twin():
    rs = np.random.RandomState(19)
    spec, params, a = trained_like(rs)
    _, _, b = trained_like(np.random.RandomState(19))
    batches = [random_batch(spec, rs, 64, zipf=True) for _ in range(20)]
    ids = rs.choice(2000, 20, replace=False).astype(np.int64)
    for words, ww, labels, iw, eids in batches:
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=eids)
        a.related_terms(ids, top_k=30)
        a.nearest_terms(entity_ids=ids, top_k=20)
        a.related_documents(ids, top_k=10, exclude_self=True)
        a.term_similarity(ids, ids[::-1])
    for n in list(PARAMS) + ADAM_STATE:                       # b never searched
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    after = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(after[W_NAME] - params[W_NAME]).max() > 0
    W = after[W_NAME].reshape(-1, 300)
    s64, err32, tol = tolerance(W[ids], W, "cosine")
    bands_are_narrow(s64, 30, tol)
    check_result(a.related_terms(ids, top_k=30), s64, 30, tol)      # the scan sees the finished updates of the last step


# ---- 7. same call, same bits -----------------------------------------------------------------------------------------------------------
def test_same_call_same_bits_on_two_handles_and_across_a_repeat():
    rs = np.random.RandomState(3)
    spec, params, a = trained_like(rs)
    _, _, b = trained_like(np.random.RandomState(3))
    wids = rs.choice(2000, 70, replace=False).astype(np.int64)
    eids = rs.choice(6000, 70, replace=False).astype(np.int64)
    vec = rs.standard_normal((70, 256)).astype(np.float32)
    calls = [lambda m: m.related_terms(wids, top_k=30),
             lambda m: m.neighbors("words", ids=wids, top_k=100, exclude_self=True, similarity="dot"),
             lambda m: m.nearest_terms(entity_ids=eids, top_k=20),
             lambda m: m.nearest_terms(vectors=vec, top_k=2000, bias_coefficient=0.0),
             lambda m: m.related_documents(eids, top_k=100),
             lambda m: m.neighbors("projected_words", ids=wids, top_k=50, exclude_self=True),
             lambda m: (m.similarity("projected_words", wids, wids[::-1]),)]
    for call in calls:
        r1, r2, r3 = call(a), call(a), call(b)
        same_bits(r1, r2)
        same_bits(r1, r3)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def raw_neighbors(m, space, top_k, ids=None, source=0, vectors=None, dim=0, similarity=ca.SIM_COSINE, activation=ca.ACT_MODEL,
                  exclude_self=0, bias=1.0):
    q, o = ca.NvsmNeighborQueries(), ca.NvsmNeighborOptions()
    ca.lib().nvsm_neighbor_options_default(C.byref(o))
    keep = []
    n = 0
    if ids is not None:
        keep.append(np.asarray(ids, np.int64))
        q.ids, n = keep[-1].ctypes.data, keep[-1].size
    if vectors is not None:
        keep.append(np.ascontiguousarray(vectors, np.float32))
        q.vectors, n = keep[-1].ctypes.data, keep[-1].shape[0]
    q.num_queries, q.source_space, q.dim = n, source, dim
    o.space, o.top_k, o.similarity, o.activation, o.exclude_self, o.bias_coefficient = space, top_k, similarity, activation, exclude_self, bias
    k = max(top_k, 1)
    out_ids, out_sc, out_cnt = np.zeros((max(n, 1), k), np.int64), np.zeros((max(n, 1), k), np.float32), np.zeros(max(n, 1), np.int64)
    return ca.lib().nvsm_neighbors(m._h, C.byref(q), C.byref(o), out_ids.ctypes.data, out_sc.ctypes.data, out_cnt.ctypes.data)


def test_bad_arguments_are_status_codes_and_the_handle_still_trains():
    rs = np.random.RandomState(2)
    spec, params, m = trained_like(rs, de=64, dw=16, D=500, V=300)
    V, D = spec["num_words"], spec["num_entities"]
    WORDS, PROJ, ENTS = ca.SPACE_WORDS, ca.SPACE_PROJECTED_WORDS, ca.SPACE_ENTITIES
    err = ca.lib().nvsm_last_error
    assert raw_neighbors(m, WORDS, 5, ids=[1, 2], source=WORDS) == 0
    assert raw_neighbors(m, WORDS, 5, ids=[1, 2], source=ENTS) == 1 and b"dimension" in err()
    assert raw_neighbors(m, ENTS, 5, ids=[1, 2], source=WORDS) == 1 and b"dimension" in err()
    assert raw_neighbors(m, PROJ, 5, vectors=np.zeros((2, 16)), dim=16) == 1 and b"dim" in err()
    assert raw_neighbors(m, PROJ, 5, vectors=np.zeros((2, 64)), dim=64) == 0
    assert raw_neighbors(m, WORDS, 5, ids=[1, V], source=WORDS) == 1 and b"outside" in err()
    assert raw_neighbors(m, WORDS, 5, ids=[-1], source=WORDS) == 1
    assert raw_neighbors(m, PROJ, 5, ids=[D], source=ENTS) == 1
    assert raw_neighbors(m, 3, 5, ids=[1], source=WORDS) == 1 and b"space" in err()
    assert raw_neighbors(m, WORDS, 5, ids=[1], source=-1) == 1 and b"space" in err()
    assert raw_neighbors(m, WORDS, 5, ids=[1], source=WORDS, similarity=7) == 1 and b"similarity" in err()
    assert raw_neighbors(m, PROJ, 5, ids=[1], source=ENTS, activation=9) == 1 and b"activation" in err()
    assert raw_neighbors(m, PROJ, 5, ids=[1], source=ENTS, bias=float("nan")) == 1
    assert raw_neighbors(m, WORDS, 0, ids=[1], source=WORDS) == 1 and b"top_k" in err()
    assert raw_neighbors(m, WORDS, V + 1, ids=[1], source=WORDS) == 1 and b"top_k" in err()
    assert raw_neighbors(m, ENTS, D + 1, ids=[1], source=ENTS) == 1
    assert raw_neighbors(m, ENTS, D, ids=[1], source=ENTS) == 0
    assert raw_neighbors(m, WORDS, 5) == 1 and b"exactly one" in err()
    assert raw_neighbors(m, WORDS, 5, ids=[1], source=WORDS, vectors=np.zeros((1, 16)), dim=16) == 1 and b"exactly one" in err()
    assert raw_neighbors(m, ENTS, 5, ids=[1], source=PROJ, exclude_self=1) == 1 and b"exclude_self" in err()
    assert raw_neighbors(m, ENTS, 5, vectors=np.zeros((1, 64)), dim=64, exclude_self=1) == 1 and b"exclude_self" in err()
    assert raw_neighbors(m, ENTS, D, ids=[1], source=ENTS, exclude_self=1) == 0
    a, b, out = np.array([1, 2], np.int64), np.array([3, V], np.int64), np.zeros(2, np.float32)
    L = ca.lib()
    assert L.nvsm_similarity(m._h, WORDS, a.ctypes.data, b.ctypes.data, 2, 0, out.ctypes.data) == 1 and b"outside" in err()
    assert L.nvsm_similarity(m._h, 5, a.ctypes.data, a.ctypes.data, 2, 0, out.ctypes.data) == 1 and b"space" in err()
    assert L.nvsm_similarity(m._h, WORDS, a.ctypes.data, a.ctypes.data, 2, 4, out.ctypes.data) == 1 and b"similarity" in err()
    assert L.nvsm_similarity(m._h, WORDS, a.ctypes.data, a.ctypes.data, -1, 0, out.ctypes.data) == 1
    assert L.nvsm_similarity(m._h, WORDS, a.ctypes.data, a.ctypes.data, 2, 0, out.ctypes.data) == 0
    with pytest.raises(ValueError):
        m.related_terms([1], top_k=V + 1)
    words, ww, labels, iw, ids = random_batch(spec, rs, 64)
    cost = m.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids, want_cost=True)
    assert np.isfinite(cost)
    m.synchronize()
    W = m.get_param(W_NAME).reshape(V, 16)
    s64, err32, tol = tolerance(W[[5, 6, 7]], W, "cosine")
    bands_are_narrow(s64, 10, tol)
    check_result(m.related_terms([5, 6, 7], top_k=10), s64, 10, tol)


# ---- 9. profile names ----------------------------------------------------------------------------------------------------------------
def test_a_neighbor_call_records_no_new_rank_names():
    rs = np.random.RandomState(5)
    spec, params, m = trained_like(rs, de=64, dw=300, D=500, V=400)
    m.profile_enable(True)
    m.synchronize()
    assert not any(n.startswith(("rank_", "nbr_")) for n in m.profile())
    m.related_terms([1, 2], top_k=30)
    m.nearest_terms(entity_ids=[3], top_k=20)
    m.related_documents([4], top_k=10, exclude_self=True)
    m.neighbors("entities", ids=[5], source="projected_words", top_k=10)
    m.term_similarity([1], [2])
    m.similarity("projected_words", [1], [2])
    names = set(m.profile())
    # the selection and the sort keep their names; nothing of the query side or the scans of infer / rank is recorded
    assert {n for n in names if n.startswith("rank_")} == {"rank_select", "rank_select_radix", "rank_sort", "rank_sort_lds"}
    assert {n for n in names if n.startswith("nbr_")} == {"nbr_scan", "nbr_scan_mfma", "nbr_project", "nbr_gather", "nbr_pairs"}
    m.rank([[1, 2]], top_k=10)
    before = {n for n in m.profile() if n.startswith("rank_")}
    assert before == {"rank_query", "rank_scan", "rank_scan_mfma", "rank_select", "rank_select_radix", "rank_sort", "rank_sort_lds"}
    m.related_terms([1, 2], top_k=30)
    m.nearest_terms(vectors=np.ones((2, 64), np.float32), top_k=20)
    m.related_documents([4], top_k=10)
    assert {n for n in m.profile() if n.startswith("rank_")} == before
