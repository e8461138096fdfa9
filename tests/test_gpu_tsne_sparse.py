"""nvsm_tsne_sparse on the device (include/cunvsm_amd.h; kernels: csrc/tsne_sparse.hip) against tests/tsne_sparse_reference.py, the
fp64 numpy restatement that tests/test_tsne_sparse_reference.py holds to scikit-learn's barnes_hut method at angle 0 on the CPU.
Nothing here reads scikit-learn.

TOLERANCE RULE (tests/test_gpu_tsne.py's): the fp64 value and err32, the deviation of the float32 numpy chain from it, both come from
the reference; the device must stay within 4·err32; neither is ever taken from the device. Every group prints `tsne-sparse-error`
lines with err32 and the observed ratio (DESIGN.md §25 quotes the worst of each). An error (KL) is ONE number: its err32 is the
largest deviation over VARIANTS relabelled float32 runs.

Shapes: n in {2, 3, 63, 64, 65, 257, 300} (rows end inside a wave, at a 64-row workgroup's edge and one past it; 257 and 300 end
inside a 256-column step of a tile), d in {1, 6, 36, 300}; 4097 crosses an LDS tile of 4096 columns when one range is forced; 32 769
is one past nvsm_tsne's cap. perplexity 30 where n > 90, else max(1.5, n / 4); k is sklearn's min(n − 1, int(3·perplexity + 1))."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import check
from tests import tsne_reference as tr
from tests import tsne_sparse_reference as ts
from tests.conftest import ROOT
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE
from tests.test_gpu_tsne import float32_runs, perplexity_of, ptr, rows_of, table_model, worst

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
GUARD = np.float32(12345.0)
VARIANTS = 6


# ---- the hooks -------------------------------------------------------------------------------------------------------------------------
def hook_knn(X, k, round_rows=0):
    n, d = X.shape
    ids, d2 = np.full((n, k), -7, dtype=np.int32), np.full((n, k), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_knn(ptr(X), n, d, k, round_rows, ptr(ids), ptr(d2)))
    return ids, d2


def hook_affinities(X, perplexity, k):
    n, d = X.shape
    indptr = np.full(n + 1, -7, dtype=np.int64)
    indices, data = np.full(2 * n * k, -7, dtype=np.int32), np.full(2 * n * k, GUARD, dtype=np.float32)
    cond = np.full((n, k), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_sparse_affinities(ptr(X), n, d, perplexity, k, ptr(indptr), ptr(indices), ptr(data), ptr(cond)))
    nnz = int(indptr[n])
    assert 0 < nnz <= 2 * n * k and (indices[nnz:] == -7).all() and (data[nnz:] == GUARD).all(), "nothing is written past the matrix"
    return indptr, indices[:nnz].copy(), data[:nnz].copy(), cond


def hook_gradient(csr, Y, exaggeration, ranges=0):
    indptr, indices, data = csr
    n = len(Y)
    g, kl = np.full((n, 2), GUARD, dtype=np.float32), C.c_double(-1.0)
    check(ca.lib().nvsm_debug_tsne_sparse_gradient(ptr(indptr), ptr(indices), ptr(data), ptr(Y), n, exaggeration, ranges, ptr(g), C.byref(kl)))
    return g, kl.value


def hook_descent(csr, Y0, lr, exploration, max_iter, min_grad_norm=1e-7, without_progress=300, exaggeration=12.0):
    indptr, indices, data = csr
    o = ca.NvsmTsneOptions()
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    o.learning_rate, o.max_iter, o.min_grad_norm, o.n_iter_without_progress, o.early_exaggeration = lr, max_iter, min_grad_norm, without_progress, exaggeration
    Y = np.ascontiguousarray(Y0, dtype=np.float32).copy()
    kl, it = C.c_double(-1.0), C.c_int32(-1)
    check(ca.lib().nvsm_debug_tsne_sparse_descent(ptr(indptr), ptr(indices), ptr(data), ptr(Y), len(Y), C.byref(o), exploration, C.byref(kl),
                                                 C.byref(it)))
    return Y, kl.value, it.value


def csr32(indptr, indices, data):
    """a reference matrix as the hooks take it"""
    return np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(data, dtype=np.float32)


# ---- inputs, and their references computed once ---------------------------------------------------------------------------------------------
def sparse_rows(kind, n, d):
    rs = np.random.RandomState(n * 1000 + d)
    if kind == "outlier":          # one row far from every other: in no list but its own (in-degree 0)
        X = rs.standard_normal((n, d))
        X[n // 3] += 100.0
        return X.astype(np.float32)
    if kind == "hub":              # a row at the centre of n − 1 rows on a sphere: nearer to each than any of them to another
        X = rs.standard_normal((n, d))
        X /= np.sqrt((X * X).sum(axis=1))[:, None]
        X[0] = 0.0
        return X.astype(np.float32)
    if kind == "grid":             # rows from {0, 1, 2, 3}^6: every sum is exact in fp32 and fp64 alike, and ties abound
        return rs.randint(0, 4, size=(n, d)).astype(np.float32)
    if kind == "twins":            # distinct integer rows, each of them twice: row i and row i + n / 2
        half = np.unique(rs.randint(0, 8, size=(4 * n, d)), axis=0)
        half = half[rs.permutation(len(half))[:n // 2]].astype(np.float32)
        assert len(half) == n // 2
        return np.concatenate([half, half])
    return rows_of(kind, rs, n, d)


_REF = {}


def reference(kind, n, d, perplexity=None, k=None):
    """X, perplexity, k and the fp64 / float32 affinities (affinities_nn's tuples) of a case, shared between the tests"""
    key = (kind, n, d, perplexity, k)
    if key not in _REF:
        X = sparse_rows(kind, n, d)
        perp = perplexity_of(n) if perplexity is None else perplexity
        kk = ts.default_neighbors(n, perp) if k is None else k
        _REF[key] = dict(X=X, perp=perp, k=kk, a64=ts.affinities_nn(X, perp, kk), a32=ts.affinities_nn(X, perp, kk, np.float32))
    return _REF[key]


def adjacent_or_equal(a, b):
    """float32 values that are equal or neighbouring floats (both non-negative)"""
    ia, ib = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64), np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib) <= 1


def neighbour_rule(X, ids, d2, k, rows=None, label=""):
    """the neighbour rule: distances within one fp32 ulp of the reference's, position by position; a row is never its own neighbour;
    distances ascend and equal ones come by ascending id; the ids are the reference's except in rows whose reference k-th and (k+1)-th
    distances are equal or adjacent floats — at most 1 % of the rows"""
    n = len(X)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    ids64, d64 = ts.knn(X, min(k + 1, n - 1), rows=rows)
    assert adjacent_or_equal(d2, d64[:, :k]).all(), "a distance is more than one fp32 ulp from the reference"
    assert not (ids == rows[:, None]).any() and (ids >= 0).all() and (ids < n).all()
    assert (np.diff(d2, axis=1) >= 0).all()
    tied = np.diff(d2, axis=1) == 0
    assert (np.diff(ids, axis=1)[tied] > 0).all(), "equal distances come by ascending id"
    band = adjacent_or_equal(d64[:, k - 1], d64[:, k]) if ids64.shape[1] > k else np.zeros(len(rows), dtype=bool)
    same = (ids == ids64[:, :k]).all(axis=1)
    print("tsne-sparse-error neighbours %s n=%d k=%d: %d of %d rows in the band, %d rows differ" % (label, n, k, band.sum(), len(rows), (~same).sum()))
    assert band.mean() <= 0.01
    assert same[~band].all()
    return same.all()


# ---- 1. neighbours -------------------------------------------------------------------------------------------------------------------------
NEIGHBOUR_CASES = [("gauss", 2, 1, 0), ("gauss", 3, 6, 0), ("gauss", 63, 36, 0), ("l2", 64, 300, 0), ("gauss", 65, 6, 0), ("gauss", 257, 36, 0),
                   ("gauss", 300, 1, 0), ("gauss", 300, 6, 0), ("gauss", 300, 300, 0), ("gauss", 300, 6, 7)]


@pytest.mark.parametrize("kind,n,d,round_rows", NEIGHBOUR_CASES, ids=lambda v: str(v))
def test_neighbours(kind, n, d, round_rows):
    r = reference(kind, n, d)
    ids, d2 = hook_knn(r["X"], r["k"], round_rows)      # round_rows 7 at n = 300: 43 rounds, the last one of 6 rows
    neighbour_rule(r["X"], ids, d2, r["k"], label="%s d=%d rounds of %d" % (kind, d, round_rows))
    if round_rows:
        whole = hook_knn(r["X"], r["k"], 0)
        assert np.array_equal(ids, whole[0]) and np.array_equal(d2.view(np.uint32), whole[1].view(np.uint32)), "the rounds do not show in the result"


@pytest.mark.parametrize("kind", ["grid", "twins"])
def test_neighbours_bit_for_bit_where_the_sums_are_exact(kind):
    n, d, k = 130, 6, 91
    X = sparse_rows(kind, n, d)
    ids64, d64 = ts.knn(X, k)
    for round_rows in (0, 7):
        ids, d2 = hook_knn(X, k, round_rows)
        assert np.array_equal(ids, ids64), "massive exact ties: ascending id decides"
        assert np.array_equal(d2.view(np.uint32), d64.view(np.uint32))      # (+0 at distance 0: never −0)
    if kind == "twins":
        twin = (np.arange(n) + n // 2) % n
        assert (d2[:, 0] == 0).all() and np.array_equal(ids[:, 0], twin) and (d2[:, 1] > 0).all()
    else:
        assert (np.diff(d64, axis=1) == 0).mean() > 0.5, "the grid must tie"


# ---- 2. affinities -----------------------------------------------------------------------------------------------------------------------
AFFINITY_CASES = [("gauss", 2, 1, None, None), ("gauss", 3, 6, None, None), ("gauss", 63, 36, None, None), ("l2", 64, 300, None, None),
                  ("gauss", 65, 6, None, None), ("gauss", 257, 36, None, None), ("gauss", 300, 1, None, None), ("gauss", 300, 6, None, None),
                  ("gauss", 300, 300, None, None), ("outlier", 130, 6, None, None), ("hub", 130, 32, 1.5, None), ("l2", 300, 36, None, None),
                  ("gauss", 65, 6, None, 64)]


def cells(indptr, indices):
    n = len(indptr) - 1
    return ts._entry_rows(indptr).astype(np.int64) * n + indices


@pytest.mark.parametrize("kind,n,d,perplexity,k", AFFINITY_CASES, ids=lambda v: str(v))
def test_affinities(kind, n, d, perplexity, k):
    r = reference(kind, n, d, perplexity, k)
    X, perp, k = r["X"], r["perp"], r["k"]
    ip64, ix64, dt64, ids64, d64, C64, steps = r["a64"]
    indptr, indices, data, cond = hook_affinities(X, perp, k)
    # structure, exact
    rows = ts._entry_rows(indptr)
    assert indptr[0] == 0 and (np.diff(indptr) >= k).all() and indptr[n] == len(indices) == len(data)
    assert (indices >= 0).all() and (indices < n).all() and (indices != rows).all()
    assert (np.diff(indices)[np.diff(rows) == 0] > 0).all(), "columns ascend strictly inside a row"
    mine = cells(indptr, indices)
    mirror = indices.astype(np.int64) * n + rows
    order = np.argsort(mirror)
    assert np.array_equal(mirror[order], mine), "the pattern is symmetric"
    assert np.array_equal(data[order].view(np.uint32), data.view(np.uint32)), "P_ij and P_ji are the same bits"
    ids, d2 = hook_knn(X, k)
    own = np.unique(np.concatenate([np.repeat(np.arange(n), k) * n + ids.ravel(), ids.ravel().astype(np.int64) * n + np.repeat(np.arange(n), k)]))
    assert np.array_equal(own, mine), "the pattern is the union of both directions of the device's own edges"
    if kind == "outlier":
        assert indptr[n // 3 + 1] - indptr[n // 3] == k and not (ids == n // 3).any()      # in no list but its own
    if kind == "hub":
        assert indptr[1] - indptr[0] == n - 1 and (ids[1:] == 0).any(axis=1).all() and k == 5      # in every list: a row of n − 1 >> k entries
    agreed = neighbour_rule(X, ids, d2, k, label="(affinities) " + kind)
    # values by the rule; where the float32 chain, or the device, chose another neighbour in a tie, over the cells both store
    ref = cells(ip64, ix64)
    if agreed:
        assert np.array_equal(mine, ref), "the pattern is the union of the reference's edges"
    at, at64 = np.isin(mine, ref), np.isin(ref, mine)
    ref32 = cells(r["a32"][0], r["a32"][1])
    b32, b64 = np.isin(ref32, ref), np.isin(ref, ref32)
    # relative to the value, down to sklearn's MACHINE_EPSILON: the sparse path clamps no cell, so some lie far below what the exact
    # path lifts to eps, where a float32 chain has no digit left and a relative figure would let anything through
    err32 = worst(r["a32"][2][b32], dt64[b64], np.maximum(dt64[b64], tr.EPS)) if n > 2 else 2.0 ** -24      # two points: 0.5 exactly in any arithmetic
    got = worst(data[at], dt64[at64], np.maximum(dt64[at64], tr.EPS))
    total = data.astype(np.float64).sum()
    print("tsne-sparse-error affinities %s n=%d d=%d k=%d: nnz %d, err32 %.3g, max relative |P - P64| / err32 %.3g, ΣP − 1 = %.3g, search steps %d..%d"
          % (kind, n, d, k, len(data), err32, got / err32, total - 1.0, steps.min(), steps.max()))
    assert got <= 4 * err32
    assert abs(total - 1.0) <= 2.0 ** -23
    # the conditionals beside the neighbour lists: the entropy every converged row realises
    assert (cond >= 0).all() and (cond <= 1).all()
    target = float(np.log(np.float64(np.float32(perp))))
    converged = steps < 100
    if k > perp and converged.any():
        entropy = np.array([ts.row_entropy_nn(cond[i]) for i in np.nonzero(converged)[0]])
        assert np.abs(entropy - target).max() <= 1.1e-5, np.abs(entropy - target).max()


def test_with_every_other_row_a_neighbour_the_matrix_is_the_exact_calls():
    """k = n − 1: the sparse matrix against nvsm_debug_tsne_affinities' dense one, outside the cells that one clamps to eps. Both
    searches see the same distances but add them in another order (256 threads over a row of n, 64 over a sorted row of n − 1), so
    they agree to the rule's err32, not bit for bit."""
    from tests.test_gpu_tsne import hook_affinities as dense_affinities
    r = reference("gauss", 65, 6, None, 64)
    indptr, indices, data, _ = hook_affinities(r["X"], r["perp"], 64)
    dense, _ = dense_affinities(r["X"], r["perp"])
    P = ts.densify(indptr, indices, data, np.float32)
    free = dense > np.float32(tr.EPS)
    dt64 = r["a64"][2]
    err32 = worst(r["a32"][2], dt64, dt64)
    got = float((np.abs(P.astype(np.float64) - dense)[free] / dense[free]).max())
    print("tsne-sparse-error affinities k = n - 1 against the exact call: err32 %.3g, max relative difference / err32 %.3g, clamped cells %d"
          % (err32, got / err32, (~free).sum() - 65))
    assert np.diff(indptr).tolist() == [64] * 65 and got <= 4 * err32
    assert (P[~free] <= np.float32(tr.EPS)).all()


# ---- 3. gradient and error at a given (P, Y) -----------------------------------------------------------------------------------------------
def given_csr(kind, n, d=6, perplexity=None):
    """the matrix of a gradient or loop case: the reference's, float32 values. Two points always have P = 0.5 both ways, for which
    attraction and repulsion cancel exactly (tests/test_gpu_tsne.py given_p): n = 2 takes an unnormalised 0.3."""
    if n == 2:
        return csr32([0, 1, 2], [1, 0], [0.3, 0.3])
    return csr32(*reference(kind, n, d, perplexity)["a64"][:3])


def check_gradient(label, csr, Y, e, ranges=(0,)):
    """the device's gradient and error at (csr, Y) under every setting of `ranges`, each held by the rule and launched twice"""
    n = len(Y)
    g64, largest, Z = ts.gradient_sparse(*csr, Y, e)
    g32 = ts.gradient_sparse(*csr, Y, e, np.float32)[0]
    kl64 = ts.kl_sparse(*csr, Y, e, Z=Z)
    kl_err32 = 0.0
    for v in range(VARIANTS):
        perm = np.arange(n) if v == 0 else np.random.RandomState(1000 + v).permutation(n)
        kl_err32 = max(kl_err32, abs(ts.kl_sparse(*ts.relabel(*csr, perm), Y[perm], e, np.float32) - kl64))
    err32 = worst(g32, g64, largest[:, None])
    for r in ranges:
        g, kl = hook_gradient(csr, Y, e, r)
        g2, kl2 = hook_gradient(csr, Y, e, r)
        got = worst(g, g64, largest[:, None])
        print("tsne-sparse-error gradient %s e %g ranges %d: err32 %.3g, max |g - g64| / largest term / err32 %.3g; KL %.7g err32 %.3g, |KL - KL64| / err32 %.3g"
              % (label, e, r, err32, got / max(err32, 1e-300), kl64, kl_err32, abs(kl - kl64) / max(kl_err32, 1e-300)))
        assert got <= 4 * err32
        assert abs(kl - kl64) <= 4 * kl_err32
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and kl == kl2      # two launches, the same bits
    return g


@pytest.mark.parametrize("n", (2, 3, 63, 64, 65, 257))
def test_gradient_and_error(n):
    rs = np.random.RandomState(77 + n)
    csr = given_csr("gauss", n)
    base = rs.standard_normal((n, 2))
    for scale in (1e-4, 1.0, 30.0):
        for e in (1.0, 12.0):
            check_gradient("n=%d scale %g" % (n, scale), csr, (base * scale).astype(np.float32), e)


def test_gradient_with_two_points_in_one_place():
    rs = np.random.RandomState(5)
    csr = given_csr("gauss", 65)
    Y = rs.standard_normal((65, 2)).astype(np.float32)
    Y[int(csr[1][0])] = Y[0]      # row 0 and its first stored neighbour coincide: q = 1, no force between them
    g = check_gradient("n=65 coincident", csr, Y, 12.0)
    assert np.isfinite(g).all()


def test_gradient_across_an_lds_tile():
    """n = 4097: the product's layout takes ranges of 512 columns; one forced range walks two tiles, of 4096 columns and of 1"""
    csr = given_csr("gauss", 4097, 6, 10.0)
    Y = (np.random.RandomState(41).standard_normal((4097, 2)) * 20.0).astype(np.float32)
    check_gradient("n=4097", csr, Y, 1.0, ranges=(0, 1))


def test_gradient_with_the_ranges_forced():
    csr = given_csr("gauss", 300)
    Y = (np.random.RandomState(42).standard_normal((300, 2)) * 3.0).astype(np.float32)
    check_gradient("n=300", csr, Y, 12.0, ranges=(1, 2, 5))


@pytest.mark.parametrize("kind,d,perplexity", [("hub", 32, 1.5), ("outlier", 6, None)])
def test_gradient_on_the_hub_and_outlier_matrices(kind, d, perplexity):
    csr = given_csr(kind, 130, d, perplexity)
    Y = (np.random.RandomState(43).standard_normal((130, 2)) * 3.0).astype(np.float32)
    for e in (1.0, 12.0):
        check_gradient("%s n=130" % kind, csr, Y, e)


# ---- 4. the loop and the whole call ----------------------------------------------------------------------------------------------------------
def held(label, n, Y, kl, it, Y64, kl64, it64, runs, want_it):
    scale = np.abs(Y64).max()
    err32, kl_err32 = worst(runs[0][0], Y64, scale), max(abs(k - kl64) for _, k in runs)
    print("tsne-sparse-error %s n=%d: err32 %.3g, max |Y - Y64| / extent / err32 %.3g; KL %.7g err32 %.3g (one run: %.3g), |KL - KL64| / err32 %.3g"
          % (label, n, err32, worst(Y, Y64, scale) / max(err32, 1e-300), kl64, kl_err32, abs(runs[0][1] - kl64), abs(kl - kl64) / max(kl_err32, 1e-300)))
    assert it == it64 == want_it and worst(Y, Y64, scale) <= 4 * err32 and abs(kl - kl64) <= 4 * kl_err32


@pytest.mark.parametrize("n,d", [(5, 6), (65, 36), (130, 300), (300, 16)])
def test_five_iterations_of_the_whole_call(n, d):
    rs = np.random.RandomState(n)
    X = rows_of("gauss", rs, n, d)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    perp = perplexity_of(n)
    Y64, kl64, it64 = ts.tsne_sparse(X, perplexity=perp, max_iter=5, init=Y0)
    runs = float32_runs(lambda perm: ts.tsne_sparse(X[perm], perplexity=perp, max_iter=5, init=Y0[perm], dtype=np.float32)[:2], n)
    m = table_model(X)
    Y, kl, it = m.tsne(perplexity=perp, max_iter=5, init=Y0, method="sparse")
    again = m.tsne(perplexity=perp, max_iter=5, init=Y0, method="sparse")
    named = m.tsne(perplexity=perp, max_iter=5, init=Y0, method="sparse", n_neighbors=ts.default_neighbors(n, perp))
    m.close()
    held("call d=%d" % d, n, Y, kl, it, Y64, kl64, it64, runs, 4)
    for other in (again, named):      # the same call twice, and sklearn's k spelled out: the same bits
        assert np.array_equal(Y.view(np.uint32), other[0].view(np.uint32)) and (kl, it) == other[1:]


@pytest.mark.parametrize("n", (2, 3, 63, 64, 65, 257, 300))
def test_the_phase_boundary_through_the_hook(n):
    rs = np.random.RandomState(500 + n)
    csr = given_csr("gauss", n)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    lr = np.float32(tr.auto_learning_rate(n))
    Y64, kl64, it64 = ts.descent_sparse(*csr, Y0, lr, 12.0, exploration=3, max_iter=5)
    runs = float32_runs(lambda perm: ts.descent_sparse(*ts.relabel(*csr, perm), Y0[perm], lr, 12.0, exploration=3, max_iter=5, dtype=np.float32)[:2], n)
    Y, kl, it = hook_descent(csr, Y0, float(lr), 3, 5)
    held("loop 3+2", n, Y, kl, it, Y64, kl64, it64, runs, 4)


def test_a_run_that_min_grad_norm_ends():
    """min_grad_norm = 1e30 ends each phase at its first check: iterations 49 and 99, from a picture the fp64 reference has already
    run to its end (tests/test_gpu_tsne.py `settled`: from a 1e-4 start a hundred iterations are far into the chaotic regime)"""
    n = 130
    csr = given_csr("gauss", n)
    Y0 = (1e-4 * np.random.RandomState(9).standard_normal((n, 2))).astype(np.float32)
    Y0 = ts.descent_sparse(*csr, Y0, 50.0, 12.0, exploration=250, max_iter=1000)[0].astype(np.float32)
    kw = dict(exploration=250, max_iter=1000, min_grad_norm=1e30)
    Y64, kl64, it64 = ts.descent_sparse(*csr, Y0, 50.0, 1.0, **kw)
    runs = float32_runs(lambda perm: ts.descent_sparse(*ts.relabel(*csr, perm), Y0[perm], np.float32(50.0), 1.0, dtype=np.float32, **kw)[:2], n)
    Y, kl, it = hook_descent(csr, Y0, 50.0, 250, 1000, min_grad_norm=1e30, exaggeration=1.0)
    assert worst(runs[0][0], Y64, np.abs(Y64).max()) < 1e-4, "the run must stay out of the chaotic regime for the rule to say anything"
    held("loop min_grad_norm 50+50", n, Y, kl, it, Y64, kl64, it64, runs, 99)


@pytest.mark.parametrize("method", ["sparse_adam", "dense_adam"])
def test_lazy_tables_are_read_at_their_logical_values_and_training_goes_on_unchanged(method, monkeypatch):
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(num_words=3000, num_entities=500, word_dim=12, entity_dim=36, window=3, num_random=2, nonlinearity="tanh", batch_norm=False,
                update_method=method)
    spec["lambda"] = 0.02
    rs = np.random.RandomState(12)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    a, b = gpu_model(spec, 40), gpu_model(spec, 40)
    for m in (a, b):
        load_params(m, params, True)
    batches = [random_batch(spec, rs, 40, zipf=True) for _ in range(20)]

    def ten(lo):
        for words, ww, labels, iw, ids in batches[lo:lo + 10]:
            for m in (a, b):
                m.step(ca.Batch(words, labels, ww, iw), 2e-2, entity_ids=ids)
    ten(0)
    eids = rs.choice(500, 130, replace=False).astype(np.int64)
    wids = rs.choice(3000, 65, replace=False).astype(np.int64)      # rare words: rows with ten pending factors
    Y0 = (1e-4 * rs.standard_normal((130, 2))).astype(np.float32)
    got_e = a.tsne(ids=eids, max_iter=5, init=Y0, method="sparse")      # straight behind nvsm_step
    got_w = a.tsne(space="words", ids=wids, max_iter=5, init=Y0[:65], perplexity=16.0, method="sparse")
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0 and np.abs(logical[W_NAME] - params[W_NAME]).max() > 0
    for got, X, perp, y0 in ((got_e, logical[E_NAME].reshape(-1, 36)[eids], 30.0, Y0), (got_w, logical[W_NAME].reshape(-1, 12)[wids], 16.0, Y0[:65])):
        Y64, kl64, _ = ts.tsne_sparse(X, perplexity=perp, max_iter=5, init=y0)
        Y32, _, _ = ts.tsne_sparse(X, perplexity=perp, max_iter=5, init=y0, dtype=np.float32)
        scale = np.abs(Y64).max()
        err32 = worst(Y32, Y64, scale)
        print("tsne-sparse-error lazy %s n=%d: err32 %.3g, ratio %.3g" % (method, len(X), err32, worst(got[0], Y64, scale) / err32))
        assert worst(got[0], Y64, scale) <= 4 * err32
    ten(10)
    for n in list(PARAMS) + ADAM_STATE:                       # b never called nvsm_tsne_sparse
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.close()
    b.close()


# ---- 5. past nvsm_tsne's cap -----------------------------------------------------------------------------------------------------------------
def z_fp64(Y, chunk=512):
    """Σ_{i≠j} 1 / (1 + |y_i − y_j|²) in fp64, each pair evaluated once (chunks of rows against the rows behind them)"""
    Y = np.asarray(Y, dtype=np.float64)
    z = 0.0
    for c0 in range(0, len(Y), chunk):
        a = Y[c0:c0 + chunk]
        d2 = ((a[:, None, 0] - Y[None, c0:, 0]) ** 2) + ((a[:, None, 1] - Y[None, c0:, 1]) ** 2)
        q = 1.0 / (1.0 + d2)
        inside = q[:, :len(a)]
        z += 2.0 * (q[:, len(a):].sum() + np.triu(inside, 1).sum())
    return z


def test_one_row_past_the_exact_calls_cap():
    n, d = ca.TSNE_MAX_ROWS + 1, 8
    rs = np.random.RandomState(32769)
    X = rs.standard_normal((n, d)).astype(np.float32)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    m = table_model(X)
    a = m.tsne(max_iter=3, init=Y0, method="sparse")
    b = m.tsne(max_iter=3, init=Y0, method="sparse")
    assert a[2] == 2 and np.isfinite(a[0]).all() and np.isfinite(a[1]) and a[1] > 0
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:] == b[1:]
    o = ca.NvsmTsneOptions()
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    out, kl, it = np.zeros(2 * n, dtype=np.float32), C.c_double(), C.c_int32()
    assert ca.lib().nvsm_tsne(m._h, C.byref(o), ptr(out), C.byref(kl), C.byref(it)) == 2      # NVSM_ERR_UNSUPPORTED, as before
    assert b"32768" in ca.lib().nvsm_last_error()
    m.close()
    # the neighbours of 64 sampled rows against a brute force, and their gradient on the device's own matrix
    k = ts.default_neighbors(n, 30.0)
    sample = np.sort(rs.choice(n, 64, replace=False))
    sample[0], sample[-1] = 0, n - 1
    ids, d2 = hook_knn(X, k)
    neighbour_rule(X, ids[sample], d2[sample], k, rows=sample, label="past the cap")
    indptr, indices, data, _ = hook_affinities(X, 30.0, k)
    assert indptr[n] == len(indices) and abs(data.astype(np.float64).sum() - 1.0) <= 2.0 ** -23
    Y = (rs.standard_normal((n, 2)) * 30.0).astype(np.float32)
    Z = z_fp64(Y)
    g64, largest, _ = ts.gradient_sparse(indptr, indices, data, Y, 12.0, rows=sample, Z=Z)
    g32 = ts.gradient_sparse(indptr, indices, data, Y, 12.0, np.float32, rows=sample, Z=Z)[0]
    g, kl = hook_gradient((indptr, indices, data), Y, 12.0)
    err32, got = worst(g32, g64, largest[:, None]), worst(g[sample], g64, largest[:, None])
    kl64 = ts.kl_sparse(indptr, indices, data, Y, 12.0, Z=Z)
    print("tsne-sparse-error past the cap n=%d nnz %d: gradient of 64 rows err32 %.3g, ratio %.3g; KL %.7g, device %.7g" % (n, len(data), err32, got / err32, kl64, kl))
    assert got <= 4 * err32
    # the error is fp64 throughout, its Z included: what is left is the order of 4·10^6 terms and of 10^9 pairs, and P's float32 sum
    assert abs(kl - kl64) <= 1e-9 * abs(kl64)


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end():
    with open(os.path.join(ROOT, "tests", "golden", "tsne", "sparse_end_to_end.json")) as f:
        gold = json.load(f)
    X, labels = tr.clusters(np.random.RandomState(gold["seed"]), gold["n"], gold["d"], gold["clusters"], gold["spread"])
    m = table_model(X)
    yield gold, X, labels, ts.affinities_nn(X, gold["perplexity"])[:3], m
    m.close()


@pytest.mark.parametrize("init", ["pca", "random"])
def test_end_to_end_lands_in_the_references_band(end_to_end, init):
    gold, X, labels, csr, m = end_to_end
    kls = [r["kl"] for r in gold["runs"]]
    trusts = [r["trustworthiness"] for r in gold["runs"]]
    Y, kl_device, n_iter = m.tsne(perplexity=gold["perplexity"], max_iter=gold["max_iter"], init=init, random_state=0, method="sparse")
    kl, trust = ts.kl_sparse(*csr, Y), tr.trustworthiness(X, Y, gold["n_neighbors"])      # fp64, from the RETURNED embedding
    print("tsne-sparse-error end to end %s: KL %.4f (reference runs %.4f .. %.4f; the device's own %.4f), trustworthiness %.4f (%.4f .. %.4f), n_iter %d"
          % (init, kl, min(kls), max(kls), kl_device, trust, min(trusts), max(trusts), n_iter))
    assert kl <= max(kls) + (max(kls) - min(kls))
    assert trust >= min(trusts) - (max(trusts) - min(trusts))
    assert tr.nearest_label_agreement(Y, labels) == 1.0
    assert n_iter == gold["max_iter"] - 1 and abs(kl_device - kl) <= 1e-3


def test_refusals_of_the_sparse_call_and_its_profiler_names(end_to_end):
    gold, X, labels, csr, m = end_to_end

    def raw(n_neighbors, **fields):
        o, sp = ca.NvsmTsneOptions(), ca.NvsmTsneSparseOptions()
        ca.lib().nvsm_tsne_options_default(C.byref(o))
        for key, v in fields.items():
            setattr(o, key, v)
        sp.n_neighbors = n_neighbors
        out = np.full(600, GUARD, dtype=np.float32)
        kl, it = C.c_double(-5.0), C.c_int32(-5)
        st = ca.lib().nvsm_tsne_sparse(m._h, C.byref(o), C.byref(sp), ptr(out), C.byref(kl), C.byref(it))
        return st, ca.lib().nvsm_last_error(), (out == GUARD).all() and kl.value == -5.0 and it.value == -5
    for k, fields, status, word in ((-1, {}, 1, b"n_neighbors"), (300, {}, 1, b"n_neighbors"), (1025, {}, 1, b"n_neighbors"),
                                    (5, dict(num_rows=5, perplexity=2.0), 1, b"n_neighbors"), (0, dict(perplexity=float("nan")), 1, b"perplexity"),
                                    (-1, dict(max_iter=0), 1, b"max_iter"), (0, dict(space=ca.SPACE_PROJECTED_WORDS), 1, b"space")):
        st, msg, untouched = raw(k, **fields)
        assert st == status and word in msg and untouched, (k, fields, st, msg)
    big = table_model(np.zeros((1100, 1), dtype=np.float32))      # sklearn's k for this perplexity is 1099: above the cap
    o = ca.NvsmTsneOptions()
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    o.perplexity = 400.0
    out, kl, it = np.zeros(2200, dtype=np.float32), C.c_double(), C.c_int32()
    assert ca.lib().nvsm_tsne_sparse(big._h, C.byref(o), None, ptr(out), C.byref(kl), C.byref(it)) == 2 and b"neighbours" in ca.lib().nvsm_last_error()
    big.close()
    m.profile_enable(True)
    m.profile_reset()
    Y, kl, it = m.tsne(limit=64, max_iter=50, perplexity=10.0, method="sparse", n_neighbors=12)
    names = {n for n in m.profile() if n.startswith("tsne_")}
    m.profile_enable(False)
    assert np.isfinite(Y).all() and it == 49
    assert names == {"tsne_rows", "tsne_nn_scan", "tsne_conditionals", "tsne_symmetrize", "tsne_pca", "tsne_forces", "tsne_update", "tsne_kl"}, names
