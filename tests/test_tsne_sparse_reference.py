"""tests/tsne_sparse_reference.py, the restatement the GPU tests of nvsm_tsne_sparse are held to, against scikit-learn itself (1.7)
on the CPU: sklearn.manifold.TSNE's method='barnes_hut' at angle = 0, where the tree summarises nothing.

Neighbour sets against NearestNeighbors: sklearn ranks by sqrt of an expanded float64 distance, the reference by a float32-rounded
direct sum, so a row whose k-th and (k+1)-th distances are closer than 1e-5 of the k-th may pick the other one; such rows are left
out, at most 5 % of a case's rows.
_joint_probabilities_nn, and _kl_divergence_bh(angle=0.0) (gradient and error) at a given (P, Y), and five iterations of
_gradient_descent over it: sklearn's gradient path is float32, so the rule is the project's — |sklearn − ref64| <= 4·|ref32 − ref64|
per case and per quantity; the ratios are printed. An error is ONE number, whose deviation in one float32 run is a single draw: its
err32 is the largest over VARIANTS relabelled float32 runs (tests/test_gpu_tsne.py float32_runs), each adding the terms one after the
other in a float32 accumulator as _barnes_hut_tsne.pyx's `float C` does (numpy's pairwise float32 sum is ten times closer to fp64 than
any plain float32 loop, sklearn's included: 1.6e-7 against sklearn's 3.5e-6 at n = 65).
With k = n − 1 the sparse matrix is the exact path's wherever that one does not clamp a cell to eps."""
import numpy as np
import pytest

from tests import tsne_reference as tr
from tests import tsne_sparse_reference as ts

sklearn = pytest.importorskip("sklearn")
from scipy.sparse import csr_matrix  # noqa: E402
from sklearn.manifold import _t_sne  # noqa: E402
from sklearn.neighbors import NearestNeighbors  # noqa: E402

CASES = [(3, 6, 1.5), (65, 16, 5.0), (130, 300, 20.0), (300, 16, 30.0), (1000, 32, 30.0), (2049, 64, 30.0)]
VARIANTS = 6
_CASE = {}


def case(n, d, perplexity):
    """the rows, their fp64 and float32 affinities and a spread-out picture, computed once and shared"""
    key = (n, d, perplexity)
    if key not in _CASE:
        rs = np.random.default_rng(n * 1000 + d)
        X = rs.standard_normal((n, d)).astype(np.float32)
        k = ts.default_neighbors(n, perplexity)
        a64 = ts.affinities_nn(X, perplexity, k)
        a32 = ts.affinities_nn(X, perplexity, k, np.float32)
        _CASE[key] = dict(X=X, k=k, a64=a64, a32=a32, Y=(rs.standard_normal((n, 2)) * 3.0).astype(np.float32))
    return _CASE[key]


def worst(got, want, scale):
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / scale).max())


@pytest.mark.parametrize("n,d,perplexity", CASES)
def test_neighbour_sets_match_sklearns_nearest_neighbors(n, d, perplexity):
    c = case(n, d, perplexity)
    X, k = c["X"], c["k"]
    ids = c["a64"][3]
    assert k == min(n - 1, int(3.0 * perplexity + 1))
    assert not (ids == np.arange(n)[:, None]).any(), "a row is never its own neighbour"
    G = NearestNeighbors(n_neighbors=k).fit(X).kneighbors_graph(mode="distance")
    G.sort_indices()
    theirs = G.indices.reshape(n, k)
    # reference distances to every row, for the band: k-th and (k+1)-th nearest
    D = tr.sq_distances(X).astype(np.float64)
    np.fill_diagonal(D, np.inf)
    D.sort(axis=1)
    close = np.zeros(n, dtype=bool) if k == n - 1 else (np.sqrt(D[:, k]) - np.sqrt(D[:, k - 1]) < 1e-5 * np.sqrt(D[:, k - 1]))
    same = np.array([np.array_equal(np.sort(ids[i]), theirs[i]) for i in range(n)])
    print("tsne-sparse-reference neighbours n=%d d=%d k=%d: %.2f %% of rows in the band, %d rows differ (all inside it: %s)"
          % (n, d, k, 100.0 * close.mean(), (~same).sum(), bool(same[~close].all())))
    assert close.mean() <= 0.05
    assert same[~close].all()


@pytest.mark.parametrize("n,d,perplexity", CASES)
def test_joint_probabilities_match_sklearn(n, d, perplexity):
    c = case(n, d, perplexity)
    indptr, indices, data, ids, d2 = c["a64"][:5]
    k = c["k"]
    order = np.argsort(ids, axis=1)
    dist = csr_matrix((np.take_along_axis(d2, order, 1).ravel().astype(np.float64), np.take_along_axis(ids, order, 1).ravel(),
                       np.arange(0, n * k + 1, k)), shape=(n, n))
    theirs = _t_sne._joint_probabilities_nn(dist, perplexity, 0)
    theirs.sort_indices()
    assert np.array_equal(theirs.indptr, indptr) and np.array_equal(theirs.indices, indices)
    assert (np.diff(indices)[np.diff(ts._entry_rows(indptr)) == 0] > 0).all(), "columns ascend strictly inside a row"
    assert not (indices == ts._entry_rows(indptr)).any()
    P = ts.densify(indptr, indices, data) if n <= 1000 else None
    if P is not None:
        assert np.array_equal(P, P.T)
    i32 = c["a32"]
    if np.array_equal(i32[0], indptr) and np.array_equal(i32[1], indices):
        err32 = worst(i32[2], data, data)
    else:      # the float32 chain picked another neighbour somewhere: compare where both store a cell
        A, B = csr_matrix((data, indices, indptr), shape=(n, n)), csr_matrix((i32[2].astype(np.float64), i32[1], i32[0]), shape=(n, n))
        both = A.multiply(B.astype(bool)).tocsr()
        other = B.multiply(A.astype(bool)).tocsr()
        both.sort_indices(); other.sort_indices()
        err32 = worst(other.data, both.data, both.data)
    got = worst(theirs.data, data, data)
    print("tsne-sparse-reference joint n=%d d=%d: err32 %.3g, sklearn's deviation / err32 %.3g, ΣP − 1 = %.3g"
          % (n, d, err32, got / max(err32, 1e-300), data.sum() - 1.0))
    assert got <= 4 * err32
    assert abs(data.sum() - 1.0) <= 1e-12


def bh(P_csr, Y, n):
    kl, grad = _t_sne._kl_divergence_bh(np.asarray(Y, dtype=np.float64).ravel().copy(), P_csr, 1.0, n, 2, angle=0.0)
    return kl, grad.reshape(n, 2)


@pytest.mark.parametrize("n,d,perplexity", CASES)
def test_gradient_and_error_match_sklearns_barnes_hut_at_angle_zero(n, d, perplexity):
    c = case(n, d, perplexity)
    indptr, indices, data = c["a64"][:3]
    data = data.astype(np.float32)
    for e in (1.0, 12.0):
        Y = c["Y"]
        g64, largest, Z = ts.gradient_sparse(indptr, indices, data, Y, e)
        g32 = ts.gradient_sparse(indptr, indices, data, Y, e, np.float32)[0]
        kl64 = ts.kl_sparse(indptr, indices, data, Y, e, Z=Z)
        kl_err32 = 0.0
        for v in range(VARIANTS):
            perm = np.arange(n) if v == 0 else np.random.RandomState(1000 + v).permutation(n)
            ip, ix, dt = ts.relabel(indptr, indices, data, perm)
            kl_err32 = max(kl_err32, abs(ts.kl_sparse(ip, ix, dt, Y[perm], e, np.float32, sequential=True) - kl64))
        kl, g = bh(csr_matrix((data * np.float32(e), indices, indptr), shape=(n, n)), Y, n)
        err32, got = worst(g32, g64, largest[:, None]), worst(g, g64, largest[:, None])
        print("tsne-sparse-reference gradient n=%d e %g: err32 %.3g, sklearn's deviation / err32 %.3g (%.3g of the largest entry); "
              "error %.7g err32 %.3g, sklearn's deviation / err32 %.3g"
              % (n, e, err32, got / max(err32, 1e-300), np.abs(g - g64).max() / np.abs(g64).max(), kl64, kl_err32,
                 abs(kl - kl64) / max(kl_err32, 1e-300)))
        assert got <= 4 * err32
        assert abs(kl - kl64) <= 4 * kl_err32


@pytest.mark.parametrize("n,d,perplexity", CASES[:5])
def test_five_iterations_match_sklearns_gradient_descent(n, d, perplexity):
    c = case(n, d, perplexity)
    indptr, indices, data = c["a64"][:3]
    data = data.astype(np.float32)
    Y0 = (1e-4 * np.random.default_rng(n).standard_normal((n, 2))).astype(np.float32)
    lr = np.float32(tr.auto_learning_rate(n))
    P12 = csr_matrix((data * np.float32(12.0), indices, indptr), shape=(n, n))
    p, err, it = _t_sne._gradient_descent(_t_sne._kl_divergence_bh, Y0.astype(np.float64).ravel(), it=0, max_iter=5, n_iter_check=50,
                                          momentum=0.5, learning_rate=float(lr), n_iter_without_progress=250, args=[P12, 1.0, n, 2],
                                          kwargs=dict(angle=0.0))
    Y64, kl64, it64 = ts.descent_sparse(indptr, indices, data, Y0, lr, 12.0, exploration=5, max_iter=5)
    Y32, kl32 = None, 0.0
    for v in range(VARIANTS):
        perm = np.arange(n) if v == 0 else np.random.RandomState(1000 + v).permutation(n)
        ip, ix, dt = ts.relabel(indptr, indices, data, perm)
        Yv, klv, _ = ts.descent_sparse(ip, ix, dt, Y0[perm], lr, 12.0, exploration=5, max_iter=5, dtype=np.float32, sequential=True)
        Y32 = Yv if v == 0 else Y32
        kl32 = max(kl32, abs(klv - kl64))
    scale = np.abs(Y64).max()
    err32, got = worst(Y32, Y64, scale), worst(p.reshape(n, 2), Y64, scale)
    print("tsne-sparse-reference five iterations n=%d: err32 %.3g, sklearn's deviation / err32 %.3g; error %.7g err32 %.3g, sklearn's / err32 %.3g"
          % (n, err32, got / max(err32, 1e-300), kl64, kl32, abs(err - kl64) / max(kl32, 1e-300)))
    assert it == it64 == 4
    assert got <= 4 * err32
    assert abs(err - kl64) <= 4 * kl32


@pytest.mark.parametrize("n,d,perplexity", [(3, 6, 1.5), (65, 16, 5.0), (130, 300, 20.0)])
def test_with_every_other_row_a_neighbour_the_matrix_is_the_exact_paths(n, d, perplexity):
    X = case(n, d, perplexity)["X"]
    indptr, indices, data = ts.affinities_nn(X, perplexity, n - 1)[:3]
    dense = tr.affinities(X, perplexity)[0]
    P = ts.densify(indptr, indices, data)
    clamped = dense <= tr.EPS      # cells the exact path lifts to eps (and its diagonal)
    assert np.diff(indptr).tolist() == [n - 1] * n
    assert np.abs(P - dense)[~clamped].max() <= 1e-12 * dense.max()
    assert (P[clamped] <= tr.EPS).all()
