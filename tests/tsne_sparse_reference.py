"""numpy restatement of sparse-affinity t-SNE as nvsm_tsne_sparse defines it (include/cunvsm_amd.h; scikit-learn 1.7's
TSNE(method='barnes_hut', angle=0)): the k nearest other rows by (float32 distance, row id), _binary_search_perplexity over a row's k
distances, _joint_probabilities_nn as CSR arrays, the gradient and error of _kl_divergence_bh at angle 0 — attraction over the stored
entries, repulsion over all pairs — and the two-phase descent. Every function takes the arithmetic as `dtype`, as
tests/tsne_reference.py does and for the same purpose: np.float64 is the reference of the GPU tests, np.float32 the chain whose
deviation from it (err32) sets their tolerance. tests/test_tsne_sparse_reference.py holds the fp64 functions to scikit-learn."""
import numpy as np

from tests.tsne_reference import EPS, EXPLORATION_PROGRESS, N_ITER_CHECK

TINY = float(np.finfo(np.float32).tiny)      # _barnes_hut_tsne.pyx FLOAT32_TINY


def default_neighbors(n, perplexity):
    """TSNE._fit: min(n_samples − 1, int(3 · perplexity + 1))"""
    return min(n - 1, int(3.0 * float(np.float32(perplexity)) + 1.0))


def knn(X, k, dtype=np.float64, rows=None):
    """(ids [m][k] int64, d2 [m][k] float32) of the rows `rows` (None: all): the k OTHER rows of smallest squared distance — the sum in
    `dtype`, rounded to float32 — nearest first, ties by ascending row id. A duplicate of a row is its neighbour at distance 0; the row
    itself never is."""
    X = np.asarray(X, dtype=dtype)
    n = X.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    ids = np.empty((len(rows), k), dtype=np.int64)
    d2 = np.empty((len(rows), k), dtype=np.float32)
    every = np.arange(n)
    for r, i in enumerate(rows):
        df = X[i][None, :] - X
        d = (df * df).sum(axis=1, dtype=dtype).astype(np.float32)
        order = np.lexsort((every, d))           # by distance, then by id
        order = order[order != i][:k]
        ids[r], d2[r] = order, d[order]
    return ids, d2


def conditionals_nn(d2, perplexity, dtype=np.float64):
    """sklearn.manifold._utils._binary_search_perplexity over rows of k distances: (C [n][k] in `dtype`, steps [n])"""
    D = np.asarray(d2, dtype=dtype)
    n, k = D.shape
    target = dtype(np.log(np.float64(np.float32(perplexity))))
    C = np.zeros((n, k), dtype=dtype)
    steps = np.zeros(n, dtype=np.int64)
    for i in range(n):
        d = D[i]
        beta, lo, hi = dtype(1), dtype(-np.inf), dtype(np.inf)
        for step in range(100):
            p = np.exp(-d * beta)
            s = p.sum(dtype=dtype)
            if s == 0:
                s = dtype(1e-8)
            p = p / s
            h = dtype(np.log(s) + beta * (d * p).sum(dtype=dtype))
            diff = dtype(h - target)
            steps[i] = step + 1
            if abs(diff) <= dtype(1e-5):
                break
            if diff > 0:
                lo = beta
                beta = dtype(beta * dtype(2)) if hi == np.inf else dtype((beta + hi) / dtype(2))
            else:
                hi = beta
                beta = dtype(beta / dtype(2)) if lo == -np.inf else dtype((beta + lo) / dtype(2))
        C[i] = p
    return C, steps


def joint_nn(ids, C, dtype=np.float64):
    """_joint_probabilities_nn behind the search: (indptr [n + 1] int64, indices [nnz] int32, data [nnz] in `dtype`) of
    P = (C + Cᵀ) / max(ΣC + ΣCᵀ, eps) over the union of both directions of every edge; columns ascending, no clamp per cell"""
    ids = np.asarray(ids, dtype=np.int64)
    C = np.asarray(C, dtype=dtype)
    n, k = ids.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = ids.ravel()
    key = np.concatenate([rows * n + cols, cols * n + rows])
    val = np.concatenate([C.ravel(), C.ravel()])
    cells, inverse = np.unique(key, return_inverse=True)
    data = np.zeros(len(cells), dtype=dtype)
    np.add.at(data, inverse, val)          # at most two terms a cell: the sum does not depend on their order
    total = dtype(2) * C.sum(dtype=dtype)
    data = (data / np.maximum(total, dtype(EPS))).astype(dtype)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cells // n, minlength=n), out=indptr[1:])
    return indptr, (cells % n).astype(np.int32), data


def affinities_nn(X, perplexity, k=None, dtype=np.float64):
    """X -> (indptr, indices, data, ids, d2, C as stored: float32, steps); the conditionals are rounded to float32 before they are
    symmetrised, as the device stores them"""
    k = default_neighbors(len(X), perplexity) if k is None else k
    ids, d2 = knn(X, k, dtype)
    C, steps = conditionals_nn(d2, perplexity, dtype)
    C = C.astype(np.float32)
    return joint_nn(ids, C, dtype) + (ids, d2, C, steps)


def densify(indptr, indices, data, dtype=np.float64):
    n = len(indptr) - 1
    P = np.zeros((n, n), dtype=dtype)
    P[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    return P


def _entry_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def relabel(indptr, indices, data, perm):
    """the CSR matrix with its points relabelled: row r of the result is row perm[r] of the input, and the columns likewise (the
    picture that goes with it is Y[perm]). Nothing changes but the order in which float32 sums run."""
    n = len(indptr) - 1
    new = np.argsort(perm)
    r, c = new[_entry_rows(indptr)], new[np.asarray(indices)]
    order = np.lexsort((c, r))
    out = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=out[1:])
    return out, c[order].astype(np.int32), np.asarray(data)[order]


def row_entropy_nn(C_row):
    """the entropy a stored row of k conditionals realises, in fp64: −Σ p log p over the p > 0 (tsne_reference.row_entropy without a
    diagonal to drop)"""
    p = np.asarray(C_row, dtype=np.float64)
    p = p[p > 0]
    p = p / p.sum()
    return float(-(p * np.log(p)).sum())


def repulsion(Y, dtype=np.float64, rows=None, chunk=256):
    """(Σ_{j≠i} q_ij² (y_i − y_j) [m][2], Σ_{j≠i} q_ij [m], largest |q² (y_i − y_j)| [m]) for the rows `rows` (None: all), every pair"""
    Y = np.asarray(Y, dtype=dtype)
    rows = np.arange(len(Y)) if rows is None else np.asarray(rows)
    rep = np.zeros((len(rows), 2), dtype=dtype)
    qsum = np.zeros(len(rows), dtype=dtype)
    largest = np.zeros(len(rows), dtype=np.float64)
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        dy = Y[r][:, None, :] - Y[None, :, :]
        q = (dtype(1) / (dtype(1) + (dy * dy).sum(axis=2, dtype=dtype))).astype(dtype)
        q[np.arange(len(r)), r] = 0
        t = (q * q)[:, :, None] * dy
        rep[c0:c0 + chunk] = t.sum(axis=1, dtype=dtype)
        qsum[c0:c0 + chunk] = q.sum(axis=1, dtype=dtype)
        largest[c0:c0 + chunk] = np.abs(t).max(axis=(1, 2))
    return rep, qsum, largest


def gradient_sparse(indptr, indices, data, Y, exaggeration=1.0, dtype=np.float64, rows=None, Z=None):
    """(g [m][2], largest |term| per row, Z): g_i = 4·(e·Σ_{j stored} P_ij q_ij (y_i − y_j) − Σ_{j≠i} q_ij² (y_i − y_j) / Z), Z = Σ_{i≠j}
    q_ij over all pairs. rows: only those rows (then Z must be given: it is a sum over every row)."""
    Y = np.asarray(Y, dtype=dtype)
    n = len(Y)
    er = _entry_rows(indptr)
    dy = Y[er] - Y[indices]
    q = dtype(1) / (dtype(1) + (dy * dy).sum(axis=1, dtype=dtype))
    t = (dtype(exaggeration) * np.asarray(data, dtype=dtype) * q)[:, None] * dy
    att = np.zeros((n, 2), dtype=dtype)
    np.add.at(att, er, t)
    big_att = np.zeros(n, dtype=np.float64)
    np.maximum.at(big_att, er, np.abs(t).max(axis=1))
    rep, qsum, big_rep = repulsion(Y, dtype, rows)
    if Z is None:
        assert rows is None
        Z = qsum.sum(dtype=dtype)
    Z = dtype(Z)
    sel = slice(None) if rows is None else np.asarray(rows)
    g = dtype(4) * (att[sel] - rep / Z)
    largest = 4.0 * np.maximum(big_att[sel], big_rep / np.float64(Z))
    return g.astype(dtype), largest, Z


def kl_sparse(indptr, indices, data, Y, exaggeration=1.0, dtype=np.float64, Z=None, sequential=False):
    """Σ_{stored} e·P_ij · log(max(e·P_ij, tiny) / max(q_ij / Z, tiny)), tiny = np.finfo(np.float32).tiny. sequential: the terms are added
    one after the other in `dtype`, as _barnes_hut_tsne.pyx's `float C` accumulates them, instead of by numpy's pairwise sum"""
    Y = np.asarray(Y, dtype=dtype)
    if Z is None:
        Z = repulsion(Y, dtype)[1].sum(dtype=dtype)
    er = _entry_rows(indptr)
    dy = Y[er] - Y[indices]
    q = dtype(1) / (dtype(1) + (dy * dy).sum(axis=1, dtype=dtype))
    p = dtype(exaggeration) * np.asarray(data, dtype=dtype)
    t = p * np.log(np.maximum(p, dtype(TINY)) / np.maximum(q / dtype(Z), dtype(TINY)))
    return float(np.cumsum(t, dtype=dtype)[-1] if sequential else t.sum(dtype=dtype))


def descent_sparse(indptr, indices, data, Y0, learning_rate, early_exaggeration=12.0, exploration=250, max_iter=1000,
                   n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64, details=None, sequential=False):
    """tests/tsne_reference.py descent's loop — sklearn's _gradient_descent twice — over gradient_sparse and kl_sparse (that loop calls
    the dense functions by name, so it is restated here): (Y, kl_divergence, n_iter)"""
    Y = np.array(Y0, dtype=dtype)
    state = {"error": np.finfo(np.float64).max}

    def phase(Y, it0, last, momentum, exaggeration, without_progress):
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best_error, best_iter, i = np.finfo(np.float64).max, it0, it0 - 1
        for i in range(it0, last):
            check = (i + 1) % N_ITER_CHECK == 0
            g, _, Z = gradient_sparse(indptr, indices, data, Y, exaggeration, dtype)
            if check or i == last - 1:
                state["error"] = kl_sparse(indptr, indices, data, Y, exaggeration, dtype, Z, sequential)
                state["Y_eval"], state["exaggeration_eval"] = Y.copy(), exaggeration
            inc = update * g < 0
            gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8)).astype(dtype)
            gains = np.maximum(gains, dtype(0.01))
            g = g * gains
            update = (dtype(momentum) * update - dtype(learning_rate) * g).astype(dtype)
            Y = (Y + update).astype(dtype)
            if check:
                if state["error"] < best_error:
                    best_error, best_iter = state["error"], i
                elif i - best_iter > without_progress:
                    break
                if np.sqrt((g.astype(np.float64) ** 2).sum()) <= min_grad_norm:
                    break
        return Y, i

    Y, it = phase(Y, 0, exploration, 0.5, early_exaggeration, EXPLORATION_PROGRESS)
    if it + 1 < max_iter:
        Y, it = phase(Y, it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    if details is not None:
        details.update(state)
    return Y, state["error"], it


def tsne_sparse(X, perplexity=30.0, k=None, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300,
                min_grad_norm=1e-7, init=None, dtype=np.float64, exploration=None, details=None):
    """the whole chain on rows X from the start `init` [n][2]: (Y, kl_divergence, n_iter)"""
    from tests.tsne_reference import auto_learning_rate, pca_start
    indptr, indices, data = affinities_nn(X, perplexity, k, dtype)[:3]
    Y0 = pca_start(np.asarray(X, dtype=np.float32), dtype)[0].astype(np.float32) if init is None else np.asarray(init, dtype=np.float32)
    lr = auto_learning_rate(len(X), early_exaggeration) if learning_rate == "auto" else learning_rate
    if details is not None:
        details.update(csr=(indptr, indices, data))
    return descent_sparse(indptr, indices, data.astype(np.float32), Y0, np.float32(lr), early_exaggeration,
                          min(250, max_iter) if exploration is None else exploration, max_iter, n_iter_without_progress, min_grad_norm, dtype,
                          details=details)
