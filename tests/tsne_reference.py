"""numpy restatement of exact t-SNE as nvsm_tsne defines it (include/cunvsm_amd.h; scikit-learn 1.7's TSNE(method='exact')): squared
distances, _binary_search_perplexity, _joint_probabilities, the exact gradient and KL of _kl_divergence, _gradient_descent in its two
phases with the stopping rules, the PCA start, and trustworthiness. Every function takes the arithmetic as `dtype`: np.float64 is the
reference of the GPU tests, np.float32 the "float32 numpy chain" whose deviation from it (err32) sets their tolerance — the rule of
tests/test_gpu_rank.py: the device must stay within 4·err32, and neither figure is ever taken from the device.
tests/test_tsne_reference.py holds the fp64 functions to scikit-learn itself."""
import numpy as np

EPS = 2.220446049250313e-16      # sklearn's MACHINE_EPSILON
N_ITER_CHECK = 50
EXPLORATION_PROGRESS = 250


def l2_normalize(X, dtype=np.float64):
    """rows divided by their norms, a zero row kept; float32 out (what the table gather hands on)"""
    X = np.asarray(X, dtype=dtype)
    norm = np.sqrt((X * X).sum(axis=1, dtype=dtype))
    inv = np.where(norm > 0, dtype(1) / np.where(norm > 0, norm, dtype(1)), dtype(0)).astype(dtype)
    return (X * inv[:, None]).astype(np.float32)


def sq_distances(X, dtype=np.float64):
    """D[i][j] = Σ_t (x_it − x_jt)² in `dtype`, rounded to float32 (sklearn hands float32 to the perplexity search)"""
    X = np.asarray(X, dtype=dtype)
    D = np.empty((X.shape[0], X.shape[0]), dtype=dtype)
    for i in range(X.shape[0]):
        df = X[i][None, :] - X
        D[i] = (df * df).sum(axis=1, dtype=dtype)
    return D.astype(np.float32)


def conditionals(D, perplexity, dtype=np.float64):
    """sklearn.manifold._utils._binary_search_perplexity on the full matrix: (C [n][n] in `dtype` with a zero diagonal, steps [n]);
    steps[i] = evaluations row i took (at most 100)"""
    D = np.asarray(D, dtype=dtype)
    n = D.shape[0]
    target = dtype(np.log(np.float64(np.float32(perplexity))))
    C = np.zeros((n, n), dtype=dtype)
    steps = np.zeros(n, dtype=np.int64)
    for i in range(n):
        d = np.delete(D[i], i)
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
        C[i] = np.insert(p, i, dtype(0))
    return C, steps


def joint(C, dtype=np.float64):
    """sklearn's _joint_probabilities behind the search: max((C + Cᵀ) / max(Σ, eps), eps), zero diagonal"""
    C = np.asarray(C, dtype=dtype)
    P = C + C.T
    P = np.maximum(P / np.maximum(P.sum(dtype=dtype), dtype(EPS)), dtype(EPS)).astype(dtype)
    np.fill_diagonal(P, 0)
    return P


def affinities(X, perplexity, dtype=np.float64):
    """X -> (P, C as stored: float32, steps): the conditionals are rounded to float32 before they are symmetrised, as the device stores them"""
    C, steps = conditionals(sq_distances(X, dtype), perplexity, dtype)
    C = C.astype(np.float32)
    return joint(C, dtype), C, steps


def row_entropy(D_row, C_row, i):
    """log(perplexity) that a stored row of conditionals realises, recovered without its beta: for p_j = exp(−β d_j) / Σ, H = log Σ + β
    Σ d_j p_j = −Σ p_j log p_j over the p_j > 0 (fp64)"""
    p = np.delete(np.asarray(C_row, dtype=np.float64), i)
    p = p[p > 0]
    p = p / p.sum()
    return float(-(p * np.log(p)).sum())


def _pairs(Y, dtype):
    Y = np.asarray(Y, dtype=dtype)
    dy = Y[:, None, :] - Y[None, :, :]
    q = dtype(1) / (dtype(1) + (dy * dy).sum(axis=2, dtype=dtype))
    np.fill_diagonal(q, 0)
    return dy, q.astype(dtype)


def gradient(P, Y, exaggeration=1.0, dtype=np.float64, factor=4.0):
    """(g [n][2], largest |term| per row): g_i = 4·(e·Σ_j P_ij q_ij (y_i − y_j) − (1/Z)·Σ_j q_ij² (y_i − y_j)), Z = Σ_{i≠j} q_ij.
    `factor` is the 4 (a test of the tests drops it)."""
    P = np.asarray(P, dtype=dtype)
    dy, q = _pairs(Y, dtype)
    Z = q.sum(dtype=dtype)
    att = (dtype(exaggeration) * P * q)[:, :, None] * dy
    rep = (q * q / Z)[:, :, None] * dy
    g = dtype(factor) * (att.sum(axis=1, dtype=dtype) - rep.sum(axis=1, dtype=dtype))
    largest = dtype(factor) * np.maximum(np.abs(att).max(axis=(1, 2)), np.abs(rep).max(axis=(1, 2)))
    return g.astype(dtype), largest.astype(np.float64)


def kl_divergence(P, Y, exaggeration=1.0, dtype=np.float64):
    """Σ_{i≠j} e·P_ij · log(max(e·P_ij, eps) / max(q_ij / Z, eps))"""
    P = dtype(exaggeration) * np.asarray(P, dtype=dtype)
    _, q = _pairs(Y, dtype)
    Q = np.maximum(q / q.sum(dtype=dtype), dtype(EPS))
    t = P * np.log(np.maximum(P, dtype(EPS)) / Q)
    np.fill_diagonal(t, 0)
    return float(t.sum(dtype=dtype))


def descent(P, Y0, learning_rate, early_exaggeration=12.0, exploration=250, max_iter=1000, n_iter_without_progress=300,
            min_grad_norm=1e-7, dtype=np.float64, leave_exaggeration_on=False, details=None):
    """sklearn's _gradient_descent twice (TSNE._tsne): (Y, kl_divergence, n_iter). Gains, update and the best error start afresh in
    the second phase; where it has no iteration left the first phase's figures stand. `details` (a dict) receives Y_eval and
    exaggeration_eval: where the returned error was evaluated."""
    Y = np.array(Y0, dtype=dtype)
    state = {"error": np.finfo(np.float64).max}

    def phase(Y, it0, last, momentum, exaggeration, without_progress):
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best_error, best_iter, i = np.finfo(np.float64).max, it0, it0 - 1
        for i in range(it0, last):
            check = (i + 1) % N_ITER_CHECK == 0
            if check or i == last - 1:
                state["error"] = kl_divergence(P, Y, exaggeration, dtype)
                state["Y_eval"], state["exaggeration_eval"] = Y.copy(), exaggeration
            g, _ = gradient(P, Y, exaggeration, dtype)
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
        Y, it = phase(Y, it + 1, max_iter, 0.8, early_exaggeration if leave_exaggeration_on else 1.0, n_iter_without_progress)
    if details is not None:
        details.update(state)
    return Y, state["error"], it


def pca_start(X, dtype=np.float64):
    """(Y0 [n][2], the eigenvalues descending): the centred rows on their two leading principal axes (eigh of XcᵀXc), each axis' sign
    by its entry of largest magnitude (the lower index on a tie), scaled to np.std(Y0[:, 0]) = 1e-4"""
    X = np.asarray(X, dtype=dtype)
    Xc = X - X.mean(axis=0, dtype=dtype)
    w, v = np.linalg.eigh((Xc.T @ Xc).astype(dtype))
    order = np.argsort(-w, kind="stable")
    V = np.zeros((2, X.shape[1]), dtype=dtype)
    for c in range(min(2, X.shape[1])):
        a = v[:, order[c]]
        V[c] = -a if a[np.argmax(np.abs(a))] < 0 else a
    Y0 = (Xc @ V.T).astype(dtype)
    sd = Y0[:, 0].std(dtype=dtype)
    if not sd > 0:
        raise ValueError("the rows have no spread along their first principal axis")
    return (Y0 / sd * dtype(1e-4)).astype(dtype), w[order].astype(np.float64)


def _with(details, **more):
    if details is not None:
        details.update(more)
    return details


def auto_learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300,
         min_grad_norm=1e-7, init="pca", dtype=np.float64, exploration=None, details=None):
    """the whole chain on rows X: (Y, kl_divergence, n_iter); details as descent's, and P"""
    P, _, _ = affinities(X, perplexity, dtype)
    Y0 = pca_start(np.asarray(X, dtype=np.float32), dtype)[0].astype(np.float32) if isinstance(init, str) else np.asarray(init, dtype=np.float32)
    lr = auto_learning_rate(len(X), early_exaggeration) if learning_rate == "auto" else learning_rate
    return descent(P.astype(np.float32), Y0, np.float32(lr), early_exaggeration, min(250, max_iter) if exploration is None else exploration,
                   max_iter, n_iter_without_progress, min_grad_norm, dtype, details=_with(details, P=P))


def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness (Euclidean): 1 − 2 / (n k (2n − 3k − 1)) · Σ_i Σ_{j in the k nearest of i in Y} max(0, r_X(i, j) − k)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, k = X.shape[0], n_neighbors
    dX = sq_distances(X).astype(np.float64)
    np.fill_diagonal(dX, np.inf)
    dY = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dY, np.inf)
    ind_X = np.argsort(dX, axis=1, kind="stable")
    ind_Y = np.argsort(dY, axis=1, kind="stable")[:, :k]
    rank = np.empty((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], ind_X] = np.arange(1, n + 1)[None, :]
    excess = rank[np.arange(n)[:, None], ind_Y] - k
    return float(1.0 - excess[excess > 0].sum() * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))))


def nearest_label_agreement(Y, labels):
    """the share of points whose nearest neighbour in the picture carries their own label"""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    labels = np.asarray(labels)
    return float((labels[d.argmin(axis=1)] == labels).mean())


def clusters(rs, n=300, d=16, k=3, spread=0.25):
    """the end-to-end inputs: k Gaussian clusters with centres N(0, 1) and the given spread, float32 rows and their labels"""
    centres = rs.standard_normal((k, d))
    labels = np.arange(n) % k
    return (centres[labels] + spread * rs.standard_normal((n, d))).astype(np.float32), labels
