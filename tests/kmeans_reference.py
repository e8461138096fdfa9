"""fp64 numpy restatement of nvsm_kmeans (include/cunvsm_amd.h): Lloyd's algorithm as sklearn.cluster.KMeans(algorithm='lloyd',
n_init=1) runs it, with the rules the header adds where sklearn leaves them open — the relocation of empty clusters and the
one-candidate k-means++ draw. tests/test_kmeans_reference.py holds it to scikit-learn on the CPU; the GPU tests are held to it.
Nothing here is ever taken from the device."""
import numpy as np

MINSTD_M, MINSTD_A = 2147483647, 16807


def minstd_uniforms(seed, count):
    """u_t = (x_t - 1) / 2147483646.0 in fp64, x_t the t-th output of std::minstd_rand0(seed)"""
    x = int(seed) % MINSTD_M
    if x == 0:
        x = 1
    out = np.empty(count, dtype=np.float64)
    for t in range(count):
        x = x * MINSTD_A % MINSTD_M
        out[t] = (x - 1) / 2147483646.0
    return out


def sq_distances(X, C):
    """[n][k] fp64 squared distances, by the expansion on columns centred by X's mean (fp64: the cancellation costs ~1e-13)"""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    mu = X.mean(axis=0)
    Xc, Cc = X - mu, C - mu
    D = (Xc * Xc).sum(axis=1)[:, None] - 2.0 * Xc.dot(Cc.T) + (Cc * Cc).sum(axis=1)[None, :]
    return np.maximum(D, 0.0)


def own_distances(X, C, labels):
    """direct fp64 |x_i - c_label(i)|^2"""
    diff = np.asarray(X, dtype=np.float64) - np.asarray(C, dtype=np.float64)[labels]
    return (diff * diff).sum(axis=1)


def l2_normalize(X):
    X = np.asarray(X, dtype=np.float32)
    s = (X.astype(np.float64) ** 2).sum(axis=1)
    inv = np.where(s > 0, 1.0 / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)
    return (X.astype(np.float64) * inv[:, None]).astype(np.float32)


def kmeans_plusplus(X, k, seed):
    """row positions of the start: centre 0 = floor(u_0 n); centre t = the lowest p whose inclusive prefix of the minimum squared
    distances exceeds u_t * total, the lowest position not yet chosen where total is 0"""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    u = minstd_uniforms(seed, k)
    chosen = [min(int(np.floor(u[0] * n)), n - 1)]
    dmin = ((X - X[chosen[0]]) ** 2).sum(axis=1)
    for t in range(1, k):
        prefix = np.cumsum(dmin)
        total = prefix[-1]
        if total > 0:
            p = int(np.searchsorted(prefix, u[t] * total, side="right"))
        else:
            p = next(i for i in range(n) if i not in chosen)
        chosen.append(p)
        dmin = np.minimum(dmin, ((X - X[p]) ** 2).sum(axis=1))
    return np.array(chosen, dtype=np.int64)


def relocate(dist, labels, counts):
    """Empty clusters in ascending id each take the row with the largest `dist`, the lower position on a tie, among rows whose
    cluster has at least two members at that moment. labels and counts are changed in place; returns the relocated positions."""
    moved = []
    for j in np.flatnonzero(counts == 0):
        ok = counts[labels] >= 2
        if not ok.any():
            break
        far = int(np.argmax(np.where(ok, dist, -np.inf)))      # argmax: the first of equal maxima
        counts[labels[far]] -= 1
        labels[far] = j
        counts[j] = 1
        moved.append(far)
    return moved


def update(X, labels, C_old, center_dtype=np.float32):
    """(C_new, counts, labels after relocation): one centre update with the header's relocation rule"""
    X = np.asarray(X, dtype=np.float64)
    k = len(C_old)
    labels = np.array(labels, dtype=np.int64)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    if (counts == 0).any():
        relocate(own_distances(X, C_old, labels), labels, counts)
    C_new = np.array(C_old, dtype=np.float64)
    sums = np.zeros((k, X.shape[1]), dtype=np.float64)
    np.add.at(sums, labels, X)
    has = counts > 0
    C_new[has] = sums[has] / counts[has][:, None]
    return C_new.astype(center_dtype), counts, labels


def margin_of(D):
    """the smallest relative gap (second best - best) / second best over the rows of a distance matrix (inf with one centre)"""
    if D.shape[1] < 2:
        return np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    return float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], np.finfo(np.float64).tiny)).min())


def kmeans(X, C0, max_iter=300, tol=1e-4, center_dtype=np.float32):
    """dict(labels, centers, counts, distances, inertia, n_iter, strict, margin): nvsm_kmeans on the fp32 rows X from the start C0.
    center_dtype float32 is the device's rule (centres are fp32 roundings of fp64 means); float64 is sklearn on X.astype(float64).
    margin: the smallest margin_of over every assignment pass that ran."""
    X32 = np.asarray(X, dtype=np.float32)
    X = X32.astype(np.float64)
    k = len(C0)
    C = np.asarray(C0, dtype=center_dtype)
    bound = tol * X.var(axis=0).mean()
    old = np.full(len(X), -1, dtype=np.int64)
    strict, margin, n_iter = False, np.inf, 0
    labels = old
    for it in range(max_iter):
        D = sq_distances(X, C)
        margin = min(margin, margin_of(D))
        labels = D.argmin(axis=1)
        C_new, counts, labels = update(X, labels, C, center_dtype)
        shift = ((C_new.astype(np.float64) - C.astype(np.float64)) ** 2).sum()
        C = C_new
        n_iter = it + 1
        if np.array_equal(labels, old):
            strict = True
            break
        if shift <= bound:
            break
        old = labels
    if not strict:
        D = sq_distances(X, C)
        margin = min(margin, margin_of(D))
        labels = D.argmin(axis=1)
        counts = np.bincount(labels, minlength=k).astype(np.int64)
    dist = own_distances(X, C, labels)
    return dict(labels=labels.astype(np.int32), centers=C, counts=counts, distances=dist, inertia=float(dist.sum()), n_iter=n_iter,
                strict=strict, margin=margin)


def blobs(n, d, k, seed, noise=0.5, spread=4.0):
    """(X float32, true labels): centres spread * N(0, I), labels arange(n) % k, noise * N(0, I) around them"""
    rs = np.random.RandomState(seed)
    centres = spread * rs.standard_normal((k, d))
    labels = np.arange(n) % k
    X = centres[labels] + noise * rs.standard_normal((n, d))
    return X.astype(np.float32), labels
