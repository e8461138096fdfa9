"""nvsm_kmeans on the device against tests/kmeans_reference.py (held to scikit-learn in tests/test_kmeans_reference.py).

The assignment rule. D64 is the fp64 distance matrix, err32 the largest |D32 − D64| of a float32 numpy evaluation of the centred
expansion on the same inputs, tol = 4·err32 (tests/test_gpu_rank.py's factor: it allows for another summation order over the same
float32 terms). Every row must satisfy D64[i, label_i] <= min_j D64[i, j] + 2·tol, so a row whose two best fp64 distances differ by
more than 2·tol has the exact argmin; no row is left out. Every case prints a `kmeans-error` line with err32 and the worst excess
in units of tol (DESIGN.md §23 quotes them). Neither D64 nor err32 is ever taken from the device."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import check
from tests import kmeans_reference as kr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
DIMS = (3, 36, 64, 256, 300)


def ptr(a):
    return a.ctypes.data


def hook_assign(X, Cn):
    X, Cn = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Cn, dtype=np.float32)
    labels = np.full(len(X), -7, dtype=np.int32)
    dist = np.full(len(X), np.nan, dtype=np.float32)
    check(ca.lib().nvsm_debug_kmeans_assign(ptr(X), len(X), X.shape[1], ptr(Cn), len(Cn), ptr(labels), ptr(dist)))
    return labels, dist


def hook_update(X, labels, C_old):
    X, C_old = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(C_old, dtype=np.float32)
    labels = np.ascontiguousarray(labels, dtype=np.int32).copy()
    C_new = np.full_like(C_old, np.nan)
    counts = np.full(len(C_old), -7, dtype=np.int64)
    shift = C.c_double(-1.0)
    check(ca.lib().nvsm_debug_kmeans_update(ptr(X), len(X), X.shape[1], ptr(labels), ptr(C_old), len(C_old), ptr(C_new), ptr(counts), C.byref(shift)))
    return labels, C_new, counts, shift.value


def hook_plusplus(X, k, seed):
    X = np.ascontiguousarray(X, dtype=np.float32)
    rows = np.full(k, -7, dtype=np.int64)
    centers = np.full((k, X.shape[1]), np.nan, dtype=np.float32)
    check(ca.lib().nvsm_debug_kmeans_plusplus(ptr(X), len(X), X.shape[1], k, seed, ptr(rows), ptr(centers)))
    return rows, centers


def expansion32(X, Cn):
    """the centred expansion in float32 numpy: (D32 [n][k], the magnitudes |x|² + |c|² + 2|x·c| of its three terms)"""
    mean = X.astype(np.float64).mean(axis=0).astype(np.float32)
    Xc, Cc = X - mean, Cn - mean
    xn, cn, dot = (Xc * Xc).sum(axis=1), (Cc * Cc).sum(axis=1), Xc.dot(Cc.T)
    assert xn.dtype == np.float32 and dot.dtype == np.float32
    return xn[:, None] - np.float32(2.0) * dot + cn[None, :], xn[:, None] + cn[None, :] + np.float32(2.0) * np.abs(dot)


def assignment_rule(tag, X, Cn, labels):
    """asserts the module docstring's rule; returns (D64, tol)"""
    D64 = kr.sq_distances(X, Cn)
    D32, _ = expansion32(X, Cn)
    err32 = float(np.abs(D32.astype(np.float64) - D64).max())
    tol = 4.0 * err32
    assert labels.min() >= 0 and labels.max() < len(Cn)
    excess = D64[np.arange(len(X)), labels] - D64.min(axis=1)
    print("kmeans-error %s n=%d d=%d k=%d: err32 %.3g, worst excess %.3g tol" % (tag, len(X), X.shape[1], len(Cn), err32,
                                                                                  excess.max() / tol if tol > 0 else 0.0))
    assert (excess <= 2.0 * tol).all(), (tag, excess.max(), tol)
    return D64, tol


def ulp_close(got, want32):
    """|got − want| <= 1 fp32 ulp of want, elementwise"""
    want32 = np.asarray(want32, dtype=np.float32)
    return bool((np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.spacing(np.abs(want32)).astype(np.float64)).all())


# ---- 1. one assignment pass ---------------------------------------------------------------------------------------------------------
# (n, d, k) across the edges of kmeans_assign_kernel: a workgroup is 128 rows (n = 1, 63, 65 inside one; 257 = two and one row; 1000 =
# eight, the last with 104), a wave 32 rows in two 16-row MFMA tiles (63, 65); a centre tile is 128 centres in eight groups of 16
# (k = 1, 2 inside a group; 17, 65 one centre into the next group; 64 whole groups; 257 two tiles and one centre); a stage is 32 columns in two groups of 16
# (d = 3 inside one group, 36 a tail of 4, 64 and 256 whole stages, 300 a tail of 12).
ASSIGN_CASES = [(1, 3, 1), (63, 3, 2), (65, 36, 17), (63, 64, 17), (65, 300, 65), (257, 64, 64), (257, 256, 65), (257, 36, 257),
                (1000, 300, 17), (1000, 256, 64), (1000, 3, 257), (1000, 64, 2)]


@pytest.mark.parametrize("n,d,k", ASSIGN_CASES, ids=lambda v: str(v))
def test_assignment_far_from_the_origin(n, d, k):
    """Gaussian rows and centres around 50 in every column: without the centring the expansion loses ~|x|²·2^-24 = 0.05·d/300 here"""
    rs = np.random.RandomState(n + d + k)
    X = (50.0 + rs.standard_normal((n, d))).astype(np.float32)
    Cn = (50.0 + rs.standard_normal((k, d))).astype(np.float32)
    labels, dist = hook_assign(X, Cn)
    D64, tol = assignment_rule("far", X, Cn, labels)
    # the kernel's own distance: three float32 terms and an fmaf chain of d products, each within 2^-24 of its magnitude
    _, magnitude = expansion32(X, Cn)
    own = np.arange(n), labels
    assert (np.abs(dist.astype(np.float64) - D64[own]) <= (d + 4) * 2.0 ** -24 * magnitude[own].astype(np.float64)).all()


@pytest.mark.parametrize("n,d,k", [(65, 36, 17), (257, 256, 65), (1000, 300, 257), (63, 3, 2)], ids=lambda v: str(v))
def test_duplicated_centres_go_to_the_lowest_index_and_duplicated_rows_get_equal_labels(n, d, k):
    rs = np.random.RandomState(n + k)
    half = max(1, k // 2)
    base = rs.standard_normal((half, d)).astype(np.float32)
    Cn = np.concatenate([base, base])[:k] if k > 1 else base      # centre j + half is centre j again (a whole tile apart at k = 257)
    if len(Cn) < k:
        Cn = np.concatenate([Cn, base[:1]])                        # odd k: the last centre is centre 0 once more
    X = (Cn[rs.randint(0, k, n)] + 0.1 * rs.standard_normal((n, d))).astype(np.float32)
    h = n // 2
    X[h:2 * h] = X[:h]                                            # the second half repeats the first: other workgroups, other lanes
    labels, _ = hook_assign(X, Cn)
    assignment_rule("dup", X, Cn, labels)
    assert labels.max() < half                                    # exactly: a copy never wins against its lower-index original
    assert np.array_equal(labels[h:2 * h], labels[:h])


# ---- 2. one update --------------------------------------------------------------------------------------------------------------------
def check_update(X, labels, C_old):
    got_labels, C_new, counts, shift = hook_update(X, labels, C_old)
    want_C, want_counts, want_labels = kr.update(X, labels, C_old)
    assert np.array_equal(got_labels, want_labels)
    assert np.array_equal(counts, want_counts)
    assert ulp_close(C_new, want_C)
    want_shift = ((C_new.astype(np.float64) - C_old.astype(np.float64)) ** 2).sum()
    assert abs(shift - want_shift) <= 1e-12 * max(want_shift, 1e-300)
    return got_labels, C_new, counts


@pytest.mark.parametrize("n,d,k", [(257, 3, 2), (1000, 36, 17), (5000, 64, 5), (2000, 256, 65), (5000, 300, 3), (129, 300, 128)], ids=lambda v: str(v))
def test_update_with_a_cluster_of_one_row_and_a_cluster_of_nearly_all(n, d, k):
    """cluster 0 holds n − (k − 1) rows — up to 40 chunks of 128 members, so the segment is cut over many workgroups, with a tail
    chunk — and every other cluster one row, spread over the positions"""
    rs = np.random.RandomState(n + d)
    X = (3.0 + rs.standard_normal((n, d))).astype(np.float32)
    labels = np.zeros(n, dtype=np.int32)
    labels[rs.choice(n, k - 1, replace=False)] = np.arange(1, k)
    check_update(X, labels, rs.standard_normal((k, d)).astype(np.float32))
    # balanced, in random order: every segment has several members, none a whole chunk at the small sizes
    check_update(X, rs.permutation(np.arange(n) % k).astype(np.int32), rs.standard_normal((k, d)).astype(np.float32))


@pytest.mark.parametrize("d", DIMS)
def test_update_settles_empty_clusters_by_the_rule(d):
    rs = np.random.RandomState(d)
    n = 300
    X = rs.standard_normal((n, d)).astype(np.float32)
    C_old = rs.standard_normal((4, d)).astype(np.float32)
    # the farthest row sits alone in cluster 0 and is no candidate; cluster 1 has two members, cluster 2 the rest, cluster 3 is empty
    labels = np.full(n, 2, dtype=np.int32)
    X[5] = C_old[0] + 100.0
    labels[5] = 0
    labels[[7, 200]] = 1
    X[[7, 200]] = C_old[1] + np.array([[30.0], [20.0]], dtype=np.float32)
    got, _, counts = check_update(X, labels, C_old)
    assert got[7] == 3 and counts.tolist() == [1, 1, n - 3, 1]
    # two empty clusters draw from one donor, and rows 11 and 250 are the same row: the lower position goes first
    X = rs.standard_normal((n, d)).astype(np.float32)
    labels = np.zeros(n, dtype=np.int32)
    X[11] = X[250] = C_old[0] + 40.0
    got, _, counts = check_update(X, labels, C_old[:3])
    assert got[11] == 1 and got[250] == 2 and counts.tolist() == [n - 2, 1, 1]
    # more empty clusters than spare rows in the only donor with two members: it gives until one member is left
    labels = np.array([0, 0, 0, 1], dtype=np.int32)
    got, _, counts = check_update(X[:4], labels, C_old)
    assert counts.tolist() == [1, 1, 1, 1] and sorted(got.tolist()) == [0, 1, 2, 3] and got[3] == 1


# ---- 3. the k-means++ start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (3, 256, 300))
def test_kmeans_plusplus_draws_are_consistent_with_fp64(d):
    n, k, seed = 1000, 17, 5
    X, _ = kr.blobs(n, d, 6, seed=d, noise=1.0)
    rows, centers = hook_plusplus(X, k, seed)
    again, _ = hook_plusplus(X, k, seed)
    assert np.array_equal(rows, again)
    assert np.array_equal(centers, X[rows])
    u = kr.minstd_uniforms(seed, k)
    assert rows[0] == int(np.floor(u[0] * n))
    X64 = X.astype(np.float64)
    dmin = ((X64 - X64[rows[0]]) ** 2).sum(axis=1)
    for t in range(1, k):
        prefix = np.cumsum(dmin)
        total, p = prefix[-1], rows[t]
        below = prefix[p - 1] if p > 0 else 0.0
        assert below - 1e-9 * total <= u[t] * total <= prefix[p] + 1e-9 * total, (t, p)
        assert dmin[p] > 0
        dmin = np.minimum(dmin, ((X64 - X64[p]) ** 2).sum(axis=1))
    other, _ = hook_plusplus(X, k, seed + 1)
    assert not np.array_equal(rows, other)


def test_kmeans_plusplus_on_identical_rows_takes_positions_in_order():
    assert np.floor(kr.minstd_uniforms(1, 1)[0] * 1000) == 0      # seed 1 opens with row 0; every total after it is 0
    rows, _ = hook_plusplus(np.full((1000, 36), 0.25, dtype=np.float32), 17, 1)
    assert rows.tolist() == list(range(17))


# ---- 4. the whole call ----------------------------------------------------------------------------------------------------------------
def table_model(X, words=None):
    """a handle whose document table is X (and whose words table is `words`)"""
    n, d = X.shape
    spec = dict(num_words=50 if words is None else len(words), num_entities=n, word_dim=8 if words is None else words.shape[1], entity_dim=d,
                window=2, num_random=1, update_method="sgd")
    params = random_params(spec, np.random.RandomState(1))
    params[E_NAME] = X.ravel().astype(np.float32)
    if words is not None:
        params[W_NAME] = words.ravel().astype(np.float32)
    m = gpu_model(spec, 8)
    load_params(m, params, True)
    return m


def self_consistent(X, out, strict_means, exact_rows=True):
    """what every result must satisfy against its own centres. exact_rows False: X is the device's rows only to an fp32 rounding (the
    host normalised them in another summation order), so distances are held to 1e-5 relative, not to their last bit."""
    labels, centers, counts, inertia, n_iter, dist = out
    assignment_rule("self", X, centers, labels)
    assert np.array_equal(counts, np.bincount(labels, minlength=len(centers)))
    own = kr.own_distances(X, centers, labels)
    if exact_rows:
        assert abs(inertia - own.sum()) <= 1e-9 * own.sum()
        assert ulp_close(dist, own.astype(np.float32))
    else:
        assert abs(inertia - own.sum()) <= 1e-5 * own.sum()
        assert np.allclose(dist, own, rtol=1e-5, atol=1e-7)
    if strict_means:
        want, _, _ = kr.update(X, labels, centers)
        assert ulp_close(centers, want)


@pytest.mark.parametrize("n,d,k", [(257, 3, 2), (600, 36, 5), (1000, 256, 17), (1500, 300, 65), (700, 64, 8)], ids=lambda v: str(v))
def test_separated_blobs_follow_the_reference(n, d, k):
    X, truth = kr.blobs(n, d, k, seed=1)
    want = kr.kmeans(X, X[:k])
    assert want["margin"] >= 0.89 and want["n_iter"] == 2 and want["strict"]      # no near-tie anywhere: the trajectory is determined
    m = table_model(X)
    out = m.kmeans(num_clusters=k, init=X[:k], return_distances=True)
    m.close()
    labels, centers, counts, inertia, n_iter, dist = out
    assert np.array_equal(labels, want["labels"]) and np.array_equal(labels, truth)
    assert np.array_equal(counts, want["counts"]) and n_iter == want["n_iter"]
    assert ulp_close(centers, want["centers"])
    self_consistent(X, out, strict_means=True)


@pytest.mark.parametrize("tol", [1e-4, 0.0])
def test_overlapping_blobs_stop_and_are_self_consistent(tol):
    """noise as large as the separation, a start from random rows: many iterations, near-ties that may legitimately flip, so the
    trajectory is not compared. tol = 0 leaves only the strict stop (a zero shift means the labels stood still too)."""
    n, d, k = 1000, 36, 8
    X, _ = kr.blobs(n, d, k, seed=4, noise=4.0)
    start = X[np.random.RandomState(2).choice(n, k, replace=False)]
    m = table_model(X)
    out = m.kmeans(num_clusters=k, init=start, tol=tol, max_iter=300, return_distances=True)
    m.close()
    assert 3 <= out[4] < 300
    self_consistent(X, out, strict_means=tol == 0.0)
    assert out[3] < kr.own_distances(X, start, kr.sq_distances(X, start).argmin(axis=1)).sum()


# ---- 5. state and selection -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    rs = np.random.RandomState(8)
    X, _ = kr.blobs(400, 36, 6, seed=3, noise=1.5)
    words = rs.standard_normal((300, 300)).astype(np.float32) + 2.0
    m = table_model(X, words)
    yield X, words, m
    m.close()


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_rows_by_id_by_limit_normalised_and_from_the_words_table(tables):
    X, words, m = tables
    rs = np.random.RandomState(5)
    ids = rs.permutation(400)[:130].astype(np.int64)
    ids[17] = ids[3]                                              # unsorted, with a duplicate
    kw = dict(num_clusters=5, ids=ids, seed=7, return_distances=True)
    a, b = m.kmeans(**kw), m.kmeans(**kw)
    assert same_bits(a, b)
    assert a[0][17] == a[0][3]
    self_consistent(X[ids], a, strict_means=False)
    other = table_model(X[ids])                                   # the same rows, already gathered, in a table of their own
    assert same_bits(a, other.kmeans(num_clusters=5, seed=7, return_distances=True))
    other.close()
    c = m.kmeans(num_clusters=5, limit=130, seed=7, return_distances=True)
    assert len(c[0]) == 130 and not np.array_equal(c[1], a[1])
    self_consistent(X[:130], c, strict_means=False)
    e = m.kmeans(num_clusters=4, l2_normalize=True, seed=2, return_distances=True)
    self_consistent(kr.l2_normalize(X), e, strict_means=False, exact_rows=False)
    w = m.kmeans(space="words", num_clusters=9, limit=257, seed=2, return_distances=True)
    assert w[1].shape == (9, 300)
    self_consistent(words[:257], w, strict_means=False)
    assert same_bits(m.kmeans(**kw), a)                           # a smaller call behind larger ones: the grown scratch changes nothing


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
    got_e = a.kmeans(ids=eids, num_clusters=4, max_iter=5, seed=3, return_distances=True)      # straight behind nvsm_step
    got_w = a.kmeans(space="words", ids=wids, num_clusters=3, max_iter=5, seed=3, return_distances=True)
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0 and np.abs(logical[W_NAME] - params[W_NAME]).max() > 0
    # the distances are exact roundings of fp64 values of the rows read: they hold only if the logical rows were the ones read
    self_consistent(logical[E_NAME].reshape(-1, 36)[eids], got_e, strict_means=False)
    self_consistent(logical[W_NAME].reshape(-1, 12)[wids], got_w, strict_means=False)
    ten(10)
    for n in list(PARAMS) + ADAM_STATE:                       # b never called nvsm_kmeans
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.close()
    b.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
GUARD = np.float32(12345.0)


def raw_kmeans(m, **fields):
    o = ca.NvsmKmeansOptions()
    ca.lib().nvsm_kmeans_options_default(C.byref(o))
    keep = []
    for key, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = ptr(v)
        setattr(o, key, v)
    labels = np.full(500, -5, dtype=np.int32)
    centers = np.full(500 * 36, GUARD, dtype=np.float32)
    counts = np.full(500, -5, dtype=np.int64)
    dist = np.full(500, GUARD, dtype=np.float32)
    inertia, it = C.c_double(-5.0), C.c_int32(-5)
    st = ca.lib().nvsm_kmeans(m._h, C.byref(o), ptr(labels), ptr(centers), ptr(counts), ptr(dist), C.byref(inertia), C.byref(it))
    untouched = (labels == -5).all() and (centers == GUARD).all() and (counts == -5).all() and (dist == GUARD).all() and \
        inertia.value == -5.0 and it.value == -5
    return st, ca.lib().nvsm_last_error(), untouched


def test_refusals_are_status_codes_in_order_nothing_is_written_and_the_handle_still_works(tables):
    X, words, m = tables
    nan, inf = float("nan"), float("inf")
    bad_init = np.zeros((8, 36), dtype=np.float32)
    bad_init[5, 7] = inf
    cases = [(dict(space=ca.SPACE_PROJECTED_WORDS, num_rows=-1), b"space", 1), (dict(space=9), b"space", 1),
             (dict(num_rows=-4, num_clusters=0), b"num_rows", 1), (dict(num_rows=401, num_clusters=0), b"num_rows", 1),
             (dict(ids=np.array([1, 400], dtype=np.int64), num_rows=2, num_clusters=0), b"row id", 1),
             (dict(ids=np.array([-1, 2], dtype=np.int64), num_rows=2, num_clusters=9), b"row id", 1),
             (dict(num_clusters=0, max_iter=0), b"num_clusters", 1), (dict(num_rows=5, num_clusters=6, max_iter=0), b"num_clusters", 1),
             (dict(max_iter=0, tol=nan), b"max_iter", 1), (dict(tol=nan, init=5), b"tol", 1), (dict(tol=-1e-9, init=5), b"tol", 1),
             (dict(tol=inf, init=5), b"tol", 1), (dict(init=5, seed=0), b"init", 1),
             (dict(init=ca.KMEANS_INIT_GIVEN, seed=0), b"init_centers", 1),
             (dict(init=ca.KMEANS_INIT_GIVEN, init_centers=bad_init, seed=0), b"init_centers", 1),
             (dict(seed=0), b"seed", 1), (dict(seed=-3), b"seed", 1)]
    for fields, word, status in cases:
        st, msg, untouched = raw_kmeans(m, **fields)
        assert st == status and word in msg and untouched, (fields, st, msg)
    big = table_model(np.zeros((ca.KMEANS_MAX_CLUSTERS + 1, 1), dtype=np.float32))
    o = ca.NvsmKmeansOptions()
    ca.lib().nvsm_kmeans_options_default(C.byref(o))
    o.num_clusters, o.max_iter = ca.KMEANS_MAX_CLUSTERS + 1, 0
    out = np.zeros(8, dtype=np.int64)
    inertia, it = C.c_double(-5.0), C.c_int32(-5)
    st = ca.lib().nvsm_kmeans(big._h, C.byref(o), ptr(out), ptr(out), ptr(out), None, C.byref(inertia), C.byref(it))
    msg = ca.lib().nvsm_last_error()
    big.close()
    assert st == 2 and b"clusters" in msg and not out.any() and it.value == -5      # NVSM_ERR_UNSUPPORTED, before max_iter is looked at
    labels, centers, counts, inertia, n_iter = m.kmeans(num_clusters=6, seed=1)
    assert counts.sum() == 400 and np.isfinite(centers).all() and n_iter >= 1


def test_only_the_kmeans_call_records_the_kmeans_names(tables):
    X, words, m = tables
    m.profile_enable(True)
    m.profile_reset()
    m.related_documents([1, 2], top_k=3)
    assert not [n for n in m.profile() if n.startswith("kmeans_")]
    m.kmeans(num_clusters=6, seed=1)
    names = {n for n in m.profile() if n.startswith("kmeans_")}
    m.profile_enable(False)
    assert names >= {"kmeans_rows", "kmeans_plusplus", "kmeans_assign", "kmeans_update", "kmeans_inertia", "kmeans_assign_mfma"}, names
    assert ca.KMEANS_MAX_CLUSTERS == 4096
