"""tests/kmeans_reference.py — the fp64 restatement the GPU tests of nvsm_kmeans are held to — against scikit-learn on the CPU, and
its two own rules (relocation, the k-means++ draw) against cases written out by hand. cluster_agreement against sklearn.metrics."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import kmeans_reference as kr

sklearn_cluster = pytest.importorskip("sklearn.cluster")
sklearn_metrics = pytest.importorskip("sklearn.metrics")


@pytest.mark.parametrize("n,d,k", [(600, 36, 5), (1000, 256, 17), (257, 3, 2), (700, 64, 8)])
def test_lloyd_equals_sklearn_from_a_given_start(n, d, k):
    X, _ = kr.blobs(n, d, k, seed=n + k, noise=2.0)
    rs = np.random.RandomState(7)
    C0 = X[rs.choice(n, k, replace=False)].astype(np.float64)
    want = sklearn_cluster.KMeans(n_clusters=k, init=C0, n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X.astype(np.float64))
    got = kr.kmeans(X, C0, center_dtype=np.float64)
    assert got["n_iter"] == want.n_iter_
    assert np.array_equal(got["labels"], want.labels_)
    assert abs(got["inertia"] - want.inertia_) <= 1e-12 * want.inertia_
    assert np.array_equal(got["counts"], np.bincount(want.labels_, minlength=k))


def test_cluster_agreement_equals_sklearn_metrics():
    rs = np.random.RandomState(0)
    for n, k, c in [(500, 7, 5), (50, 3, 3), (40, 1, 4), (40, 4, 1), (30, 30, 2)]:
        labels, classes = rs.randint(0, k, n), rs.randint(0, c, n)
        purity, nmi, ari = ca.cluster_agreement(labels, classes)
        assert abs(nmi - sklearn_metrics.normalized_mutual_info_score(classes, labels)) <= 1e-12
        assert abs(ari - sklearn_metrics.adjusted_rand_score(classes, labels)) <= 1e-12
        assert 0.0 < purity <= 1.0
    same = rs.randint(0, 4, 60)
    assert ca.cluster_agreement(same, (same + 1) % 4) == (1.0, pytest.approx(1.0, abs=1e-12), 1.0)


def test_purity_by_hand_and_classes_may_be_strings():
    # cluster 0: x x x -> 3; cluster 1: x y y -> 2: (3 + 2) / 6
    purity, nmi, ari = ca.cluster_agreement([0, 0, 0, 1, 1, 1], ["x", "x", "x", "x", "y", "y"])
    assert purity == 5.0 / 6.0
    assert abs(nmi - sklearn_metrics.normalized_mutual_info_score([0, 0, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1])) <= 1e-12
    with pytest.raises(ValueError):
        ca.cluster_agreement([0, 1], [0])


def test_relocation_the_only_candidate_sits_in_a_two_member_cluster():
    # clusters: 0 = {row 0} (one member: no candidate, although it is the farthest), 1 = {rows 1, 2}, 2 = empty
    dist = np.array([9.0, 1.0, 2.0])
    labels, counts = np.array([0, 1, 1]), np.array([1, 2, 0])
    assert kr.relocate(dist, labels, counts) == [2]
    assert labels.tolist() == [0, 1, 2] and counts.tolist() == [1, 1, 1]


def test_relocation_two_empty_clusters_draw_from_one_donor_and_ties_take_the_lower_position():
    # cluster 0 = {rows 0..3}, clusters 1 and 2 empty. Rows 1 and 3 tie for the farthest: 1 goes to cluster 1, then 3 to cluster 2.
    dist = np.array([0.5, 4.0, 1.0, 4.0])
    labels, counts = np.zeros(4, dtype=np.int64), np.array([4, 0, 0])
    assert kr.relocate(dist, labels, counts) == [1, 3]
    assert labels.tolist() == [0, 1, 0, 2] and counts.tolist() == [2, 1, 1]
    # a donor that is down to two members still gives, one that is down to one does not
    dist = np.array([3.0, 2.0, 1.0])
    labels, counts = np.zeros(3, dtype=np.int64), np.array([3, 0, 0, 0])
    assert kr.relocate(dist, labels, counts) == [0, 1]
    assert labels.tolist() == [1, 2, 0] and counts.tolist() == [1, 1, 1, 0]


def test_update_relocates_before_the_sums_are_taken():
    X = np.array([[0.0], [1.0], [10.0]], dtype=np.float32)
    C_old = np.array([[0.0], [50.0]], dtype=np.float32)
    C_new, counts, labels = kr.update(X, [0, 0, 0], C_old)
    assert labels.tolist() == [0, 0, 1] and counts.tolist() == [2, 1]
    assert C_new.ravel().tolist() == [0.5, 10.0]


def test_kmeans_plusplus_by_hand():
    # seed 1: x = 16807, 282475249, 1622650073 -> u = 7.826e-6, 0.13154, 0.75560
    u = kr.minstd_uniforms(1, 3)
    assert u[0] == 16806 / 2147483646.0 and u[1] == 282475248 / 2147483646.0 and u[2] == 1622650072 / 2147483646.0
    X = np.array([[0.0], [1.0], [3.0], [3.0]], dtype=np.float32)
    # centre 0 = row floor(u0 * 4) = 0; dmin = (0, 1, 9, 9), prefix (0, 1, 10, 19), u1 * 19 = 2.499 -> row 2;
    # dmin = (0, 1, 0, 0), prefix (0, 1, 1, 1), u2 * 1 = 0.756 -> row 1
    assert kr.kmeans_plusplus(X, 3, 1).tolist() == [0, 2, 1]
    # identical rows: total is 0, the lowest position not yet chosen
    assert kr.kmeans_plusplus(np.ones((5, 2), dtype=np.float32), 4, 1).tolist() == [0, 1, 2, 3]


def test_minstd_uniforms_follow_the_package_generator():
    from cunvsm_amd.model import minstd_canonical
    got = kr.minstd_uniforms(12345, 6)
    x = np.round(got * 2147483646.0 + 1.0)
    want = minstd_canonical(12345, 6)      # (x - 1) / 2^31 in float32
    assert np.allclose((x - 1.0) / 2.0 ** 31, want, rtol=1e-6)


@pytest.mark.parametrize("n,d,k", [(257, 3, 2), (600, 36, 5), (1000, 256, 17), (1500, 300, 65), (700, 64, 8)])
def test_the_blob_cases_of_the_gpu_suite_have_their_margin(n, d, k):
    X, truth = kr.blobs(n, d, k, seed=1)
    got = kr.kmeans(X, X[:k])
    assert got["margin"] >= 0.89, got["margin"]
    assert got["strict"] and got["n_iter"] == 2 and np.array_equal(got["labels"], truth)
