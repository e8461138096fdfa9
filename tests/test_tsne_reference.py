"""tests/tsne_reference.py, the fp64 restatement the GPU tests of nvsm_tsne are held to, against scikit-learn itself (1.7), on the CPU.

Exact inputs: the conditional probabilities against sklearn.manifold._utils._binary_search_perplexity on the same float32
distances, _joint_probabilities, _kl_divergence for a given (P, Y) and five iterations of _gradient_descent from a given start.
MEASURED (n = 120, d = 8, this file's inputs): conditionals 5.4e-16 of the largest (the sums run in another order), joint
probabilities 3.4e-16, KL equal to the last bit, the gradient 1.1e-15 of its largest component, five iterations 1.4e-15 of the
embedding's extent — sklearn's loop takes the dtype of the start, and the start here is float64.
The bounds below are 1e-11: fp64 rounding with room, orders of magnitude under any restatement mistake.

Whole runs cannot be compared point by point: from a 1e-4 start an fp32 and an fp64 run of the same code differ by 2e-6 after 5
iterations, by 7e-2 after 20 and by the size of the picture after 50 (n = 300, d = 16, three clusters, perplexity 30). They are
held to scikit-learn only by their final KL and trustworthiness.

The file also vets the rules of tests/test_gpu_tsne.py without a device: the float32 numpy chain passes each of them, and each
still separates a deliberately wrong result with the tolerance DOUBLED — a perplexity off by 1 %, a dropped 4·, the exaggeration
left on."""
import numpy as np
import pytest

from tests import tsne_reference as tr

sklearn = pytest.importorskip("sklearn")
from sklearn.manifold import TSNE, _t_sne, _utils, trustworthiness  # noqa: E402
from scipy.spatial.distance import squareform  # noqa: E402

BOUND = 1e-11


@pytest.fixture(scope="module")
def small():
    rs = np.random.RandomState(5)
    X, labels = tr.clusters(rs, n=120, d=8)
    D = tr.sq_distances(X)
    C, steps = tr.conditionals(D, 30.0)
    return dict(X=X, labels=labels, D=D, C=C, steps=steps, P=tr.joint(C), Y=(rs.standard_normal((120, 2)) * 3.0))


def test_squared_distances_are_symmetric_with_a_zero_diagonal(small):
    D = small["D"]
    assert D.dtype == np.float32 and np.array_equal(D, D.T) and not D.diagonal().any()
    X = small["X"].astype(np.float64)
    want = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    assert np.abs(D - want).max() <= 2.0 ** -24 * want.max()


def test_conditionals_match_sklearns_binary_search(small):
    theirs = _utils._binary_search_perplexity(small["D"], 30.0, 0)
    rel = np.abs(small["C"] - theirs).max() / theirs.max()
    print("tsne-reference conditionals: max difference / max %.3g, steps %d..%d" % (rel, small["steps"].min(), small["steps"].max()))
    assert rel <= BOUND and small["steps"].max() < 100
    assert not small["C"].diagonal().any() and np.allclose(small["C"].sum(axis=1), 1.0, atol=1e-12)
    for i in (0, 57, 119):      # the entropy a stored row realises, recovered without its beta
        assert abs(tr.row_entropy(small["D"][i], small["C"][i], i) - np.log(30.0)) <= 1e-5 + 1e-9


def test_joint_probabilities_match_sklearn(small):
    theirs = squareform(_t_sne._joint_probabilities(small["D"], 30.0, 0))
    P = small["P"]
    assert np.abs(P - theirs).max() / theirs.max() <= BOUND
    assert np.array_equal(P, P.T) and not P.diagonal().any()
    assert abs(P.sum() - 1.0) <= P.size * tr.EPS + 1e-13      # (every cell the eps clamp lifts adds up to eps to the total)


@pytest.mark.parametrize("exaggeration", (1.0, 12.0))
def test_kl_and_gradient_match_sklearn(small, exaggeration):
    P, Y = small["P"] * exaggeration, small["Y"]
    kl, grad = _t_sne._kl_divergence(Y.ravel().copy(), squareform(P, checks=False), 1.0, 120, 2)
    g, largest = tr.gradient(small["P"], Y, exaggeration)
    assert abs(tr.kl_divergence(small["P"], Y, exaggeration) - kl) <= BOUND * abs(kl)
    assert np.abs(g.ravel() - grad).max() <= BOUND * np.abs(grad).max()
    assert (largest > 0).all() and (np.abs(g).max(axis=1) <= 120 * largest).all()


def test_five_iterations_match_sklearns_gradient_descent(small):
    rs = np.random.RandomState(11)
    Y0 = 1e-4 * rs.standard_normal((120, 2))
    P12 = squareform(small["P"] * 12.0, checks=False)
    p, err, it = _t_sne._gradient_descent(_t_sne._kl_divergence, Y0.ravel().copy(), it=0, max_iter=5, n_iter_check=50, momentum=0.5,
                                          learning_rate=50.0, n_iter_without_progress=250, args=[P12, 1.0, 120, 2], kwargs={})
    Y, kl, n_iter = tr.descent(small["P"], Y0, 50.0, 12.0, exploration=5, max_iter=5)
    assert n_iter == it == 4 and abs(kl - err) <= BOUND * abs(err)
    assert np.abs(Y.ravel() - p).max() <= BOUND * np.abs(p).max()


def test_the_phase_boundary_and_the_stopping_rules(small):
    rs = np.random.RandomState(12)
    Y0 = 1e-4 * rs.standard_normal((120, 2))
    Y, kl, n_iter = tr.descent(small["P"], Y0, 50.0, 12.0, exploration=3, max_iter=5)
    # by hand: three iterations of phase one, then two of phase two with gains and update reset
    p = Y0.ravel().copy()
    for first, last, momentum, e in ((0, 3, 0.5, 12.0), (3, 5, 0.8, 1.0)):
        p, err, it = _t_sne._gradient_descent(_t_sne._kl_divergence, p, it=first, max_iter=last, n_iter_check=50, momentum=momentum,
                                              learning_rate=50.0, n_iter_without_progress=250,
                                              args=[squareform(small["P"] * e, checks=False), 1.0, 120, 2], kwargs={})
    assert n_iter == it == 4 and abs(kl - err) <= BOUND * abs(err) and np.abs(Y.ravel() - p).max() <= BOUND * np.abs(p).max()
    # min_grad_norm: the first check (iteration 49) ends each phase
    _, kl, n_iter = tr.descent(small["P"], Y0, 50.0, 12.0, exploration=250, max_iter=1000, min_grad_norm=1e30)
    assert n_iter == 99 and np.isfinite(kl)


def test_pca_start(small):
    Y0, w = tr.pca_start(small["X"])
    assert abs(Y0[:, 0].std() - 1e-4) <= 1e-16 and w[0] >= w[1] >= w[2]
    from sklearn.decomposition import PCA
    theirs = PCA(n_components=2, svd_solver="full").fit_transform(small["X"].astype(np.float64))
    theirs = theirs / theirs[:, 0].std() * 1e-4
    assert np.abs(Y0 - theirs).max() <= 1e-9 * np.abs(theirs).max()
    with pytest.raises(ValueError):
        tr.pca_start(np.ones((5, 3)))


def test_trustworthiness_matches_sklearn(small):
    for Y in (small["Y"], small["X"][:, :2]):
        assert abs(tr.trustworthiness(small["X"], Y, 5) - trustworthiness(small["X"], Y, n_neighbors=5)) <= 1e-12


def test_whole_runs_meet_sklearn_in_kl_and_trustworthiness():
    X, labels = tr.clusters(np.random.RandomState(2024))
    sk = TSNE(n_components=2, method="exact", init="pca", random_state=0, max_iter=1000)
    Ys = sk.fit_transform(X)
    Y, kl, n_iter = tr.tsne(X, max_iter=1000)
    print("tsne-reference whole run: KL %.4f (sklearn %.4f), trustworthiness %.4f (sklearn %.4f), n_iter %d (sklearn %d)"
          % (kl, sk.kl_divergence_, tr.trustworthiness(X, Y), tr.trustworthiness(X, Ys), n_iter, sk.n_iter_))
    assert abs(kl - sk.kl_divergence_) <= 0.05 and abs(tr.trustworthiness(X, Y) - tr.trustworthiness(X, Ys)) <= 0.02
    assert abs(tr.kl_divergence(tr.affinities(X, 30.0)[0], Y) - kl) <= 1e-3      # the run's own figure is the KL at (nearly) its last Y
    assert tr.nearest_label_agreement(Y, labels) == 1.0 == tr.nearest_label_agreement(Ys, labels)


# ---- the GPU cases' rules, vetted without a device: the float32 chain passes, and a wrong result fails at twice the tolerance ----
def worst(got, want, scale):
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / scale).max())


def test_the_affinity_rule_separates_a_perplexity_off_by_one_percent(small):
    X = small["X"]
    P64, _, steps = tr.affinities(X, 30.0)
    P32 = tr.affinities(X, 30.0, np.float32)[0]
    off = ~np.eye(len(X), dtype=bool)
    err32 = worst(P32[off], P64[off], P64[off])
    wrong = worst(tr.affinities(X, 30.3)[0][off], P64[off], P64[off])
    print("tsne-vet affinities: err32 %.3g, 1 %% perplexity %.3g" % (err32, wrong))
    assert steps.max() < 100 and err32 > 0 and wrong > 8 * err32


@pytest.mark.parametrize("scale,exaggeration", [(1e-4, 12.0), (1.0, 1.0), (30.0, 1.0), (30.0, 12.0)])
def test_the_gradient_rule_separates_a_dropped_factor_and_the_exaggeration(small, scale, exaggeration):
    P = small["P"].astype(np.float32)
    Y = (small["Y"] / 3.0 * scale).astype(np.float32)
    g64, largest = tr.gradient(P, Y, exaggeration)
    g32, _ = tr.gradient(P, Y, exaggeration, np.float32)
    err32 = worst(g32, g64, largest[:, None])
    dropped = worst(tr.gradient(P, Y, exaggeration, factor=1.0)[0], g64, largest[:, None])
    other = worst(tr.gradient(P, Y, 12.0 if exaggeration == 1.0 else 1.0)[0], g64, largest[:, None])
    kl64, kl32 = tr.kl_divergence(P, Y, exaggeration), tr.kl_divergence(P, Y, exaggeration, np.float32)
    kl_other = tr.kl_divergence(P, Y, 12.0 if exaggeration == 1.0 else 1.0)
    print("tsne-vet gradient scale %g e %g: err32 %.3g, dropped 4 %.3g, other exaggeration %.3g; KL err32 %.3g, other %.3g"
          % (scale, exaggeration, err32, dropped, other, abs(kl32 - kl64), abs(kl_other - kl64)))
    assert err32 > 0 and dropped > 8 * err32 and other > 8 * err32
    assert abs(kl_other - kl64) > 8 * abs(kl32 - kl64)


def test_the_loop_rule_separates_the_exaggeration_left_on(small):
    P = small["P"].astype(np.float32)
    Y0 = (1e-4 * np.random.RandomState(13).standard_normal((120, 2))).astype(np.float32)
    Y64, _, _ = tr.descent(P, Y0, 50.0, 12.0, exploration=3, max_iter=5)
    Y32, _, _ = tr.descent(P, Y0, np.float32(50.0), 12.0, exploration=3, max_iter=5, dtype=np.float32)
    wrong, _, _ = tr.descent(P, Y0, 50.0, 12.0, exploration=3, max_iter=5, leave_exaggeration_on=True)
    scale = np.abs(Y64).max()
    err32 = worst(Y32, Y64, scale)
    print("tsne-vet loop: err32 %.3g, exaggeration left on %.3g" % (err32, worst(wrong, Y64, scale)))
    assert err32 > 0 and worst(wrong, Y64, scale) > 8 * err32


# ---- ... and over the GPU cases' own generators (tests/test_gpu_tsne.py), case by case ------------------------------------------------
from tests import test_gpu_tsne as gpu_cases  # noqa: E402

# Where the element-wise affinity rule has NO power: err32 is the float32 chain's worst relative deviation over all cells, and in
# these cases some cell of the float32 P is off by a large factor (a far row whose float32 search lands elsewhere; near-eps cells at
# perplexity 1.5), so 4·err32 admits a perplexity that is 1 % off. There the entropy check (|H_i − log perplexity| <= 1.1e-5 on the
# stored conditionals) is what holds the case, and this test asserts that it does. n = 2 has P = 0.5 whatever the perplexity is.
AFFINITY_RULE_HAS_NO_POWER = {("gauss", 5, 36), ("far", 65, 6)}


@pytest.mark.parametrize("kind,n,d", [c for c in gpu_cases.AFFINITY_CASES if c[1] > 2], ids=lambda v: str(v))
def test_every_gpu_affinity_case_separates_a_perplexity_off_by_one_percent(kind, n, d):
    X, perp, P64, C64, steps, err32 = gpu_cases.reference_affinities(kind, n, d)
    off = ~np.eye(n, dtype=bool)
    Pw, Cw, _ = tr.affinities(X, perp * 1.01)
    wrong = worst(Pw[off], P64[off], P64[off])
    D = tr.sq_distances(X)
    target = float(np.log(np.float64(np.float32(perp))))
    entropy_right = max(abs(tr.row_entropy(D[i], C64[i], i) - target) for i in range(n))
    entropy_wrong = max(abs(tr.row_entropy(D[i], Cw[i], i) - target) for i in range(n))
    print("tsne-vet affinities %s n=%d d=%d: err32 %.3g, 1 %% perplexity %.3g; entropy off by %.3g (right) / %.3g (wrong)"
          % (kind, n, d, err32, wrong, entropy_right, entropy_wrong))
    assert steps.max() < 100 and entropy_right <= 1.1e-5 and entropy_wrong > 2 * 1.1e-5      # the entropy check holds every case
    assert (wrong > 8 * err32) == ((kind, n, d) not in AFFINITY_RULE_HAS_NO_POWER)


@pytest.mark.parametrize("n", gpu_cases.NS)
def test_every_gpu_gradient_and_loop_case_separates_the_wrong_results(n):
    rs = np.random.RandomState(77 + n)
    P = gpu_cases.given_p(rs, n)
    base = rs.standard_normal((n, 2))
    for scale in (1e-4, 1.0, 30.0):
        for e in (1.0, 12.0):
            Y = (base * scale).astype(np.float32)
            g64, largest = tr.gradient(P, Y, e)
            err32 = worst(tr.gradient(P, Y, e, np.float32)[0], g64, largest[:, None])
            dropped = worst(tr.gradient(P, Y, e, factor=1.0)[0], g64, largest[:, None])
            other = worst(tr.gradient(P, Y, 13.0 - e)[0], g64, largest[:, None])
            kl64 = tr.kl_divergence(P, Y, e)
            kl_err32, kl_other = abs(tr.kl_divergence(P, Y, e, np.float32) - kl64), abs(tr.kl_divergence(P, Y, 13.0 - e) - kl64)
            assert dropped > 8 * err32 and other > 8 * err32 and kl_other > 8 * kl_err32, (n, scale, e, err32, dropped, other, kl_err32, kl_other)
    rs = np.random.RandomState(500 + n)
    P = gpu_cases.given_p(rs, n)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    lr = np.float32(tr.auto_learning_rate(n))
    kw = dict(exploration=3, max_iter=5)
    Y64, kl64, _ = tr.descent(P, Y0, lr, 12.0, **kw)
    runs = gpu_cases.float32_runs(lambda perm: tr.descent(P[np.ix_(perm, perm)], Y0[perm], lr, 12.0, dtype=np.float32, **kw)[:2], n)
    Yw, klw, _ = tr.descent(P, Y0, lr, 12.0, leave_exaggeration_on=True, **kw)
    scale = np.abs(Y64).max()
    err32, kl_err32 = worst(runs[0][0], Y64, scale), max(abs(k - kl64) for _, k in runs)
    print("tsne-vet loop n=%d: err32 %.3g, exaggeration left on %.3g; KL err32 %.3g, left on %.3g" % (n, err32, worst(Yw, Y64, scale), kl_err32, abs(klw - kl64)))
    assert worst(Yw, Y64, scale) > 8 * err32 and abs(klw - kl64) > 8 * kl_err32
