"""nvsm_tsne on the device (include/cunvsm_amd.h; kernels: csrc/tsne.hip) against tests/tsne_reference.py, the fp64 numpy
restatement that tests/test_tsne_reference.py holds to scikit-learn on the CPU. Nothing here reads scikit-learn.

TOLERANCE RULE (tests/test_gpu_rank.py's): the fp64 value and err32, the deviation of the float32 numpy chain from it, both come
from the reference; the device must stay within 4·err32; neither is ever taken from the device. Every case prints a `tsne-error`
line with err32 and the observed ratio (DESIGN.md §19 quotes them). The KL a run reports is a single number: its err32 is the
largest deviation over VARIANTS float32 runs of the reference (float32_runs), and the device is held to 4 times that as well.

Shapes: n in {2, 3, 5, 63, 64, 65, 130, 300} (rows and columns end inside a wave, at a tile's edge and one past it, column slabs
end inside a tile), d in {1, 6, 36, 256, 300}; perplexity 30 where n > 90, else max(1.5, n / 4).
n = 2 in the affinity test is a case of its own: a row with ONE neighbour has entropy 0 whatever beta is, so the search runs out
its 100 steps by construction (asserted on the reference) and the entropy check does not apply; every other case needs fewer than
100 steps in every row, asserted on the reference."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import check
from tests import tsne_reference as tr
from tests.conftest import ROOT
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
GUARD = np.float32(12345.0)
NS = (2, 3, 5, 63, 64, 65, 130, 300)


def perplexity_of(n):
    return 30.0 if n > 90 else max(1.5, n / 4.0)


def ptr(a):
    return a.ctypes.data


def rows_of(kind, rs, n, d):
    X = rs.standard_normal((n, d))
    if kind == "identical":            # pairs at distance 0
        X[1] = X[0]
        X[n - 1] = X[n // 2]
    elif kind == "far":                # one row whose every exp(-D) underflows at beta = 1: the 1e-8 sum and the halving branch
        X[n // 3] += 100.0
    elif kind == "tight":              # every distance tiny: the entropy starts too high, beta doubles with no upper bound yet
        X *= 0.01
    X = X.astype(np.float32)
    return tr.l2_normalize(X) if kind == "l2" else X


def hook_affinities(X, perplexity):
    n, d = X.shape
    P = np.full((n + 2, n), GUARD, dtype=np.float32)
    cond = np.full((n, n), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_affinities(ptr(X), n, d, perplexity, ptr(P), ptr(cond)))
    assert (P[0] == GUARD).all() and (P[-1] == GUARD).all(), "the rows round the output came back changed"
    return P[1:-1].copy(), cond


def hook_gradient(P, Y, exaggeration):
    n = len(Y)
    g, kl = np.full((n, 2), GUARD, dtype=np.float32), C.c_double(-1.0)
    check(ca.lib().nvsm_debug_tsne_gradient(ptr(P), ptr(Y), n, exaggeration, ptr(g), C.byref(kl)))
    return g, kl.value


def hook_descent(P, Y0, lr, exploration, max_iter, min_grad_norm=1e-7, without_progress=300, exaggeration=12.0):
    o = ca.NvsmTsneOptions()
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    o.learning_rate, o.max_iter, o.min_grad_norm, o.n_iter_without_progress, o.early_exaggeration = lr, max_iter, min_grad_norm, without_progress, exaggeration
    Y = np.ascontiguousarray(Y0, dtype=np.float32).copy()
    kl, it = C.c_double(-1.0), C.c_int32(-1)
    check(ca.lib().nvsm_debug_tsne_descent(ptr(P), ptr(Y), len(Y), C.byref(o), exploration, C.byref(kl), C.byref(it)))
    return Y, kl.value, it.value


def worst(got, want, scale):
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / scale).max())


_AFFINITIES = {}


def reference_affinities(kind, n, d):
    """(X, perplexity, P64, stored conditionals, steps, err32), computed once and shared"""
    key = (kind, n, d)
    if key not in _AFFINITIES:
        X = rows_of(kind, np.random.RandomState(n * 1000 + d), n, d)
        perp = perplexity_of(n)
        P64, C64, steps = tr.affinities(X, perp)
        P32 = tr.affinities(X, perp, np.float32)[0]
        off = ~np.eye(n, dtype=bool)
        _AFFINITIES[key] = (X, perp, P64, C64, steps, worst(P32[off], P64[off], P64[off]))
    return _AFFINITIES[key]


# ---- 1. affinities ---------------------------------------------------------------------------------------------------------------------
AFFINITY_CASES = [("gauss", 3, 6), ("gauss", 5, 36), ("identical", 63, 256), ("l2", 64, 300), ("far", 65, 6), ("tight", 65, 1),
                  ("gauss", 130, 36), ("far", 130, 1), ("l2", 300, 256), ("identical", 300, 6), ("tight", 300, 36), ("gauss", 2, 1)]


@pytest.mark.parametrize("kind,n,d", AFFINITY_CASES, ids=lambda v: str(v))
def test_affinities(kind, n, d):
    X, perp, P64, C64, steps, err32 = reference_affinities(kind, n, d)
    if n == 2:
        assert (steps == 100).all()
    else:
        assert steps.max() < 100, "the inputs must let the reference's search end in every row"
    P, cond = hook_affinities(X, perp)
    off = ~np.eye(n, dtype=bool)
    assert np.array_equal(P.view(np.uint32), P.T.view(np.uint32)) and not P.diagonal().any()
    assert (P[off] >= np.float32(tr.EPS)).all()
    assert abs(P.astype(np.float64).sum() - 1.0) <= 2.0 ** -23 + n * n * tr.EPS      # fp32 rounding of n² terms, and the clamp's lifts
    ratio = worst(P[off], P64[off], P64[off]) / err32 if err32 > 0 else worst(P[off], P64[off], P64[off])
    print("tsne-error affinities %s n=%d d=%d: err32 %.3g, max relative |P - P64| / err32 %.3g, search steps %d..%d"
          % (kind, n, d, err32, ratio, steps.min(), steps.max()))
    assert worst(P[off], P64[off], P64[off]) <= 4 * err32
    assert not cond.diagonal().any() and (cond[off] >= 0).all()
    if n > 2:
        D = tr.sq_distances(X)
        target = float(np.log(np.float64(np.float32(perp))))
        entropy = np.array([tr.row_entropy(D[i], cond[i], i) for i in range(n)])
        assert np.abs(entropy - target).max() <= 1.1e-5, np.abs(entropy - target).max()


def given_p(rs, n):
    """the P of a gradient or loop case: the joint probabilities of Gaussian rows. Two points always have P = [[0, .5], [.5, 0]], for
    which attraction and repulsion cancel EXACTLY in any arithmetic that evaluates both the same way (g = 0, KL = e·log e, err32 = 0):
    nothing would be measured. The n = 2 case therefore takes an unnormalised P, which the formulas accept as they are."""
    if n == 2:
        return np.array([[0.0, 0.3], [0.3, 0.0]], dtype=np.float32)
    return tr.affinities(rows_of("gauss", rs, n, 6), perplexity_of(n))[0].astype(np.float32)


# ---- 2. gradient and KL ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_gradient_and_kl(n):
    rs = np.random.RandomState(77 + n)
    P = given_p(rs, n)
    base = rs.standard_normal((n, 2))
    for scale in (1e-4, 1.0, 30.0):
        for e in (1.0, 12.0):
            Y = (base * scale).astype(np.float32)
            g64, largest = tr.gradient(P, Y, e)
            g32, _ = tr.gradient(P, Y, e, np.float32)
            kl64, kl32 = tr.kl_divergence(P, Y, e), tr.kl_divergence(P, Y, e, np.float32)
            err32, kl_err32 = worst(g32, g64, largest[:, None]), abs(kl32 - kl64)
            g, kl = hook_gradient(P, Y, e)
            g2, kl2 = hook_gradient(P, Y, e)
            got = worst(g, g64, largest[:, None])
            print("tsne-error gradient n=%d scale %g e %g: err32 %.3g, max |g - g64| / largest term / err32 %.3g; KL %.6g err32 %.3g, |KL - KL64| / err32 %.3g"
                  % (n, scale, e, err32, got / max(err32, 1e-300), kl64, kl_err32, abs(kl - kl64) / max(kl_err32, 1e-300)))
            assert got <= 4 * err32
            assert abs(kl - kl64) <= 4 * kl_err32
            assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)) and kl == kl2      # two launches, the same bits


# ---- 3. PCA start ----------------------------------------------------------------------------------------------------------------------
def pca_rows(rs, n, d):
    """rows whose covariance has the eigenvalues 64, 16, 4, 1 (as many as n − 1 and d allow) on random axes, off-centre"""
    r = min(n - 1, d, 4)
    A = rs.standard_normal((n, r))
    A, _ = np.linalg.qr(A - A.mean(axis=0))
    B, _ = np.linalg.qr(rs.standard_normal((d, r)))
    return ((A * np.array([8.0, 4.0, 2.0, 1.0])[:r]) @ B.T + rs.standard_normal(d)).astype(np.float32)


@pytest.mark.parametrize("n,d", [(5, 6), (63, 36), (64, 256), (65, 300), (130, 6), (300, 36), (300, 256)])
def test_pca_start(n, d):
    X = pca_rows(np.random.RandomState(n + d), n, d)
    Y64, w = tr.pca_start(X)
    Y32, _ = tr.pca_start(X, np.float32)
    assert w[0] >= 1.5 * w[1] and w[1] >= 1.5 * w[2] > 0, w[:3]
    err32 = float(np.abs(Y32 - Y64).max())
    Y0 = np.full((n, 2), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_pca(ptr(X), n, d, ptr(Y0)))
    print("tsne-error pca n=%d d=%d: err32 %.3g, max |Y0 - Y64| / err32 %.3g" % (n, d, err32, np.abs(Y0 - Y64).max() / err32))
    assert np.abs(Y0 - Y64).max() <= 4 * err32
    assert abs(Y0[:, 0].astype(np.float64).std() - 1e-4) <= 1e-4 * 2.0 ** -23


def test_pca_start_with_one_column_and_identical_rows():
    X = np.random.RandomState(4).standard_normal((65, 1)).astype(np.float32)
    Y0 = np.full((65, 2), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_pca(ptr(X), 65, 1, ptr(Y0)))
    Y64, _ = tr.pca_start(X)
    assert np.abs(Y0 - Y64).max() <= 4 * float(np.abs(tr.pca_start(X, np.float32)[0] - Y64).max()) and not Y0[:, 1].any()
    same = np.ones((64, 36), dtype=np.float32) * 0.375
    assert ca.lib().nvsm_debug_tsne_pca(ptr(same), 64, 36, ptr(Y0)) == 1 and b"identical" in ca.lib().nvsm_last_error()


def test_pca_start_on_a_diagonal_covariance_with_tied_eigenvalues():
    """The solver's corners: a covariance that is diagonal already (no sweep runs), two EQUAL leading eigenvalues (the
    lower index comes first), axes whose entries tie in magnitude only with zeros (sign by the first largest entry: already
    positive), and a trailing zero eigenvalue. numpy's eigh may return any basis of a tied eigenspace, so the expected picture is
    written out: column 0 is coordinate 0, column 1 coordinate 1, both divided by np.std of column 0 and times 1e-4."""
    a = 3.0
    X = np.array([[a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, 0]], dtype=np.float32) + np.float32(0.5)
    Y0 = np.full((5, 2), GUARD, dtype=np.float32)
    check(ca.lib().nvsm_debug_tsne_pca(ptr(X), 5, 3, ptr(Y0)))
    centred = X[:, :2].astype(np.float64) - 0.5
    want = centred / centred[:, 0].std() * 1e-4
    assert np.abs(Y0 - want).max() <= 1e-4 * 2.0 ** -22
    # ... and the mirrored table gives the same axes, not their negatives
    check(ca.lib().nvsm_debug_tsne_pca(ptr(np.ascontiguousarray(X[::-1])), 5, 3, ptr(Y0)))
    assert np.abs(Y0 - want[::-1]).max() <= 1e-4 * 2.0 ** -22


# ---- 4. the loop -----------------------------------------------------------------------------------------------------------------------
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


VARIANTS = 6


def float32_runs(run, n):
    """The float32 numpy chain, VARIANTS times: run(perm) evaluates it on the inputs with their points relabelled by `perm` and
    returns (Y, KL); the pictures come back in the original order. Relabelling changes nothing but the order in which float32 sums
    run, so every variant is the same formula in float32. The KL of a run is ONE number: its deviation in one float32 run is a single
    draw (1.4e-8 at KL = 1.89 in the n = 65 loop case, a tenth of float32's rounding of the KL itself), so err32 of the KL is the
    largest deviation over the variants; the first variant is the identity, the chain every other err32 of this file comes from."""
    out = []
    for v in range(VARIANTS):
        perm = np.arange(n) if v == 0 else np.random.RandomState(1000 + v).permutation(n)
        Y, kl = run(perm)
        out.append((Y[np.argsort(perm)], kl))
    return out


@pytest.mark.parametrize("n,d", [(5, 6), (65, 36), (130, 300), (300, 16)])
def test_five_iterations_of_the_whole_call(n, d):
    rs = np.random.RandomState(n)
    X = rows_of("gauss", rs, n, d)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    perp = perplexity_of(n)
    Y64, kl64, it64 = tr.tsne(X, perplexity=perp, max_iter=5, init=Y0)
    runs = float32_runs(lambda perm: tr.tsne(X[perm], perplexity=perp, max_iter=5, init=Y0[perm], dtype=np.float32)[:2], n)
    m = table_model(X)
    Y, kl, it = m.tsne(perplexity=perp, max_iter=5, init=Y0)
    m.close()
    scale = np.abs(Y64).max()
    err32, kl_err32 = worst(runs[0][0], Y64, scale), max(abs(k - kl64) for _, k in runs)
    print("tsne-error call n=%d d=%d: err32 %.3g, max |Y - Y64| / extent / err32 %.3g; KL %.6g err32 %.3g (one run: %.3g), |KL - KL64| / err32 %.3g"
          % (n, d, err32, worst(Y, Y64, scale) / err32, kl64, kl_err32, abs(runs[0][1] - kl64), abs(kl - kl64) / kl_err32))
    assert it == it64 == 4 and worst(Y, Y64, scale) <= 4 * err32 and abs(kl - kl64) <= 4 * kl_err32


@pytest.mark.parametrize("n", NS)
def test_the_phase_boundary_through_the_hook(n):
    rs = np.random.RandomState(500 + n)
    P = given_p(rs, n)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    lr = np.float32(tr.auto_learning_rate(n))
    Y64, kl64, it64 = tr.descent(P, Y0, lr, 12.0, exploration=3, max_iter=5)
    runs = float32_runs(lambda perm: tr.descent(P[np.ix_(perm, perm)], Y0[perm], lr, 12.0, exploration=3, max_iter=5, dtype=np.float32)[:2], n)
    Y, kl, it = hook_descent(P, Y0, float(lr), 3, 5)
    scale = np.abs(Y64).max()
    err32, kl_err32 = worst(runs[0][0], Y64, scale), max(abs(k - kl64) for _, k in runs)
    print("tsne-error loop 3+2 n=%d: err32 %.3g, max |Y - Y64| / extent / err32 %.3g; KL %.6g err32 %.3g (one run: %.3g), |KL - KL64| / err32 %.3g"
          % (n, err32, worst(Y, Y64, scale) / max(err32, 1e-300), kl64, kl_err32, abs(runs[0][1] - kl64), abs(kl - kl64) / max(kl_err32, 1e-300)))
    assert it == it64 == 4 and worst(Y, Y64, scale) <= 4 * err32 and abs(kl - kl64) <= 4 * kl_err32


@pytest.fixture(scope="module")
def settled():
    """P of 130 Gaussian rows and a picture the fp64 reference has already run to its end (1 000 iterations): spread out and nearly
    converged, so that further iterations WITHOUT exaggeration stay where they are and float32 runs stay next to the fp64 one —
    from a 1e-4 start a hundred iterations are far into the chaotic regime and nothing about Y or the KL could be held."""
    n = 130
    rs = np.random.RandomState(9)
    P = tr.affinities(rows_of("gauss", rs, n, 6), 30.0)[0].astype(np.float32)
    Y0 = (1e-4 * rs.standard_normal((n, 2))).astype(np.float32)
    Y, _, _ = tr.descent(P, Y0, 50.0, 12.0, exploration=250, max_iter=1000)
    return P, Y.astype(np.float32)


def test_a_run_that_min_grad_norm_ends(settled):
    """min_grad_norm = 1e30 ends each phase at its first check: iterations 49 and 99 (early_exaggeration 1: the settled picture is
    the objective's own). Y, the KL and n_iter are the reference's."""
    P, Y0 = settled
    n = len(Y0)
    kw = dict(exploration=250, max_iter=1000, min_grad_norm=1e30)
    Y64, kl64, it64 = tr.descent(P, Y0, 50.0, 1.0, **kw)
    runs = float32_runs(lambda perm: tr.descent(P[np.ix_(perm, perm)], Y0[perm], np.float32(50.0), 1.0, dtype=np.float32, **kw)[:2], n)
    Y, kl, it = hook_descent(P, Y0, 50.0, 250, 1000, min_grad_norm=1e30, exaggeration=1.0)
    scale = np.abs(Y64).max()
    err32, kl_err32 = worst(runs[0][0], Y64, scale), max(abs(k - kl64) for _, k in runs)
    print("tsne-error loop min_grad_norm 50+50: err32 %.3g, max |Y - Y64| / extent / err32 %.3g; KL %.6g err32 %.3g (one run: %.3g), |KL - KL64| / err32 %.3g"
          % (err32, worst(Y, Y64, scale) / err32, kl64, kl_err32, abs(runs[0][1] - kl64), abs(kl - kl64) / kl_err32))
    assert err32 < 1e-4, "the run must stay out of the chaotic regime for the rule to say anything"
    assert it == it64 == 99 and worst(Y, Y64, scale) <= 4 * err32 and abs(kl - kl64) <= 4 * kl_err32
    # ... and with the exaggeration on, from the same start, the count is the reference's too (the pictures part ways)
    _, _, it64 = tr.descent(P, Y0, 50.0, 12.0, **kw)
    _, _, it = hook_descent(P, Y0, 50.0, 250, 1000, min_grad_norm=1e30)
    assert it == it64 == 99


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end():
    with open(os.path.join(ROOT, "tests", "golden", "tsne", "end_to_end.json")) as f:
        gold = json.load(f)
    X, labels = tr.clusters(np.random.RandomState(gold["seed"]), gold["n"], gold["d"], gold["clusters"], gold["spread"])
    m = table_model(X)
    yield gold, X, labels, tr.affinities(X, gold["perplexity"])[0], m
    m.close()


@pytest.mark.parametrize("init", ["pca", "random"])
def test_end_to_end_lands_in_the_references_band(end_to_end, init):
    gold, X, labels, P64, m = end_to_end
    kls = [r["kl"] for r in gold["runs"]]
    trusts = [r["trustworthiness"] for r in gold["runs"]]
    Y, kl_device, n_iter = m.tsne(perplexity=gold["perplexity"], max_iter=gold["max_iter"], init=init, random_state=0)
    kl, trust = tr.kl_divergence(P64, Y), tr.trustworthiness(X, Y, gold["n_neighbors"])      # fp64, from the RETURNED embedding
    print("tsne-error end to end %s: KL %.4f (reference runs %.4f .. %.4f; the device's own %.4f), trustworthiness %.4f (%.4f .. %.4f), n_iter %d"
          % (init, kl, min(kls), max(kls), kl_device, trust, min(trusts), max(trusts), n_iter))
    assert kl <= max(kls) + (max(kls) - min(kls))
    assert trust >= min(trusts) - (max(trusts) - min(trusts))
    assert tr.nearest_label_agreement(Y, labels) == 1.0
    assert n_iter == gold["max_iter"] - 1 and abs(kl_device - kl) <= 1e-3


# ---- 6. contract -------------------------------------------------------------------------------------------------------------------------
def test_a_repeated_call_returns_the_same_bits_and_rows_come_by_id(end_to_end):
    gold, X, labels, P64, m = end_to_end
    rs = np.random.RandomState(3)
    ids = rs.permutation(300)[:130].astype(np.int64)
    Y0 = (1e-4 * rs.standard_normal((130, 2))).astype(np.float32)
    kw = dict(ids=ids, max_iter=60, init=Y0, l2_normalize=True)
    a, b = m.tsne(**kw), m.tsne(**kw)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and a[1:] == b[1:]
    other = table_model(tr.l2_normalize(X[ids]))      # the same rows, already gathered and normalised, in a table of their own
    c = other.tsne(max_iter=60, init=Y0)
    other.close()
    assert np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32)) and a[1:] == c[1:]
    d = m.tsne(limit=130, max_iter=60, init=Y0)       # other rows: another picture
    assert not np.array_equal(a[0], d[0])
    e, f = m.tsne(limit=65, max_iter=10), m.tsne(limit=65, max_iter=10)      # the PCA start, and a smaller n behind a larger one
    assert np.array_equal(e[0].view(np.uint32), f[0].view(np.uint32)) and e[1:] == f[1:]


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
    got_e = a.tsne(ids=eids, max_iter=5, init=Y0)                   # straight behind nvsm_step
    got_w = a.tsne(space="words", ids=wids, max_iter=5, init=Y0[:65], perplexity=16.0)
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0 and np.abs(logical[W_NAME] - params[W_NAME]).max() > 0
    for got, X, perp, y0 in ((got_e, logical[E_NAME].reshape(-1, 36)[eids], 30.0, Y0), (got_w, logical[W_NAME].reshape(-1, 12)[wids], 16.0, Y0[:65])):
        Y64, kl64, _ = tr.tsne(X, perplexity=perp, max_iter=5, init=y0)
        Y32, _, _ = tr.tsne(X, perplexity=perp, max_iter=5, init=y0, dtype=np.float32)
        scale = np.abs(Y64).max()
        err32 = worst(Y32, Y64, scale)
        print("tsne-error lazy %s n=%d: err32 %.3g, ratio %.3g" % (method, len(X), err32, worst(got[0], Y64, scale) / err32))
        assert worst(got[0], Y64, scale) <= 4 * err32
    ten(10)
    for n in list(PARAMS) + ADAM_STATE:                       # b never called nvsm_tsne
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    a.close()
    b.close()


def raw_tsne(m, n_out=600, **fields):
    o = ca.NvsmTsneOptions()
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = ptr(v)
        setattr(o, k, v)
    out = np.full(n_out, GUARD, dtype=np.float32)
    kl, it = C.c_double(-5.0), C.c_int32(-5)
    st = ca.lib().nvsm_tsne(m._h, C.byref(o), ptr(out), C.byref(kl), C.byref(it))
    return st, ca.lib().nvsm_last_error(), (out == GUARD).all() and kl.value == -5.0 and it.value == -5


def test_refusals_are_status_codes_in_order_nothing_is_written_and_the_handle_still_works(end_to_end):
    gold, X, labels, P64, m = end_to_end
    nan, inf = float("nan"), float("inf")
    bad_ids = np.array([1, 300], dtype=np.int64)
    bad_init = np.zeros((300, 2), dtype=np.float32)
    bad_init[7, 1] = nan
    cases = [(dict(space=ca.SPACE_PROJECTED_WORDS), b"space"), (dict(space=9, num_rows=1), b"space"),
             (dict(num_rows=1, perplexity=nan), b"num_rows"), (dict(num_rows=301), b"num_rows"), (dict(num_rows=-4), b"num_rows"),
             (dict(ids=bad_ids, num_rows=2, perplexity=5.0), b"row id"), (dict(ids=np.array([-1, 2], dtype=np.int64), num_rows=2), b"row id"),
             (dict(perplexity=nan, early_exaggeration=nan), b"perplexity"), (dict(perplexity=0.0), b"perplexity"),
             (dict(perplexity=300.0), b"perplexity"), (dict(perplexity=inf), b"perplexity"),
             (dict(early_exaggeration=0.0, learning_rate=nan), b"early_exaggeration"), (dict(early_exaggeration=inf), b"early_exaggeration"),
             (dict(learning_rate=nan, max_iter=0), b"learning_rate"), (dict(min_grad_norm=inf, max_iter=0), b"min_grad_norm"),
             (dict(init=ca.TSNE_INIT_GIVEN, init_embedding=bad_init, max_iter=0), b"init_embedding"),
             (dict(max_iter=0, init=5), b"max_iter"), (dict(n_iter_without_progress=-1, init=5), b"n_iter_without_progress"),
             (dict(init=5), b"init"), (dict(init=ca.TSNE_INIT_GIVEN), b"init_embedding")]
    for fields, word in cases:
        st, msg, untouched = raw_tsne(m, **fields)
        assert st == 1 and word in msg and untouched, (fields, st, msg)
    big = table_model(np.zeros((ca.TSNE_MAX_ROWS + 1, 1), dtype=np.float32))
    st, msg, untouched = raw_tsne(big, n_out=8, perplexity=nan)
    big.close()
    assert st == 2 and b"rows" in msg and untouched                # NVSM_ERR_UNSUPPORTED, before the perplexity is looked at
    same = table_model(np.full((64, 6), 0.5, dtype=np.float32))
    st, msg, _ = raw_tsne(same, perplexity=10.0)
    same.close()
    assert st == 1 and b"identical" in msg                          # no principal axes: the PCA start fails, a given start does not
    Y, kl, it = m.tsne(limit=64, max_iter=3, perplexity=10.0)
    assert np.isfinite(Y).all() and np.isfinite(kl) and it == 2


def test_only_the_tsne_call_records_the_tsne_names(end_to_end):
    gold, X, labels, P64, m = end_to_end
    m.profile_enable(True)
    m.profile_reset()
    m.related_documents([1, 2], top_k=3)
    assert not [n for n in m.profile() if n.startswith("tsne_")]
    m.tsne(limit=64, max_iter=50, perplexity=10.0)
    names = {n for n in m.profile() if n.startswith("tsne_")}
    m.profile_enable(False)
    assert names == {"tsne_rows", "tsne_affinities", "tsne_pca", "tsne_forces", "tsne_update", "tsne_kl"}, names
