"""The checker of the term-pair objective checked on its own (no GPU): tests/term_pairs_reference.py against
  * central differences of the pair cost and of the mixed cost with respect to W (eps = 1e-5, relative error < 1e-4 on every
    element: the bound of tests/test_oracle_gradcheck.py, cpp/gradient_check.cu:5-140) — the text half of the mixed cost and its
    word gradient come from the fp64 oracle;
  * tests/pairs_reference.py's TableOptimizer on window-1 lists, at 1e-12 relative, every method;
  * a hand-computed two-entry example with a non-unit feature weight: the case that separates a v weighed by c·s (what the reference
    does, cpp/updates_adam.cu:242-252 with storage.cu:44-48) from c²·s;
  * the oracle's own windowed table updater (oracle.Reps), an independent statement of the same reference lines."""
import numpy as np
import pytest

from oracle import nvsm_oracle as orc
from tests import pairs_reference as pref
from tests import term_pairs_reference as ref
from tests.helpers import METHODS, PARAMS, oracle_model

W_NAME = PARAMS[0]


def relative_failures(pred, approx, thresh):
    denom = np.maximum(np.abs(pred), np.abs(approx))
    rel = np.where(denom > 0, np.abs(pred - approx) / np.where(denom > 0, denom, 1.0), 0.0)
    return int(((pred * approx < 0) | (rel >= thresh)).sum()), float(rel.max())


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("weighted", [False, True])
def test_pair_cost_central_differences_on_the_words_table(seed, weighted):
    rs = np.random.RandomState(seed)
    nV, dw, M, eps = 15, 5, 64, 1e-5
    W = rs.uniform(-1.2, 1.2, (nV, dw))
    pairs = rs.randint(0, nV, (M, 2))
    pairs[0] = (3, 3)
    pairs[1] = pairs[2] = (4, 7)
    w = rs.uniform(0.0, 2.0, M) if weighted else None
    assert np.abs((W[pairs[:, 0]] * W[pairs[:, 1]]).sum(axis=1)).max() < 8.0      # neither clamp is active
    f = ref.term_pair_forward(W, pairs, w)
    pred = -ref.dense_gradient(W.shape, [(f["grad"], f["ids"], 1, None)])          # gradient ASCENT on -cost
    approx = np.zeros_like(W)
    for i in range(nV):
        for t in range(dw):
            Wp, Wm = W.copy(), W.copy()
            Wp[i, t] += eps
            Wm[i, t] -= eps
            approx[i, t] = (ref.term_pair_cost(Wp, pairs, w) - ref.term_pair_cost(Wm, pairs, w)) / (2 * eps)
    failed, worst = relative_failures(pred, approx, 1e-4)
    assert failed == 0, worst


def test_mixed_cost_central_differences_on_the_words_table():
    """At equal weights the mean of the two costs is the cost whose gradient the weighted sum (shares 1/2, 1/2) of the two
    gradients is. Text half: the fp64 oracle (tanh, no batch-norm: smooth), whose grad_phrase is scattered with window 3 and the
    feature weights."""
    spec = dict(num_words=12, num_entities=9, word_dim=3, entity_dim=4, window=3, num_random=1, nonlinearity="tanh")
    rs = np.random.RandomState(4)
    B, M, eps = 48, 40, 1e-5
    o = oracle_model(spec)
    o.initialize(orc.Rng(3))
    W = rs.uniform(-0.9, 0.9, (12, 3))
    words = rs.randint(0, 12, B * 3)
    ww = rs.uniform(0.2, 2.0, B * 3)
    labels = rs.randint(0, 9, B)
    iw = rs.uniform(0.2, 2.0, B)
    ids = np.stack([labels, rs.randint(0, 9, B)], axis=1).ravel()
    pairs = rs.randint(0, 12, (M, 2))
    pw = rs.uniform(0.0, 2.0, M)

    def costs(Wx):
        o.set(W_NAME, Wx)
        o.forward(words, ww, ids, iw)
        return o.get_cost(), ref.term_pair_cost(Wx, pairs, pw)

    ct, cp = costs(W)
    o.backward()
    gphrase = o.get("grad_phrase").reshape(B, 3)
    f = ref.term_pair_forward(W, pairs, pw, scale=0.5)
    pred = -ref.dense_gradient(W.shape, [(0.5 * gphrase, words, 3, ww), (f["grad"], f["ids"], 1, None)])
    approx = np.zeros_like(W)
    for i in range(12):
        for t in range(3):
            Wp, Wm = W.copy(), W.copy()
            Wp[i, t] += eps
            Wm[i, t] -= eps
            approx[i, t] = (ref.mixed_cost(*costs(Wp)) - ref.mixed_cost(*costs(Wm))) / (2 * eps)
    failed, worst = relative_failures(pred, approx, 1e-4)
    assert failed == 0, worst
    assert ref.mixed_cost(ct, cp) == (ct + cp) / 2


@pytest.mark.parametrize("method", ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"])
def test_window_one_lists_are_the_table_optimizer(method):
    rs = np.random.RandomState(6)
    P0 = rs.uniform(-1, 1, (11, 6))
    a, b = ref.WindowedTableOptimizer(P0, method), pref.TableOptimizer(P0, method)
    two = method in ("sgd", "dense_adam", "full_adam")
    for step in range(3):
        g1, i1 = rs.normal(size=(14, 6)), rs.randint(0, 11, 14)
        g2, i2 = rs.normal(size=(5, 6)), rs.randint(0, 11, 5)
        lists = [(g1, i1), (g2, i2)] if two else [(g1, i1)]
        a.update([(g, i, 1, None) for g, i in lists], 0.01, 0.05)
        b.update(lists, 0.01, 0.05)
        np.testing.assert_allclose(a.P, b.P, rtol=1e-12, atol=0)
    for state in ("a", "m", "v"):
        if hasattr(b, state):
            np.testing.assert_allclose(getattr(a, state), getattr(b, state), rtol=1e-12, atol=0)


def test_hand_computed_two_entries_with_a_feature_weight():
    """One table row of two elements, dense_update Adam from zero state, lr 0.5, lambda 0. Text list: one gradient row (3, 4) over a
    window of 2 with weights (0.5, 1): entry 0 goes to row 0 with weight 0.5, entry 1 to row 1 (not looked at). Pair list: one
    multiplied row (1, 2), window 1, weight 1, to row 0.
      m[0] = 0.1·(0.5·(3, 4) + (1, 2)) = (0.25, 0.4)
      mean of squares: text (9 + 16)/2 = 12.5, pair (1 + 4)/2 = 2.5
      v[0] = 0.001·(0.5·12.5 + 2.5) = 0.00875           — weighed LINEARLY; weighing by the square would give 0.001·(0.25·12.5 + 2.5)
      bc   = sqrt(1 − 0.999)/(1 − 0.9)
      P[0] = P0 + 0.5·bc·m[0]/(sqrt(v[0]) + 1e-6)"""
    b1, b2, eps = np.float64(np.float32(0.9)), np.float64(np.float32(0.999)), np.float64(np.float32(1e-6))
    omb1, omb2 = np.float64(np.float32(1.0 - b1)), np.float64(np.float32(1.0 - b2))
    P0 = np.array([[0.3, -0.2], [0.1, 0.1]])
    o = ref.WindowedTableOptimizer(P0, "dense_adam")
    o.update([(np.array([[3.0, 4.0]]), [0, 1], 2, [0.5, 1.0]), (np.array([[1.0, 2.0]]), [0], 1, None)], 0.5, 0.0)
    m0 = omb1 * (0.5 * np.array([3.0, 4.0]) + np.array([1.0, 2.0]))
    v_linear = omb2 * (0.5 * 12.5 + 2.5)
    v_squared = omb2 * (0.25 * 12.5 + 2.5)
    np.testing.assert_allclose(o.m[0], m0, rtol=1e-14)
    assert o.v[0] == pytest.approx(v_linear, rel=1e-14) and abs(o.v[0] - v_squared) > 0.1 * v_linear
    bc = np.float64(np.float32(np.sqrt(1.0 - b2) / (1.0 - b1)))
    np.testing.assert_allclose(o.P[0], P0[0] + 0.5 * bc * m0 / (np.sqrt(v_linear) + eps), rtol=1e-14)
    # sgd with the same lists: the plain weighted scatter, one decay
    s = ref.WindowedTableOptimizer(P0, "sgd")
    s.update([(np.array([[3.0, 4.0]]), [0, 1], 2, [0.5, 1.0]), (np.array([[1.0, 2.0]]), [0], 1, None)], 0.5, 0.25)
    decay = np.float64(np.float32(1.0 - 0.25 * 0.5))
    np.testing.assert_allclose(s.P[0], P0[0] * decay + 0.5 * (0.5 * np.array([3.0, 4.0]) + np.array([1.0, 2.0])), rtol=1e-14)
    np.testing.assert_allclose(s.P[1], P0[1] * decay + 0.5 * 1.0 * np.array([3.0, 4.0]), rtol=1e-14)


@pytest.mark.parametrize("method", ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"])
def test_windowed_lists_against_the_oracles_table_updater(method):
    """oracle.Reps restates the same reference lines in C++; tables are [dim][n] column-major there as in the reference, which for
    get() / set() is the row-major [n][dim] array used here. The helper rounds the decay, 1 − β₁, 1 − β₂, the bias correction and ε
    to float32 where the float32 build does (pairs_reference.TableOptimizer); the fp64 oracle keeps them in double. Each constant then
    differs by at most 2⁻²⁴ relative and enters an update linearly (the square root of v halves it): three updates of at most five
    constants are 15·2⁻²⁴ = 9e-7, taken relative to the table's largest element (about 1)."""
    rs = np.random.RandomState(8)
    n, d, win = 13, 4, 3
    P0 = rs.uniform(-1, 1, (n, d))
    reps = orc.Reps(n, d, *METHODS[method])
    reps.set(P0)
    opt = ref.WindowedTableOptimizer(P0, method)
    two = method in ("sgd", "dense_adam", "full_adam")
    for step in range(3):
        g1, i1, w1 = rs.normal(size=(6, d)), rs.randint(0, n, 6 * win), rs.uniform(0.1, 2.0, 6 * win)
        g2, i2 = rs.normal(size=(5, d)), rs.randint(0, n, 5)
        lists = [(g1, i1, win, w1)] + ([(g2, i2, 1, None)] if two else [])
        reps.update([(g.ravel(), i, w, x) for g, i, w, x in lists], 0.01, 0.05)
        opt.update(lists, 0.01, 0.05)
        np.testing.assert_allclose(opt.P.ravel(), reps.get(0), rtol=0, atol=15 * 2.0 ** -24)


def test_refusals_of_two_lists():
    o = ref.WindowedTableOptimizer(np.ones((3, 2)), "adagrad")
    with pytest.raises(RuntimeError, match="Adagrad currently does not implement multiple gradients."):
        o.update([(np.ones((1, 2)), [0, 1], 2, None), (np.ones((1, 2)), [0], 1, None)], 0.1, 0.0)
    o = ref.WindowedTableOptimizer(np.ones((3, 2)), "sparse_adam")
    with pytest.raises(RuntimeError, match="Sparse Adam currently does not implement multiple gradients."):
        o.update([(np.ones((1, 2)), [0, 1], 2, None), (np.ones((1, 2)), [0], 1, None)], 0.1, 0.0)
