"""The checker of the pair objective checked on its own (no GPU): tests/pairs_reference.py's analytic gradient against central
differences of its cost, with the bound tests/test_oracle_gradcheck.py uses (eps = 1e-5, relative error < 1e-4 on every
parameter, cpp/gradient_check.cu:5-140), on data where neither clamp is active (|E[a]·E[b]| < 8); the two saturated cases
(dot = +-40: multiplier 0, the log of the clamp); and the table optimisers' treatment of one against two gradient lists."""
import numpy as np
import pytest

from tests import pairs_reference as ref

# the reference's own pair set, cpp/gradient_checking_tests.cu:142-148
REFERENCE_PAIRS = [(0, 1, 1.0), (1, 2, 0.5), (2, 3, 1.0), (0, 2, 1.0), (1, 2, 1.0)]


def central_difference_check(E, pairs, weights, eps=1e-5, thresh=1e-4):
    fwd = ref.pair_forward(E, pairs, weights)
    pred = -ref.dense_gradient(E.shape, [(fwd["grad"], fwd["ids"])])        # gradient ASCENT on -cost (objective.cu:586-588)
    worst, failed = 0.0, 0
    for i in range(E.shape[0]):
        for t in range(E.shape[1]):
            Ep, Em = E.copy(), E.copy()
            Ep[i, t] += eps
            Em[i, t] -= eps
            approx = (ref.pair_cost(Ep, pairs, weights) - ref.pair_cost(Em, pairs, weights)) / (2 * eps)
            denom = max(abs(pred[i, t]), abs(approx))
            rel = abs(pred[i, t] - approx) / denom if denom > 0 else 0.0
            worst = max(worst, rel)
            failed += int(pred[i, t] * approx < 0 or rel >= thresh)
    return failed, worst


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_pair_gradient_against_central_differences(seed, weighted):
    rs = np.random.RandomState(seed)
    nD, de, M = 15, 4, 64
    E = rs.uniform(-1.4, 1.4, (nD, de))
    pairs = rs.randint(0, nD, (M, 2))
    pairs[0] = (3, 3)                      # a == b
    pairs[1] = pairs[2] = (4, 7)           # a repeated pair
    w = rs.uniform(0.0, 2.0, M) if weighted else None
    assert np.abs((E[pairs[:, 0]] * E[pairs[:, 1]]).sum(axis=1)).max() < 8.0      # neither clamp is active
    failed, worst = central_difference_check(E, pairs, w)
    assert failed == 0, worst


def test_reference_pair_set_gradient():
    rs = np.random.RandomState(5)
    E = rs.uniform(-1.0, 1.0, (4, 4))
    pairs = np.array([(a, b) for a, b, _ in REFERENCE_PAIRS] * 8)
    w = np.array([x for _, _, x in REFERENCE_PAIRS] * 8)
    failed, worst = central_difference_check(E, pairs, w)
    assert failed == 0, worst


def test_saturated_pairs():
    E = np.zeros((4, 4))
    E[0], E[1] = (2, 2, 2, 2), (5, 5, 5, 5)           # dot = +40
    E[2], E[3] = (2, 2, 2, 2), (-5, -5, -5, -5)       # dot = -40
    f = ref.pair_forward(E, [(0, 1), (2, 3)], [1.0, 1.0])
    hi, lo = np.float64(np.float32(1.0 - np.float64(np.float32(1e-7)))), np.float64(np.float32(1e-7))
    assert f["probs"][0] == hi and f["probs"][1] == lo
    assert np.all(f["multipliers"] == 0.0) and np.all(f["grad"] == 0.0)
    assert f["cost"] == -(np.log(hi) + np.log(lo)) / 2
    # just inside the derivative's clamp the multiplier is 1 - p
    E[1] = (1, 1, 1, 1)                                # dot = 8: p = 0.99966
    f = ref.pair_forward(E, [(0, 1)])
    assert f["multipliers"][0] == pytest.approx(1.0 - ref.sigmoid(8.0), rel=1e-12)


def test_mixture_scale_and_lambda():
    rs = np.random.RandomState(1)
    E = rs.uniform(-1, 1, (6, 8))
    pairs = rs.randint(0, 6, (10, 2))
    a, b = ref.pair_forward(E, pairs), ref.pair_forward(E, pairs, scale=0.3)
    assert np.allclose(b["grad"], 0.3 * a["grad"], rtol=1e-15) and b["cost"] == a["cost"]
    assert ref.scaled_lambda(0.1, M=10) == pytest.approx(0.01)
    assert ref.scaled_lambda(0.1, B=20, M=10) == pytest.approx((0.1 / 20 + 0.1 / 10) / 2)


@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_two_lists_are_one_decay_and_both_scatters(method):
    """CompositeGradients: the table takes ONE decay and one Adam step from both lists — the same as the concatenated list."""
    rs = np.random.RandomState(2)
    E = rs.uniform(-1, 1, (9, 4))
    g1, i1 = rs.normal(size=(12, 4)), rs.randint(0, 9, 12)
    g2, i2 = rs.normal(size=(6, 4)), rs.randint(0, 9, 6)
    two, one = ref.TableOptimizer(E, method), ref.TableOptimizer(E, method)
    for _ in range(3):
        two.update([(g1, i1), (g2, i2)], 0.01, 0.05)
        one.update([(np.concatenate([g1, g2]), np.concatenate([i1, i2]))], 0.01, 0.05)
    assert np.allclose(two.P, one.P, rtol=1e-13, atol=0)
    assert not np.allclose(two.P, E)


def test_sgd_without_decay_is_the_scatter():
    rs = np.random.RandomState(3)
    E = rs.uniform(-1, 1, (5, 4))
    f = ref.pair_forward(E, [(0, 1), (1, 1), (0, 1)], [1.0, 0.5, 2.0])
    o = ref.TableOptimizer(E, "sgd")
    o.update([(f["grad"], f["ids"])], 0.1, 0.0)
    assert np.allclose(o.P, E + 0.1 * ref.dense_gradient(E.shape, [(f["grad"], f["ids"])]), rtol=1e-15)


@pytest.mark.parametrize("method,message", [("adagrad", "Adagrad currently does not implement multiple gradients."),
                                            ("sparse_adam", "Sparse Adam currently does not implement multiple gradients.")])
def test_methods_the_reference_refuses_for_two_lists(method, message):
    E = np.ones((3, 2))
    g, i = np.ones((2, 2)), np.array([0, 1])
    o = ref.TableOptimizer(E, method)
    o.update([(g, i)], 0.1, 0.0)          # one list is fine
    with pytest.raises(RuntimeError, match=message):
        o.update([(g, i), (g, i)], 0.1, 0.0)
