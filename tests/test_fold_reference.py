"""CPU: the numpy restatement of a fold-in step (tests/fold_reference.py) against the fp64 oracle.

The feature is DEFINED as "the oracle's full step, then W, T, b and the frozen rows of E put back" (oracle_fold_step). The rows that
train, and their optimiser state, must then equal the restatement's row formulas — which is what nvsm_step_fold implements on the
device — to fp64 rounding, over three steps, for the five update methods and λ ∈ {0, 0.01}.

The bound is relative 1e-12 (norm-wise, per tensor). The oracle adds a row's entries into the row one at a time, in batch order,
where the restatement forms the row's sum first: the two differ by a few roundings of 1.1e-16 per entry, times the cancellation of
a sum of signed terms (a positive against up to k negatives) — four orders of magnitude of room at these shapes."""
import numpy as np
import pytest

from tests import fold_reference as fr
from tests.helpers import PARAMS, load_params, oracle_model, random_batch, random_params

SPEC = dict(num_words=50, num_entities=30, word_dim=7, entity_dim=5, window=3, num_random=4, nonlinearity="hard_tanh", batch_norm=True)
N0, B, STEPS, TOL = 20, 96, 3, 1e-12


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("lam", [0.0, 0.01])
@pytest.mark.parametrize("method", fr.METHOD_NAMES)
def test_restatement_equals_full_step_then_restore(method, lam):
    spec = dict(SPEC, update_method=method)
    spec["lambda"] = lam
    nD, de, R = spec["num_entities"], spec["entity_dim"], spec["num_random"] + 1
    rs = np.random.RandomState(7)
    params = random_params(spec, rs)
    o = oracle_model(spec)
    load_params(o, params, False)
    lr = {"sgd": 0.1, "adagrad": 0.01}.get(method, 0.001)
    P = o.get(fr.E).reshape(nD, de).copy()
    state = {}
    for _, on, scalar in fr.oracle_state_names(method):
        key = "a" if method == "adagrad" else ("m" if on.endswith("s0") else "v")
        state[key] = o.get(on).copy() if scalar else o.get(on).reshape(nD, de).copy()
    frozen = {p: o.get(p).copy() for p in PARAMS}
    for step in range(STEPS):
        words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
        ids = ids.reshape(B, R)
        ids[:, 0] = np.where(np.arange(B) % 3 == 0, labels, N0 + np.arange(B) % (nD - N0 - 1))      # most positives on new rows, one new row without
        ids = ids.ravel()
        fr.oracle_fold_step(o, words, ww, ids, iw, N0, lr)
        g, q, cnt = fr.oracle_sums(o, ids, R, nD)
        fr.fold_update(method, P, state, g, q, cnt, N0, lr, o.scaled_regularization_lambda(), step + 1)
        got = o.get(fr.E).reshape(nD, de)
        assert _rel(P[N0:], got[N0:]) <= TOL, (step, _rel(P[N0:], got[N0:]))
        for _, on, scalar in fr.oracle_state_names(method):
            key = "a" if method == "adagrad" else ("m" if on.endswith("s0") else "v")
            ref = o.get(on) if scalar else o.get(on).reshape(nD, de)
            assert _rel(state[key][N0:], ref[N0:]) <= TOL, (step, on, _rel(state[key][N0:], ref[N0:]))
        # ... and the definition's other half: what is frozen is what it was
        for p in fr.FROZEN:
            np.testing.assert_array_equal(o.get(p), frozen[p])
        np.testing.assert_array_equal(o.get(fr.E)[:N0 * de], frozen[fr.E][:N0 * de])
    assert np.abs(got[N0:] - frozen[fr.E].reshape(nD, de)[N0:]).max() > 0      # the new rows did train


def test_grow_documents_keeps_the_old_rows_and_draws_glorot():
    """cunvsm_amd.grow_documents: W, T, b and the old rows unchanged; the new rows inside Glorot's bound of the GROWN table, drawn
    from minstd_rand0(seed) in row-major order (the first draw checked by hand: x1 = 16807·seed mod (2^31 − 1))."""
    import cunvsm_amd as ca
    spec = dict(SPEC)
    rs = np.random.RandomState(1)
    params = random_params(spec, rs)
    grown = ca.grow_documents(params, 12, seed=5)
    de, nD = spec["entity_dim"], spec["num_entities"]
    for p in fr.FROZEN:
        np.testing.assert_array_equal(grown[p], params[p])
    e = grown[fr.E]
    assert e.dtype == np.float32 and e.size == (nD + 12) * de
    np.testing.assert_array_equal(e[:nD * de], params[fr.E])
    bound = np.float32(np.sqrt(6.0 / (de + nD + 12)))
    fresh = e[nD * de:]
    assert np.all(np.abs(fresh) <= bound) and fresh.std() > 0.3 * bound
    u0 = np.float32(16807 * 5 - 1) / np.float32(2147483648.0)
    assert fresh[0] == np.float32(np.float64(np.float32(2) * bound) * (np.float64(u0) - 0.5))
    np.testing.assert_array_equal(ca.grow_documents(params, 12, seed=5)[fr.E], e)
    assert not np.array_equal(ca.grow_documents(params, 12, seed=6)[fr.E], e)
    np.testing.assert_array_equal(ca.grow_documents(params, 0, seed=5)[fr.E], params[fr.E])
