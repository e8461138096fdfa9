"""No GPU: tests/loss_reference.py - the numpy restatement that tests/test_gpu_loss_shapes.py holds the loss kernels to - against
the pinned oracle, element by element. The restatement gets the oracle's own `pre` and parameters (in float64) and must return the
oracle's proj, probs, multipliers, grad_proj, grad_bias, bn_inv_std and cost.

Equal means: every element within 1e-12 of the tensor's largest magnitude. (An element's own magnitude is no
scale for it: grad_proj elements are sums of R products that cancel, and batch-norm's backward subtracts a column mean - a float64
evaluation in another order of additions moves such an element by 1e-16 of the TERMS, whatever is left of their sum.)"""
import numpy as np
import pytest

from tests import loss_reference as lr
from tests.helpers import PARAMS, load_params, oracle_model, random_batch, random_params
from tests.test_gpu_parity import SPECS

RTOL = 1e-12
CASES = [("lse", 96), ("nvsm", 128), ("tiny", 64), ("tiny_odd", 100), ("wide", 33), ("many_negatives", 48), ("k4_window1", 70),
         ("l2_entity", 64)]


def inputs_from_oracle(spec, o, params, ids, iw, B, dtype=np.float64):
    de = spec["entity_dim"]
    pre = o.get("pre").reshape(B, de)
    bn = bool(spec.get("batch_norm"))
    return lr.LossInputs(
        pre=pre.astype(dtype), E=params[PARAMS[1]].reshape(-1, de).astype(dtype), ids=ids.reshape(B, -1), bn=bn,
        bn_sums=lr.column_sums(pre) if bn else None, bias=params[PARAMS[3]].astype(dtype), inst_w=iw.astype(dtype),
        nonlinearity=1 if spec.get("nonlinearity", "tanh") == "hard_tanh" else 0, clip_sigmoid=spec.get("clip_sigmoid", True),
        bias_negative_samples=spec.get("bias_negative_samples", False), l2_entity=spec.get("l2_entity", False))


def close(name, got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert got.shape == want.shape, name
    scale = np.abs(want).max()
    err = np.abs(got - want)
    assert np.all(err <= RTOL * scale), (name, int(np.argmax(err)), err.max() / scale)


@pytest.mark.parametrize("name,B", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_oracle(name, B):
    spec = SPECS[name]
    rs = np.random.RandomState(29)
    params = random_params(spec, rs)
    o = oracle_model(spec)
    load_params(o, params, False)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    o.forward(words, ww, ids, iw)
    cost = o.get_cost()
    o.backward()
    inp = inputs_from_oracle(spec, o, params, ids, iw, B)
    ref = lr.loss_reference(inp, np.float64)
    R = inp.R
    sign = np.where(np.arange(R) == 0, 1.0, -1.0)
    close("proj", ref["proj"], o.get("proj"))
    close("probs", ref["probs"], o.get("probs"))
    close("multipliers", ref["coef"] * sign, o.get("multipliers"))      # (the oracle keeps |m| and negates the rows instead)
    close("grad_proj", lr.bn_backward(ref, inp) if inp.bn else ref["dy"], o.get("grad_proj"))
    close("grad_bias", ref["colsum_dy"], o.get("grad_bias"))
    if inp.bn:
        close("bn_inv_std", ref["bn_inv_std"], o.get("bn_inv_std"))
        close("bn_mean", ref["bn_mean"], o.get("bn_mean"))
    assert abs(-ref["loss"] / B - cost) <= RTOL * abs(cost)
    assert np.abs(ref["logits"]).max() < 30 and np.all(np.isfinite(ref["dy"]))


def test_float32_yardstick_is_a_float32_evaluation():
    """Every tensor of the float32 restatement is float32 and sits within a few float32 roundings of the float64 one: it is the same
    formulas, not another computation."""
    spec = SPECS["nvsm"]
    B = 64
    rs = np.random.RandomState(5)
    params = random_params(spec, rs)
    o = oracle_model(spec)
    load_params(o, params, False)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    o.forward(words, ww, ids, iw)
    inp = inputs_from_oracle(spec, o, params, ids, iw, B, dtype=np.float32)
    r64, r32 = lr.loss_reference(inp, np.float64), lr.loss_reference(inp, np.float32)
    for t in ("proj", "pp", "probs", "coef", "dy", "bn_mean", "bn_inv_std"):
        assert r32[t].dtype == np.float32 and r64[t].dtype == np.float64
        d = np.abs(r32[t] - r64[t]).max()
        assert 0 < d <= 1e-5 * np.abs(r64[t]).max(), (t, d)


def test_lazy_rows_get_their_factors_in_update_order_in_float32():
    rs = np.random.RandomState(3)
    E = rs.uniform(-1, 1, (6, 4)).astype(np.float32)
    decay = rs.uniform(0.9, 1.0, 128).astype(np.float32)
    now = 300
    stamp = np.array([300, 299, 237, 236, 173, 172], np.int32)      # lags 0, 1, 63, 64, 127, 128: the last one goes once round the ring
    got = lr.rows_up_to_date(E, stamp, decay, now)
    for r in range(6):
        row = E[r].copy()
        for u in range(stamp[r], now):
            row = (row * decay[u % 128]).astype(np.float32)
        np.testing.assert_array_equal(got[r], row)
    np.testing.assert_array_equal(got[0], E[0])
    with pytest.raises(AssertionError):
        lr.rows_up_to_date(E, np.array([171, 300, 300, 300, 300, 300], np.int32), decay, now)
