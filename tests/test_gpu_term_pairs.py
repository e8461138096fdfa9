"""-m gpu: the term-term similarity objective on the words table (pairs.hip, the words-table form) alone and mixed into the text
objective — nvsm_compute_cost_term_mixed / nvsm_step_term_mixed against tests/term_pairs_reference.py (fp64 numpy, held to central
differences, to the entity-side optimiser and to a hand-computed example by tests/test_term_pairs_reference.py).

Bounds of the kernel's own outputs (section 1) are forward error bounds, written out where they are used. Everything else uses the
project's stated fp32 tolerances as tests/test_gpu_pairs.py does (its lines 16-17): forward tensors and loss rel 2e-5, gradients rel-L2
2e-4, a parameter change after updates 5e-4 (5e-3 for the Adam modes)."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import pairs_reference as pref
from tests import term_pairs_reference as ref
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params, rel_err

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME = PARAMS[0], PARAMS[1], PARAMS[2]
FWD_TOL, GRAD_TOL = 2e-5, 2e-4                                                                           # tests/test_gpu_pairs.py:16
UPD_TOL = {"sgd": 5e-4, "adagrad": 5e-4, "sparse_adam": 5e-3, "dense_adam": 5e-3, "full_adam": 5e-3}     # tests/test_gpu_pairs.py:17
LR = {"sgd": 0.1, "adagrad": 0.01, "sparse_adam": 0.001, "dense_adam": 0.001, "full_adam": 0.001}
METHODS = ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"]
MIXED_METHODS = ["sgd", "dense_adam", "full_adam"]
STATE = {"sgd": [], "adagrad": ["/a"], "sparse_adam": ["/m", "/v"], "dense_adam": ["/m", "/v"], "full_adam": ["/m", "/v"]}
U = 2.0 ** -24      # unit roundoff of float32


def make_spec(nV, dw, method="sgd", lam=0.0, **kw):
    spec = dict(num_words=nV, num_entities=50, word_dim=dw, entity_dim=8, window=3, num_random=2, update_method=method)
    spec["lambda"] = lam
    spec.update(kw)
    return spec


def random_pairs(rs, nV, M, weighted=True):
    pairs = rs.randint(0, nV, (M, 2)).astype(np.int64)
    if M >= 5:
        pairs[1] = (pairs[1, 0], pairs[1, 0])          # a == b
        pairs[3] = pairs[2]                            # a repeated pair
    w = rs.uniform(0.0, 2.0, M).astype(np.float32) if weighted else None
    return pairs, w


def all_state(m, method):
    names = list(PARAMS) + [t + s for t in ("word_representations", "entity_representations") for s in STATE[method]]
    return {n: m.get_param(n) for n in names}


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)


def change_error(P, P0, R, updates=1):
    """|(P - P0) - (R - P0)|, the reference's change, and the floor of keeping the table in float32: every update rounds each
    element once (tests/test_gpu_pairs.py change_error)."""
    return np.linalg.norm(np.asarray(P, np.float64) - R), np.linalg.norm(R - P0), updates * U * np.linalg.norm(R)


def pairs_per_workgroup(dw):
    """pairs.hip: four waves of eight turns, 64 / G pairs per wave and turn; G lanes of V floats cover a row."""
    v = 4 if dw % 4 == 0 else 1
    cols = (dw + v - 1) // v
    g = 2
    while g < cols and g < 64:
        g *= 2
    return 4 * 8 * (64 // g)


# ---- 1. the kernel's outputs, pairs only --------------------------------------------------------------------------------------
# d_w: the smallest group (8), one float per lane (30), a ragged group (36), the 32-lane broadcast (128), a full wave (256), two column
# turns with a ragged second (300), four turns (1024). M: 1, 5, one more than a workgroup's pairs, 1 000.
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("dw", [8, 30, 36, 128, 256, 300, 1024])
def test_pairs_only_forward_multipliers_rows_and_mean_squares(dw, weighted):
    nV = 700
    Ms = [1, 5, pairs_per_workgroup(dw) + 1, 1000]
    m = gpu_model(make_spec(nV, dw), max(Ms))
    rs = np.random.RandomState(dw)
    W = (rs.uniform(-1, 1, (nV, dw)) * np.sqrt(3.0 / dw)).astype(np.float32)      # unit-variance rows: |dot| of a few units
    m.set_param(W_NAME, W)
    W64 = W.astype(np.float64)
    for M in Ms:
        pairs, w = random_pairs(rs, nV, M, weighted)
        m.compute_cost_term_mixed(None, ca.PairBatch(pairs, w))
        m.compute_gradients()
        f = ref.term_pair_forward(W, pairs, w)
        probs, mults = m.get_tensor("term_pair_probs"), m.get_tensor("term_pair_multipliers")
        rows, msq = m.get_tensor("grad_pair_word").reshape(2 * M, dw), m.get_tensor("term_pair_msq")
        cost = m.get_cost()
        a, b = pairs[:, 0], pairs[:, 1]
        # the dot product's forward error, d_w·u·Σ|x·y| (any summation order), through σ' <= 1/4; σ itself and its clamp: two roundings
        bound = 0.25 * dw * U * np.abs(W64[a] * W64[b]).sum(axis=1) + 2 * U
        perr = np.abs(probs.astype(np.float64) - f["probs"])
        # mult = ω·(1 − prob)/M·scale: the probability's error times ω/M·scale, plus the three roundings of the float32 expression
        omega = np.ones(M) if w is None else w.astype(np.float64)
        mbound = bound * omega / M + 3 * np.spacing(np.abs(f["multipliers"]).astype(np.float32)).astype(np.float64)
        merr = np.abs(mults.astype(np.float64) - f["multipliers"])
        print("term pairs dw=%d M=%d weighted=%d: probs err/bound %.3f, multipliers err/bound %.3f, cost rel %.2e" % (
            dw, M, weighted, (perr / bound).max(), (merr / mbound).max(), abs(cost - f["cost"]) / abs(f["cost"])))
        assert np.all(perr <= bound)
        assert np.all(merr <= mbound)
        assert abs(cost - f["cost"]) <= FWD_TOL * abs(f["cost"])
        assert m.get_tensor("pair_cost")[0] == np.float32(cost)
        # one float32 multiplication per element: nothing to tolerate
        np.testing.assert_array_equal(rows[0::2], mults[:, None] * W[b])
        np.testing.assert_array_equal(rows[1::2], mults[:, None] * W[a])
        # the sum of d_w squares, each rounded once, in any order, and the division by d_w: (d_w + 2)·u relative
        want = (rows.astype(np.float64) ** 2).sum(axis=1) / dw
        assert np.all(np.abs(msq.astype(np.float64) - want) <= (dw + 2) * U * want)
        assert m.scaled_regularization_lambda() == 0.0


def test_saturated_pairs_agree_with_the_reference_on_the_clamp_side():
    for dw in (8, 36, 300):
        nV = 6
        m = gpu_model(make_spec(nV, dw, lam=0.5), 8)
        W = np.zeros((nV, dw), np.float32)
        W[0, :4], W[1, :4] = 2.0, 5.0           # dot = +40
        W[2, :4], W[3, :4] = 2.0, -5.0          # dot = -40
        m.set_param(W_NAME, W)
        pairs = np.array([(0, 1), (2, 3)])
        f = ref.term_pair_forward(W, pairs)
        # (CPU) float32 and fp64 agree on the clamp side: σ(±40) in float32 is beyond the clamps, and so is the fp64 value
        p32 = pref.sigmoid(np.float32([40.0, -40.0])).astype(np.float32)
        p64 = pref.sigmoid(np.float64([40.0, -40.0]))
        hi, lo = np.float32(1.0 - np.float64(np.float32(1e-7))), np.float32(1e-7)
        assert p32[0] >= hi and p64[0] >= np.float64(hi) and p32[1] <= lo and p64[1] <= np.float64(lo)
        m.compute_cost_term_mixed(None, ca.PairBatch(pairs))
        m.compute_gradients()
        np.testing.assert_array_equal(m.get_tensor("term_pair_probs"), f["probs"].astype(np.float32))      # the float32 clamps themselves
        assert np.all(m.get_tensor("term_pair_multipliers") == 0.0) and np.all(m.get_tensor("grad_pair_word") == 0.0)
        assert np.all(m.get_tensor("term_pair_msq") == 0.0)
        assert abs(m.get_cost() - f["cost"]) <= FWD_TOL * abs(f["cost"])
        assert m.scaled_regularization_lambda() == pytest.approx(0.25)                                  # lambda / M


# ---- 2. updates -----------------------------------------------------------------------------------------------------------------
def reference_pair_set():
    data = []
    while len(data) < 3 * (1 << 10):                   # cpp/gradient_checking_tests.cu:142-148
        data += [(0, 1, 1.0), (1, 2, 0.5), (2, 3, 1.0), (0, 2, 1.0), (1, 2, 1.0)]
    data = data[:3072]
    return np.array([(a, b) for a, b, _ in data], np.int64), np.array([x for _, _, x in data], np.float32)


@pytest.mark.parametrize("lam", [0.0, 0.1])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fused", [False, True])
def test_reference_pair_set_updates(method, lam, fused):
    """Tolerances: tests/test_gpu_pairs.py::test_reference_pair_set_updates (UPD_TOL, its line 17; the first cost at FWD_TOL, line 16)."""
    nV, dw = 15, 4
    pairs, w = reference_pair_set()
    m = gpu_model(make_spec(nV, dw, method, lam), 4096)
    rs = np.random.RandomState(7)
    W0 = rs.uniform(-0.5, 0.5, (nV, dw)).astype(np.float32)
    m.set_param(W_NAME, W0)
    other = {p: m.get_param(p) for p in PARAMS if p != W_NAME}
    opt = ref.WindowedTableOptimizer(W0, method)
    sl = pref.scaled_lambda(lam, M=len(pairs))
    for step in range(3):
        f = ref.term_pair_forward(opt.P, pairs, w)
        opt.update([(f["grad"], f["ids"], 1, None)], LR[method], sl)
        if fused:
            c = m.step_term_mixed(None, ca.PairBatch(pairs, w), LR[method], want_cost=True)
        else:
            m.compute_cost_term_mixed(None, ca.PairBatch(pairs, w))
            assert m.scaled_regularization_lambda() == pytest.approx(sl, rel=1e-6)
            m.compute_gradients()
            c = m.get_cost()
            m.update(LR[method])
        if step == 0:
            assert abs(c - f["cost"]) <= FWD_TOL * abs(f["cost"])
    W = m.get_param(W_NAME).reshape(nV, dw)
    err = rel_err(W - W0, opt.P - W0)
    print("reference pair set on words %s lambda %.1f fused %d: parameter change rel %.2e" % (method, lam, fused, err))
    assert err < UPD_TOL[method]
    for p, v in other.items():                         # nothing else has a gradient (cpp/params.cu:304-307)
        np.testing.assert_array_equal(m.get_param(p), v, err_msg=p)
    assert not m.get_tensor("arrival_counters").any()


def mixed_case(method="sgd", lam=0.0, B=600, M=400, dw=12, seed=5, nV=900, bn=False, **kw):
    spec = make_spec(nV, dw, method, lam, entity_dim=16, num_entities=300, batch_norm=bn, nonlinearity="hard_tanh" if bn else "tanh", **kw)
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    pairs, pw = random_pairs(rs, nV, M)
    return spec, params, (words, ww, labels, iw, ids), (pairs, pw)


def make_batch(words, labels, ww, iw, on_device):
    if not on_device:
        return ca.Batch(words, labels, ww, iw), None
    import torch
    dev = torch.device("cuda", 0)
    t = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (words, labels, ww, iw)]
    return ca.Batch(*t), t


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("feature_weights", ["uniform", "non_uniform"])
@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("method", MIXED_METHODS)
def test_mixed_words_update_against_the_windowed_reference(method, lam, feature_weights, on_device):
    """The reference optimiser takes the GPU's own text-side grad_phrase (mixture scale included: the text path is held to the oracle
    elsewhere) with window w and the feature weights, and its own pair gradient with window 1 and weight 1: one decay, one Adam step.
    Non-uniform feature weights are what separates a v weighed linearly from one weighed by the square (dense_adam)."""
    spec, params, _, _ = mixed_case(method, lam)
    nV, dw, w, B, M = spec["num_words"], spec["word_dim"], spec["window"], 600, 400
    m = gpu_model(spec, B)
    load_params(m, params, True)
    opt = ref.WindowedTableOptimizer(params[W_NAME].reshape(nV, dw), method)
    rs = np.random.RandomState(9)
    scale = np.float32(0.3) / (np.float32(0.7) + np.float32(0.3))
    for step in range(3):
        words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
        if feature_weights == "uniform":
            ww = None
        pairs, pw = random_pairs(rs, nV, M)
        batch, keep = make_batch(words, labels, ww, iw, on_device)
        m.compute_cost_term_mixed(batch, ca.PairBatch(pairs, pw), (0.7, 0.3), entity_ids=ids)
        m.compute_gradients()
        Wnow = m.get_param(W_NAME).reshape(nV, dw)
        f = ref.term_pair_forward(Wnow, pairs, pw, scale=scale)
        assert rel_err(m.get_tensor("grad_pair_word"), f["grad"]) < GRAD_TOL
        mults = m.get_tensor("term_pair_multipliers")
        rows = m.get_tensor("grad_pair_word").reshape(2 * M, dw)
        np.testing.assert_array_equal(rows[0::2], mults[:, None] * Wnow[pairs[:, 1]])      # the backward product left the pair rows alone
        opt.P[...] = Wnow                                                                  # (follow the GPU's table: one update at a time)
        before = opt.P.copy()
        opt.update([(m.get_tensor("grad_phrase").reshape(B, dw), words, w, ww), (f["grad"], f["ids"], 1, None)], LR[method],
                   pref.scaled_lambda(lam, B, M))
        m.update(LR[method])
        err = rel_err(m.get_param(W_NAME).reshape(nV, dw) - before, opt.P - before)
        print("term-mixed %s lambda %.1f %s weights device %d step %d: words change rel %.2e" % (method, lam, feature_weights, on_device, step, err))
        assert err < UPD_TOL[method]
        del keep


# ---- 3. gradients and identities ------------------------------------------------------------------------------------------------
# Central differences as in tests/test_gpu_pairs.py (its lines 149-153): step 2^-6 on parameters on that grid, rel-L2 < 2e-3.
FD_STEP, FD_TOL = 2.0 ** -6, 2e-3


def central_differences(m, name, forward):
    n = m.get_param(name).size
    out = np.zeros(n)
    for i in range(n):
        m.increment_parameter(name, i, FD_STEP)
        forward()
        cp = m.get_cost_f64()
        m.increment_parameter(name, i, -2 * FD_STEP)
        forward()
        cm = m.get_cost_f64()
        m.increment_parameter(name, i, FD_STEP)
        out[i] = (cp - cm) / (2 * FD_STEP)
    return out


def test_central_differences_pairs_only():
    nV, dw, M = 15, 4, 1024
    rs = np.random.RandomState(3)
    m = gpu_model(make_spec(nV, dw), M)
    W = (np.round(rs.uniform(-0.5, 0.5, (nV, dw)) * 64) / 64).astype(np.float32)
    m.set_param(W_NAME, W)
    pairs = rs.randint(0, 11, (M, 2))
    pb = ca.PairBatch(pairs, rs.uniform(0, 2, M).astype(np.float32))
    forward = lambda: m.compute_cost_term_mixed(None, pb)
    forward(); m.compute_gradients()
    g = m.get_tensor("grad_pair_word").reshape(2 * M, dw)
    pred = -ref.dense_gradient((nV, dw), [(g, pairs.reshape(-1), 1, None)]).ravel()
    approx = central_differences(m, W_NAME, forward)
    np.testing.assert_array_equal(m.get_param(W_NAME), W.ravel())
    print("central differences, term pairs only: rel-L2 %.2e" % rel_err(pred, approx))
    assert rel_err(pred, approx) < FD_TOL


def test_central_differences_mixed_equal_weights():
    """At equal weights the mean of the two costs IS the cost whose gradient the weighted sum of the gradients is."""
    spec = dict(num_words=20, num_entities=15, word_dim=3, entity_dim=4, window=3, num_random=1, update_method="sgd", nonlinearity="tanh")
    B, M = 256, 256
    rs = np.random.RandomState(11)
    m = gpu_model(spec, B)
    params = random_params(spec, rs, scale=0.5)
    params = {k: (np.round(v * 64) / 64).astype(np.float32) for k, v in params.items()}
    load_params(m, params, True)
    words = rs.randint(0, 11, B * 3).astype(np.int64)
    ww = rs.uniform(0, 2, B * 3).astype(np.float32)
    labels = rs.randint(0, 11, B).astype(np.int64)
    iw = rs.uniform(0, 2, B).astype(np.float32)
    ids = np.stack([labels, rs.randint(0, 15, B)], axis=1).astype(np.int64).ravel()
    pairs = rs.randint(0, 11, (M, 2))
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, rs.uniform(0, 2, M).astype(np.float32))
    forward = lambda: m.compute_cost_term_mixed(batch, pb, (1.0, 1.0), entity_ids=ids)
    forward(); m.compute_gradients()
    dw, de = 3, 4
    gW = ref.dense_gradient((20, dw), [(m.get_tensor("grad_phrase").reshape(B, dw), words, 3, ww),
                                        (m.get_tensor("grad_pair_word").reshape(-1, dw), pairs.reshape(-1), 1, None)])
    gE = pref.dense_gradient((15, de), [(m.get_tensor("grad_entity").reshape(-1, de), ids)])
    pred = {PARAMS[0]: -gW.ravel(), PARAMS[1]: -gE.ravel(), PARAMS[2]: -m.get_tensor("grad_transform").astype(np.float64),
            PARAMS[3]: -m.get_tensor("grad_bias").astype(np.float64)}
    for name in PARAMS:
        approx = central_differences(m, name, forward)
        print("central differences, term-mixed (1, 1): %s rel-L2 %.2e" % (name, rel_err(pred[name], approx)))
        assert rel_err(pred[name], approx) < FD_TOL, name


@pytest.mark.parametrize("variant", ["plain", "batch_norm", "l2_phrase"])
def test_mixed_tensors_are_the_weighted_tensors(variant):
    lam = 0.2
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case(lam=lam, bn=variant == "batch_norm", l2_phrase=variant == "l2_phrase")
    B, M = labels.size, len(pairs)
    m = gpu_model(spec, B)
    load_params(m, params, True)
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    m.compute_cost(batch, ids); m.compute_gradients()
    text = {n: m.get_tensor(n) for n in ("grad_transform", "grad_bias", "grad_phrase", "multipliers", "grad_entity", "probs", "proj")}
    text_cost = m.get_cost()
    m.compute_cost_term_mixed(None, pb); m.compute_gradients()
    pair_grad, pair_cost = m.get_tensor("grad_pair_word"), m.get_cost()
    m.compute_cost_term_mixed(batch, pb, (0.7, 0.3), entity_ids=ids); m.compute_gradients()
    for n in ("grad_transform", "grad_bias", "grad_phrase", "multipliers", "grad_entity"):
        err = rel_err(m.get_tensor(n), np.float32(0.7) * text[n])
        print("term-mixed (0.7, 0.3) %s: %s against 0.7 x text-only rel %.2e" % (variant, n, err))
        assert err < GRAD_TOL, n
    for n in ("probs", "proj"):
        np.testing.assert_array_equal(m.get_tensor(n), text[n], err_msg=n)
    assert rel_err(m.get_tensor("grad_pair_word"), np.float32(0.3) * pair_grad) < GRAD_TOL
    assert abs(m.get_cost() - (text_cost + pair_cost) / 2) <= FWD_TOL * abs(text_cost + pair_cost) / 2
    assert abs(m.get_tensor("text_cost")[0] - text_cost) <= FWD_TOL * abs(text_cost)
    assert m.get_tensor("pair_cost")[0] == np.float32(pair_cost)
    assert m.scaled_regularization_lambda() == pytest.approx((lam / B + lam / M) / 2, rel=1e-6)
    # ... and a text-only call afterwards is the text-only result again, bit for bit
    m.compute_cost(batch, ids); m.compute_gradients()
    for n in text:
        np.testing.assert_array_equal(m.get_tensor(n), text[n], err_msg=n)
    assert m.get_cost() == text_cost


def test_mixed_sgd_step_documents_and_projection_see_the_text_share_only():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case()
    B = labels.size
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    after = {}
    for kind in ("text", "pairs", "mixed"):
        m = gpu_model(spec, B)
        load_params(m, params, True)
        if kind == "text":
            m.compute_cost(batch, ids)
        elif kind == "pairs":
            m.compute_cost_term_mixed(None, pb)
        else:
            m.compute_cost_term_mixed(batch, pb, (0.7, 0.3), entity_ids=ids)
        m.compute_gradients(); m.update(0.1)
        after[kind] = {p: m.get_param(p).astype(np.float64) - params[p].ravel() for p in PARAMS}
    want = 0.7 * after["text"][W_NAME] + 0.3 * after["pairs"][W_NAME]
    print("term-mixed sgd: dW against 0.7 dW_text + 0.3 dW_pairs rel %.2e" % rel_err(after["mixed"][W_NAME], want))
    assert rel_err(after["mixed"][W_NAME], want) < UPD_TOL["sgd"]
    for p in PARAMS:
        if p != W_NAME:
            # both changes are differences of float32 tables, each element rounded once by its update: the floor of change_error, twice
            # (the projection moves by 1e-5 of elements of 0.3, whose ulp is 3e-8: the change itself is known to 3e-3 per element)
            err = np.linalg.norm(after["mixed"][p] - 0.7 * after["text"][p])
            floor = 2 * U * np.linalg.norm(params[p].astype(np.float64))
            print("term-mixed sgd: %s error %.3e, change %.3e, float32 floor %.3e" % (p, err, np.linalg.norm(0.7 * after["text"][p]), floor))
            assert err <= UPD_TOL["sgd"] * np.linalg.norm(0.7 * after["text"][p]) + floor, p
            assert not after["pairs"][p].any(), p


# ---- 4. row shapes and table sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_one_word_in_20000_pairs_takes_both_chunk_levels(mixed):
    nV, dw, M = 3000, 32, 20000
    spec = make_spec(nV, dw, "sgd", 0.05)
    rs = np.random.RandomState(13)
    params = random_params(spec, rs)
    m = gpu_model(spec, M)
    load_params(m, params, True)
    pairs = np.stack([np.full(M, 7), rs.randint(0, nV, M)], axis=1)
    pairs[::3] = pairs[::3, ::-1]                       # the hot word on either side
    pw = rs.uniform(0, 2, M).astype(np.float32)
    W0 = params[W_NAME].reshape(nV, dw)
    opt = ref.WindowedTableOptimizer(W0, "sgd")
    if mixed:
        B = 512
        words, ww, labels, iw, ids = random_batch(spec, rs, B)
        words[::5] = 7
        m.compute_cost_term_mixed(ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw), (0.5, 0.5), entity_ids=ids)
        m.compute_gradients()
        f = ref.term_pair_forward(W0, pairs, pw, scale=0.5)
        lists = [(m.get_tensor("grad_phrase").reshape(B, dw), words, 3, ww), (f["grad"], f["ids"], 1, None)]
        sl = pref.scaled_lambda(0.05, B, M)
    else:
        m.compute_cost_term_mixed(None, ca.PairBatch(pairs, pw))
        m.compute_gradients()
        f = ref.term_pair_forward(W0, pairs, pw)
        lists = [(f["grad"], f["ids"], 1, None)]
        sl = pref.scaled_lambda(0.05, M=M)
    assert np.bincount(np.concatenate([np.asarray(l[1]) for l in lists]))[7] > 64 * 32      # more than kFan level-1 chunks: level 2 is taken
    opt.update(lists, 0.1, sl)
    m.update(0.1)
    W = m.get_param(W_NAME).reshape(nV, dw)
    print("hot word (mixed %d): row 7 change rel %.2e" % (mixed, rel_err(W[7] - W0[7], opt.P[7] - W0[7])))
    assert rel_err(W[7] - W0[7], opt.P[7] - W0[7]) < UPD_TOL["sgd"]
    err, change, floor = change_error(W, W0, opt.P)
    assert err <= UPD_TOL["sgd"] * change + floor
    assert not m.get_tensor("arrival_counters").any()


@pytest.mark.parametrize("entry_walk_min", [None, "0"])
@pytest.mark.parametrize("method", ["sgd", "sparse_adam"])
def test_words_table_much_larger_than_the_batch(method, entry_walk_min, monkeypatch):
    if entry_walk_min is not None:
        monkeypatch.setenv("NVSM_ENTRY_WALK_MIN", entry_walk_min)
    nV, dw, M = 120000, 64, 3000
    spec = make_spec(nV, dw, method, 0.02)
    rs = np.random.RandomState(17)
    m = gpu_model(spec, M)
    W0 = (rs.uniform(-1, 1, (nV, dw)) * 0.2).astype(np.float32)
    m.set_param(W_NAME, W0)
    opt = ref.WindowedTableOptimizer(W0, method)
    m.profile_enable(True)
    for step in range(2):
        pairs, pw = random_pairs(rs, nV, M)
        pairs[:40, 0] = 11                              # a row of a few dozen entries among rows of one or two
        f = ref.term_pair_forward(opt.P, pairs, pw)
        opt.update([(f["grad"], f["ids"], 1, None)], LR[method], pref.scaled_lambda(0.02, M=M))
        m.step_term_mixed(None, ca.PairBatch(pairs, pw), LR[method])
    prof = m.profile()
    assert "term_pair_loss" in prof and "pair_loss" not in prof and "row_pass_entities" not in prof
    W = m.get_param(W_NAME).reshape(nV, dw)
    touched = np.unique(f["ids"])
    err, change, floor = change_error(W[touched], W0[touched], opt.P[touched], updates=2)
    print("large words table %s entry_walk_min %s: touched rows' error %.3e, change %.3e, float32 floor %.3e" % (method, entry_walk_min, err, change, floor))
    assert err <= UPD_TOL[method] * change + floor
    assert rel_err(W, opt.P) < 1e-6


# ---- 5. bit-for-bit identities --------------------------------------------------------------------------------------------------
def mixed_run(m, spec, steps, seed, fused=lambda s: s % 2 == 0, text_only=lambda s: False, pairs_only=lambda s: False,
              entity_pairs=lambda s: False, B=40, M=24, weights=(0.6, 0.4), terms=True):
    """A sequence of steps of mixed sizes; terms False: the same sequence with every term-pair step left out (the pairs drawn all the same)."""
    rs = np.random.RandomState(seed)
    for s in range(steps):
        b, mm = int(rs.choice([1, 7, B])), int(rs.choice([1, 5, M]))
        words, ww, labels, iw, ids = random_batch(spec, rs, b, zipf=True)
        pairs, pw = random_pairs(rs, min(spec["num_words"], spec["num_entities"]), mm)
        lr = float(rs.choice([1e-3, 5e-3, 2e-2]))
        batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
        if text_only(s):
            if fused(s):
                m.step(batch, lr, entity_ids=ids)
            else:
                m.compute_cost(batch, ids); m.compute_gradients(); m.update(lr)
        elif entity_pairs(s):
            if fused(s):
                m.step_mixed(batch, pb, lr, weights, entity_ids=ids)
            else:
                m.compute_cost_mixed(batch, pb, weights, entity_ids=ids); m.compute_gradients(); m.update(lr)
        elif not terms:
            continue
        elif pairs_only(s):
            if fused(s):
                m.step_term_mixed(None, pb, lr)
            else:
                m.compute_cost_term_mixed(None, pb); m.compute_gradients(); m.update(lr)
        elif fused(s):
            m.step_term_mixed(batch, pb, lr, weights, entity_ids=ids)
        else:
            m.compute_cost_term_mixed(batch, pb, weights, entity_ids=ids); m.compute_gradients(); m.update(lr)
    return m


@pytest.mark.parametrize("method,pairs_only", [("sgd", False), ("sgd", True), ("adagrad", True), ("sparse_adam", True)])
def test_lazily_decayed_tables_equal_the_eager_twin(method, pairs_only, monkeypatch):
    spec = make_spec(5000, 16, method, 0.05, num_entities=3000, entity_dim=16)
    params = random_params(spec, np.random.RandomState(2))
    monkeypatch.setenv("NVSM_LAZY_DECAY", "0")
    eager = gpu_model(spec, 40)
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    lazy = gpu_model(spec, 40)
    for m in (eager, lazy):
        load_params(m, params, True)
        mixed_run(m, spec, 6, 31, pairs_only=lambda s: pairs_only)
    assert "words lazy" in lazy.describe() and "words eager" in eager.describe()
    assert_same_bits(all_state(eager, method), all_state(lazy, method))
    # ... and over more than one of the periodic whole-table refreshes
    for m in (eager, lazy):
        mixed_run(m, spec, 140, 32, pairs_only=lambda s: pairs_only)
    assert_same_bits(all_state(eager, method), all_state(lazy, method))


@pytest.mark.parametrize("method", MIXED_METHODS)
def test_three_launch_pass_equals_the_one_launch_pass(method, monkeypatch):
    spec = make_spec(300, 16, method, 0.05, num_entities=300, entity_dim=16)
    params = random_params(spec, np.random.RandomState(2))
    results = []
    for merged in ("1", "0"):
        monkeypatch.setenv("NVSM_MERGED_PASS", merged)
        m = gpu_model(spec, 256)
        load_params(m, params, True)
        mixed_run(m, spec, 8, 33, B=256, M=256)
        results.append(all_state(m, method))
    assert_same_bits(*results)


@pytest.mark.parametrize("B,M", [(64, 48), (2048, 3000)])
@pytest.mark.parametrize("method", MIXED_METHODS)
def test_fused_step_equals_the_three_calls(method, B, M):
    spec = make_spec(500, 16, method, 0.05, num_entities=500, entity_dim=32)
    params = random_params(spec, np.random.RandomState(4))
    results = []
    for fused in (True, False):
        m = gpu_model(spec, max(B, M))
        load_params(m, params, True)
        mixed_run(m, spec, 12, 43, fused=lambda s: fused, B=B, M=M)
        results.append(all_state(m, method))
    assert_same_bits(*results)


def test_costs_of_the_fused_step_equal_the_three_calls():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case(lam=0.1)
    costs = []
    for fused in (True, False):
        m = gpu_model(spec, labels.size)
        load_params(m, params, True)
        batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
        if fused:
            costs.append(m.step_term_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids, want_cost=True))
        else:
            m.compute_cost_term_mixed(batch, pb, (0.7, 0.3), entity_ids=ids); m.compute_gradients()
            costs.append(m.get_cost()); m.update(0.01)
    assert costs[0] == costs[1]


@pytest.mark.parametrize("method", MIXED_METHODS)
def test_200_mixed_steps_twice_are_bit_equal(method):
    spec = make_spec(400, 16, method, 0.05, num_entities=400, entity_dim=32)
    params = random_params(spec, np.random.RandomState(4))
    results = []
    for run in range(2):
        m = gpu_model(spec, 128)
        load_params(m, params, True)
        mixed_run(m, spec, 200, 41, fused=lambda s: True, B=128, M=128)
        results.append(all_state(m, method))
        assert not m.get_tensor("arrival_counters").any()
    assert_same_bits(*results)


@pytest.mark.parametrize("method", METHODS)
def test_text_only_after_term_pair_calls_equals_a_handle_that_never_made_one(method):
    """The first term-pair call replaces the words update's source buffers and the words CSR workspace; text-only steps afterwards
    must produce the bits of a handle that never made one. The term-pair calls here are forward / backward passes (they leave the
    parameters, the optimiser state and its step counters alone); with sgd, which has no state, whole steps as well, the parameters
    loaded again afterwards."""
    spec = make_spec(400, 16, method, 0.05, num_entities=400, entity_dim=32)
    params = random_params(spec, np.random.RandomState(4))
    rs = np.random.RandomState(8)
    words, ww, labels, iw, ids = random_batch(spec, rs, 96, zipf=True)
    pairs, pw = random_pairs(rs, 400, 80)
    seen, fresh = gpu_model(spec, 96), gpu_model(spec, 96)
    load_params(seen, params, True)
    seen.compute_cost_term_mixed(None, ca.PairBatch(pairs, pw)); seen.compute_gradients(); seen.get_cost()
    if method in MIXED_METHODS:
        seen.compute_cost_term_mixed(ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw), (0.5, 0.5), entity_ids=ids)
        seen.compute_gradients(); seen.get_cost()
    if method == "sgd":
        mixed_run(seen, spec, 5, 48, B=96, M=96)
    for m in (seen, fresh):
        load_params(m, params, True)
        mixed_run(m, spec, 30, 49, text_only=lambda s: True, B=96, M=96)
    assert_same_bits(all_state(seen, method), all_state(fresh, method))
    assert "term pairs" in seen.describe() and "workspaces not allocated yet" in fresh.describe().split("term pairs:")[1]
    assert "workspaces not allocated yet" not in seen.describe().split("term pairs:")[1]


def test_entity_pair_steps_after_term_pair_calls_equal_a_handle_that_made_only_those():
    spec = make_spec(400, 16, "sgd", 0.05, num_entities=400, entity_dim=32)
    params = random_params(spec, np.random.RandomState(4))
    both, only = gpu_model(spec, 96), gpu_model(spec, 96)
    load_params(both, params, True)
    mixed_run(both, spec, 6, 50, B=96, M=96, pairs_only=lambda s: s % 2 == 1)         # term-pair steps first ...
    for m, terms in ((both, True), (only, False)):
        load_params(m, params, True)
        # ... then one sequence on both handles: entity-pair steps, with term-pair steps in between on `both` only, whose effect on the
        # parameters is undone by loading them again before the entity-pair steps that are compared
        mixed_run(m, spec, 8, 51, B=96, M=96, entity_pairs=lambda s: s % 2 == 0, terms=terms)
        load_params(m, params, True)
        mixed_run(m, spec, 20, 52, B=96, M=96, entity_pairs=lambda s: True)
    assert_same_bits(all_state(both, "sgd"), all_state(only, "sgd"))


# ---- 6. errors and memory -------------------------------------------------------------------------------------------------------
def status_of(fn):
    with pytest.raises(ca.NvsmError) as e:
        fn()
    return e.value.status, str(e.value)


def test_a_bad_word_id_is_reported_at_the_next_wait_and_the_handle_recovers():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case()
    B = labels.size
    batch = ca.Batch(words, labels, ww, iw)
    bad = pairs.copy()
    bad[17, 1] = spec["num_words"]
    worse = pairs.copy()
    worse[3, 0] = -1
    hit, fresh = gpu_model(spec, B), gpu_model(spec, B)
    load_params(hit, params, True)
    hit.step_term_mixed(batch, ca.PairBatch(bad, pw), 0.01, (0.7, 0.3), entity_ids=ids)
    st, msg = status_of(hit.synchronize)
    assert st == 1 and "word id" in msg
    hit.compute_cost_term_mixed(None, ca.PairBatch(worse, pw))
    st, msg = status_of(hit.get_cost)
    assert st == 1
    for m in (hit, fresh):
        load_params(m, params, True)
        for _ in range(3):
            m.step_term_mixed(batch, ca.PairBatch(pairs, pw), 0.01, (0.7, 0.3), entity_ids=ids)
        m.step(batch, 0.01, entity_ids=ids)
    assert_same_bits(all_state(hit, "sgd"), all_state(fresh, "sgd"))
    assert not hit.get_tensor("arrival_counters").any()


def test_refused_configurations_leave_the_handle_usable():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case()
    B = labels.size
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    L = ca.lib()
    import ctypes as C

    def raw(m, st, ps, mix):
        return L.nvsm_compute_cost_term_mixed(m._h, C.byref(st) if st is not None else None, ids.ctypes.data, C.byref(ps), C.byref(mix) if mix is not None else None)

    for method, sentence in (("adagrad", "Adagrad currently does not implement multiple gradients."),
                             ("sparse_adam", "Sparse Adam currently does not implement multiple gradients.")):
        m = gpu_model(dict(spec, update_method=method), B)
        load_params(m, params, True)
        for call in (lambda: m.compute_cost_term_mixed(batch, pb, (0.7, 0.3), entity_ids=ids), lambda: m.step_term_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids)):
            st, msg = status_of(call)
            assert st == 2 and sentence in msg
        m.step_term_mixed(None, pb, 0.01)                  # the pair objective alone exists for every method
        m.step(batch, 0.01, entity_ids=ids)
        assert np.isfinite(m.get_cost())
    m = gpu_model(spec, B, world_size=2, rank=0)
    st, msg = status_of(lambda: m.compute_cost_term_mixed(None, pb))
    assert st == 2 and "world_size" in msg
    # the dimension limit: beyond 256 the rows must be a multiple of 4; beyond 1024 nothing
    for dw in (258, 1028):
        m = gpu_model(make_spec(50, dw), 8)
        st, msg = status_of(lambda: m.compute_cost_term_mixed(None, ca.PairBatch([[0, 1]])))
        assert st == 2 and "word_repr_size up to 1024" in msg
        m.initialize(1)
        m.step(ca.Batch(np.zeros(3, np.int64), np.zeros(1, np.int64)), 0.01, entity_ids=np.zeros(3, np.int64))
        assert np.isfinite(m.get_cost())
    # invalid arguments: mixture weights, pair counts
    m = gpu_model(spec, B)
    load_params(m, params, True)
    st_b, ps = batch.as_struct(), pb.as_struct()
    for wt, wp in ((0.0, 1.0), (1.0, 0.0), (-0.5, 1.5)):
        assert raw(m, st_b, ps, ca.NvsmMixture(wt, wp)) == 1 and "must both be > 0" in L.nvsm_last_error().decode()
    for n in (0, -3, B + 1):
        ps_bad = pb.as_struct()
        ps_bad.num_pairs = n
        assert raw(m, None, ps_bad, None) == 1 and "num_pairs" in L.nvsm_last_error().decode()
    ps_null = pb.as_struct()
    ps_null.pairs = None
    assert raw(m, None, ps_null, None) == 1 and "pairs are required" in L.nvsm_last_error().decode()
    assert raw(m, st_b, ps, None) == 1 and "mix" in L.nvsm_last_error().decode()
    with pytest.raises(ca.NvsmError):
        m.get_tensor("term_pair_probs")                    # no forward result with pairs yet
    m.step_term_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids)
    assert "term pairs: term_pair_loss" in m.describe()
    # one call takes one kind: a term result has no entity-pair tensors and the other way round
    m.compute_cost_term_mixed(None, pb)
    st, msg = status_of(lambda: m.get_tensor("pair_probs"))
    assert st == 4
    m.compute_cost_mixed(None, ca.PairBatch(pairs % spec["num_entities"], pw))
    st, msg = status_of(lambda: m.get_tensor("term_pair_probs"))
    assert st == 4


def test_the_entry_id_bound_is_refused_with_a_sentence():
    """3 x max_batch_size x window_size must stay below 2^26: window 128 and a batch of 2^26 / 384 + 1 windows, on small tables."""
    spec = make_spec(20, 8, window=128)
    B = (1 << 26) // (3 * 128) + 1
    m = gpu_model(spec, B)
    st, msg = status_of(lambda: m.compute_cost_term_mixed(None, ca.PairBatch([[0, 1]])))
    assert st == 2 and "2^26" in msg
    m.initialize(1)
    m.step(ca.Batch(np.zeros(128, np.int64), np.zeros(1, np.int64)), 0.01, entity_ids=np.zeros(3, np.int64))
    assert np.isfinite(m.get_cost())


def test_memory_growth_of_the_first_call_at_the_headline_shape():
    """|V| = 50 k, |D| = 100 k, 300 -> 256, window 10, 16 negatives, batch 51 200, M = 51 200, dense_adam. The buffers the header lists,
    B = Mx = 51 200, w = 10, d_w = 300, 4-byte elements: gradient rows 2Mx·d_w (122.9 MB), means of squares 2Mx, word ids 2Mx, entry ids
    B·w + 2Mx, entry weights (B + 2Mx)·w, pair ids 2Mx·8 B, pair weights / probabilities / multipliers 3Mx, scaled instance weights B
    — and the words CSR workspace again for B·w + 2Mx entries, counted in full: per entry the two sorted arrays, the touched list and
    the sort's double buffers (6 ints), plus the chunk partials 2·entries/64·(d_w + 4) floats. On top the slack
    tests/test_gpu_pairs.py::test_memory_growth_at_the_headline_shape_stays_under_400_mb grants: it allows 400 MB where the pair rows it
    names are 2·M·d_e·4 = 104.9 MB, i.e. 295.1 MB beyond them. (Measured: 142.6 MB of growth against 133.9 MB listed + 38.1 MB of CSR.)"""
    import torch
    spec = dict(num_words=50000, num_entities=100000, word_dim=300, entity_dim=256, window=10, num_random=16, batch_norm=True,
                nonlinearity="hard_tanh", update_method="dense_adam")
    spec["lambda"] = 0.01
    B = M = 51200
    w, dw = 10, 300
    listed = 4 * (2 * M * dw + 2 * M + 2 * M + (B * w + 2 * M) + (B + 2 * M) * w + 3 * M + B) + 8 * 2 * M
    entries = B * w + 2 * M
    csr = 4 * (6 * entries + 2 * entries // 64 * (dw + 4))
    allowed = listed + csr + (400e6 - 2 * M * 256 * 4)
    m = gpu_model(spec, B, sampler=ca.SAMPLER_DEVICE)
    m.initialize(1)
    rs = np.random.RandomState(0)
    words, ww, labels, iw, _ = random_batch(spec, rs, B, zipf=True)
    pairs, pw = random_pairs(rs, spec["num_words"], M)
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    for _ in range(2):
        m.step(batch, 1e-3)
    m.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        m.step_term_mixed(batch, pb, 1e-3, (0.8, 0.2))
    m.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print("term-pairs memory: device memory in use grew by %.1f MB from the first term-mixed call on; listed %.1f MB + CSR %.1f MB, allowed %.1f MB" % (
        (free0 - free1) / 1e6, listed / 1e6, csr / 1e6, allowed / 1e6))
    assert np.isfinite(m.get_param(W_NAME)).all()
    assert free0 - free1 < allowed, (free0 - free1) / 1e6


# ---- 7. training effect ---------------------------------------------------------------------------------------------------------
def test_planted_pairs_pull_linked_words_together():
    """Words come in linked pairs (2i, 2i + 1) that never share a document; only the term pairs say they belong together. After the
    same number of steps from the same seed the linked words are closer in cosine (mean over the links) than unlinked words that
    never share a document either, (2i, 2(i + 7) + 1), in the mixed run, and closer than the same links in the text-only run."""
    nD, nV, w, B, M = 200, 400, 4, 512, 256
    spec = dict(num_words=nV, num_entities=nD, word_dim=32, entity_dim=32, window=w, num_random=4, batch_norm=True,
                nonlinearity="hard_tanh", update_method="dense_adam")
    spec["lambda"] = 0.0
    rs = np.random.RandomState(1)
    evens = np.arange(0, nV, 2)
    vocab_of = [rs.choice(evens, 6, replace=False) + (d % 2) for d in range(nD)]       # even documents write even words, odd ones odd words
    links = np.stack([np.arange(0, nV, 2), np.arange(1, nV, 2)], axis=1)
    unlinked = np.stack([np.arange(0, nV, 2), (np.arange(0, nV, 2) + 14) % nV + 1], axis=1)      # (2i, 2(i + 7) + 1): no shared document either

    def cosine(Wt, pr):
        a, b = Wt[pr[:, 0]], Wt[pr[:, 1]]
        return float(((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).mean())

    def run(mixed):
        m = gpu_model(spec, B, sampler=ca.SAMPLER_DEVICE)
        m.initialize(77)
        r = np.random.RandomState(5)
        for step in range(150):
            labels = r.randint(0, nD, B).astype(np.int64)
            words = np.stack([r.choice(vocab_of[d], w) for d in labels]).astype(np.int64).ravel()
            batch = ca.Batch(words, labels)
            pairs = links[r.randint(0, len(links), M)]
            if mixed:
                m.step_term_mixed(batch, ca.PairBatch(pairs), 0.01, (0.5, 0.5))
            else:
                m.step(batch, 0.01)
        Wt = m.get_param(W_NAME).reshape(nV, 32).astype(np.float64)
        return cosine(Wt, links), cosine(Wt, unlinked)

    linked_text, _ = run(False)
    linked_mixed, unlinked_mixed = run(True)
    print("planted term pairs: mean cosine of linked words %.3f mixed (unlinked %.3f), %.3f text only" % (linked_mixed, unlinked_mixed, linked_text))
    assert linked_mixed > unlinked_mixed and linked_mixed > linked_text
