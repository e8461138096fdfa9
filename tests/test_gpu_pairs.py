"""-m gpu: the entity-entity similarity objective (pairs.hip) alone and mixed into the text objective — nvsm_compute_cost_mixed /
nvsm_step_mixed against tests/pairs_reference.py (fp64 numpy, checked on its own by tests/test_pairs_reference.py).

Tolerances are the project's stated fp32 ones: forward tensors and loss rel 2e-5, gradients rel-L2 2e-4, a
parameter change after updates 5e-4 (5e-3 for the Adam modes, whose first steps divide by sqrt(v) of a few squared gradients)."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import pairs_reference as ref
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params, rel_err

pytestmark = pytest.mark.gpu

E_NAME = "entity_representations-representations"
FWD_TOL, GRAD_TOL = 2e-5, 2e-4
UPD_TOL = {"sgd": 5e-4, "adagrad": 5e-4, "sparse_adam": 5e-3, "dense_adam": 5e-3, "full_adam": 5e-3}
LR = {"sgd": 0.1, "adagrad": 0.01, "sparse_adam": 0.001, "dense_adam": 0.001, "full_adam": 0.001}
STATE = {"sgd": [], "adagrad": ["entity_representations/a"], "sparse_adam": ["entity_representations/m", "entity_representations/v"],
         "dense_adam": ["entity_representations/m", "entity_representations/v"], "full_adam": ["entity_representations/m", "entity_representations/v"]}
WORD_STATE = {"sgd": [], "dense_adam": ["word_representations/m", "word_representations/v"], "full_adam": ["word_representations/m", "word_representations/v"]}


def make_spec(nD, de, method="sgd", lam=0.0, **kw):
    spec = dict(num_words=60, num_entities=nD, word_dim=8, entity_dim=de, window=3, num_random=2, update_method=method)
    spec["lambda"] = lam
    spec.update(kw)
    return spec


def random_pairs(rs, nD, M, weighted=True):
    pairs = rs.randint(0, nD, (M, 2)).astype(np.int64)
    if M >= 5:
        pairs[1] = (pairs[1, 0], pairs[1, 0])          # a == b
        pairs[3] = pairs[2]                            # a repeated pair
    w = rs.uniform(0.0, 2.0, M).astype(np.float32) if weighted else None
    return pairs, w


def all_state(m, method, words=False):
    names = list(PARAMS) + STATE[method] + (WORD_STATE.get(method, []) if words else [])
    return {n: m.get_param(n) for n in names}


def change_error(E, E0, P, updates=1):
    """|(E - E0) - (P - E0)| and what it may be: the tolerance's share of the reference's change plus the floor of keeping the
    table in float32 — every update rounds each element once (P·decay + lr·g is one fused rounding: half an ulp, 2^-24 relative),
    whatever the size of the change. Where a batch moves most rows by less than an ulp (a decay of 1 - 2.5e-7, a gradient of
    1e-7 of the row) that floor, not the arithmetic, is what a whole-table difference measures."""
    err = np.linalg.norm(np.asarray(E, np.float64) - P)
    return err, np.linalg.norm(P - E0), updates * 2.0 ** -24 * np.linalg.norm(P)


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)


# ---- 1. the pair objective alone against the fp64 helper ------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("de", [8, 36, 128, 256])
@pytest.mark.parametrize("M", [1, 5, 1000, 51200])
def test_pairs_only_forward_and_gradient(M, de, weighted):
    rs = np.random.RandomState(M + de)
    nD = 700
    m = gpu_model(make_spec(nD, de), max(M, 8))
    E = (rs.uniform(-1, 1, (nD, de)) * np.sqrt(3.0 / de)).astype(np.float32)      # unit-variance rows: |dot| of a few units
    m.set_param(E_NAME, E)
    pairs, w = random_pairs(rs, nD, M, weighted)
    m.compute_cost_mixed(None, ca.PairBatch(pairs, w))
    m.compute_gradients()
    f = ref.pair_forward(E, pairs, w)
    cost = m.get_cost()
    print("pairs M=%d de=%d: probs %.2e cost %.2e mult %.2e grad %.2e" % (
        M, de, rel_err(m.get_tensor("pair_probs"), f["probs"]), abs(cost - f["cost"]) / abs(f["cost"]),
        rel_err(m.get_tensor("pair_multipliers"), f["multipliers"]), rel_err(m.get_tensor("grad_pair_entity"), f["grad"])))
    assert rel_err(m.get_tensor("pair_probs"), f["probs"]) < FWD_TOL
    assert abs(cost - f["cost"]) <= FWD_TOL * abs(f["cost"])
    assert m.get_tensor("pair_cost")[0] == np.float32(cost)
    assert rel_err(m.get_tensor("pair_multipliers"), f["multipliers"]) < GRAD_TOL
    assert rel_err(m.get_tensor("grad_pair_entity"), f["grad"]) < GRAD_TOL
    assert m.scaled_regularization_lambda() == 0.0


@pytest.mark.parametrize("de", [8, 36, 256])
def test_saturated_pairs(de):
    nD = 6
    m = gpu_model(make_spec(nD, de, lam=0.5), 8)
    E = np.zeros((nD, de), np.float32)
    E[0, :4], E[1, :4] = 2.0, 5.0           # dot = +40
    E[2, :4], E[3, :4] = 2.0, -5.0          # dot = -40
    m.set_param(E_NAME, E)
    pairs = np.array([(0, 1), (2, 3)])
    m.compute_cost_mixed(None, ca.PairBatch(pairs))
    m.compute_gradients()
    f = ref.pair_forward(E, pairs)
    np.testing.assert_array_equal(m.get_tensor("pair_probs"), f["probs"].astype(np.float32))      # the float32 clamps themselves
    assert np.all(m.get_tensor("pair_multipliers") == 0.0) and np.all(m.get_tensor("grad_pair_entity") == 0.0)
    assert abs(m.get_cost() - f["cost"]) <= FWD_TOL * abs(f["cost"])
    assert m.scaled_regularization_lambda() == pytest.approx(0.25)                                  # lambda / M


# ---- 2. the reference's own pair set, three updates per method -------------------------------------------------------------
def reference_pair_set():
    data = []
    while len(data) < 3 * (1 << 10):                   # cpp/gradient_checking_tests.cu:142-148
        data += [(0, 1, 1.0), (1, 2, 0.5), (2, 3, 1.0), (0, 2, 1.0), (1, 2, 1.0)]
    data = data[:3072]
    return np.array([(a, b) for a, b, _ in data], np.int64), np.array([x for _, _, x in data], np.float32)


@pytest.mark.parametrize("lam", [0.0, 0.1])
@pytest.mark.parametrize("method", ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"])
@pytest.mark.parametrize("fused", [False, True])
def test_reference_pair_set_updates(method, lam, fused):
    nD, de = 15, 4
    pairs, w = reference_pair_set()
    m = gpu_model(make_spec(nD, de, method, lam), 4096)
    rs = np.random.RandomState(7)
    E0 = rs.uniform(-0.5, 0.5, (nD, de)).astype(np.float32)
    m.set_param(E_NAME, E0)
    other = {p: m.get_param(p) for p in PARAMS if p != E_NAME}
    opt = ref.TableOptimizer(E0, method)
    sl = ref.scaled_lambda(lam, M=len(pairs))
    for step in range(3):
        f = ref.pair_forward(opt.P, pairs, w)
        opt.update([(f["grad"], f["ids"])], LR[method], sl)
        if fused:
            c = m.step_mixed(None, ca.PairBatch(pairs, w), LR[method], want_cost=True)
        else:
            m.compute_cost_mixed(None, ca.PairBatch(pairs, w))
            assert m.scaled_regularization_lambda() == pytest.approx(sl, rel=1e-6)
            m.compute_gradients()
            c = m.get_cost()
            m.update(LR[method])
        if step == 0:                                      # (later steps start from tables that differ within the update tolerance)
            assert abs(c - f["cost"]) <= FWD_TOL * abs(f["cost"])
    E = m.get_param(E_NAME).reshape(nD, de)
    err = rel_err(E - E0, opt.P - E0)
    print("reference pair set %s lambda %.1f fused %d: parameter change rel %.2e" % (method, lam, fused, err))
    assert err < UPD_TOL[method]
    for p, v in other.items():                         # nothing else has a gradient (cpp/params.cu:304-307)
        np.testing.assert_array_equal(m.get_param(p), v, err_msg=p)
    assert not m.get_tensor("arrival_counters").any()


# ---- 3. full-parameter central differences through nvsm_increment_parameter / nvsm_get_cost_f64 -----------------------------
# Step 2^-6 on float32 parameters of magnitude <= 0.6 (exactly representable increments). Error budget of (c+ - c-) / 2h against
# the analytic gradient, relative: truncation h^2 |f'''| / 6 |f'| — h^2 / 6 = 4e-5 times a ratio of a few units for tanh / sigmoid
# compositions of O(1) arguments —, plus float32 evaluation noise of the cost (~1e-7 relative per term, averaged over the batch)
# over 2h = 1/32: a few 1e-6 absolute on gradients of 1e-3 .. 1e-1. Bound: rel-L2 per parameter tensor < 2e-3.
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
    nD, de, M = 15, 4, 1024
    rs = np.random.RandomState(3)
    m = gpu_model(make_spec(nD, de), M)
    E = rs.uniform(-0.5, 0.5, (nD, de)).astype(np.float32)
    E = (np.round(E * 64) / 64).astype(np.float32)               # on the step's grid: +h, -2h, +h returns to the same bits
    m.set_param(E_NAME, E)
    pairs = rs.randint(0, 11, (M, 2))
    w = rs.uniform(0, 2, M).astype(np.float32)
    pb = ca.PairBatch(pairs, w)
    forward = lambda: m.compute_cost_mixed(None, pb)
    forward(); m.compute_gradients()
    g = m.get_tensor("grad_pair_entity").reshape(2 * M, de)
    pred = -ref.dense_gradient((nD, de), [(g, pairs.reshape(-1))]).ravel()
    approx = central_differences(m, E_NAME, forward)
    np.testing.assert_array_equal(m.get_param(E_NAME), E.ravel())
    print("central differences, pairs only: rel-L2 %.2e" % rel_err(pred, approx))
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
    pw = rs.uniform(0, 2, M).astype(np.float32)
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    forward = lambda: m.compute_cost_mixed(batch, pb, (1.0, 1.0), entity_ids=ids)
    forward(); m.compute_gradients()
    dw, de = 3, 4
    gE = ref.dense_gradient((15, de), [(m.get_tensor("grad_entity").reshape(-1, de), ids),
                                        (m.get_tensor("grad_pair_entity").reshape(-1, de), pairs.reshape(-1))])
    gphrase = m.get_tensor("grad_phrase").reshape(B, dw)
    gW = ref.dense_gradient((20, dw), [(np.repeat(gphrase, 3, axis=0) * ww[:, None], words)])
    pred = {PARAMS[0]: -gW.ravel(), PARAMS[1]: -gE.ravel(), PARAMS[2]: -m.get_tensor("grad_transform").astype(np.float64),
            PARAMS[3]: -m.get_tensor("grad_bias").astype(np.float64)}
    for name in PARAMS:
        approx = central_differences(m, name, forward)
        print("central differences, mixed (1, 1): %s rel-L2 %.2e" % (name, rel_err(pred[name], approx)))
        assert rel_err(pred[name], approx) < FD_TOL, name


# ---- 4. mixed tensors are the weighted single-objective tensors -----------------------------------------------------------
def mixed_case(method="sgd", lam=0.0, B=600, M=400, de=16, seed=5, nD=900, bn=False):
    spec = make_spec(nD, de, method, lam, word_dim=12, batch_norm=bn, nonlinearity="hard_tanh" if bn else "tanh")
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    pairs, pw = random_pairs(rs, nD, M)
    return spec, params, (words, ww, labels, iw, ids), (pairs, pw)


@pytest.mark.parametrize("bn", [False, True])
def test_mixed_tensors_are_the_weighted_tensors(bn):
    lam = 0.2
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case(lam=lam, bn=bn)
    B, M = labels.size, len(pairs)
    m = gpu_model(spec, B)
    load_params(m, params, True)
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    m.compute_cost(batch, ids); m.compute_gradients()
    text = {n: m.get_tensor(n) for n in ("grad_transform", "grad_bias", "grad_phrase", "multipliers", "probs", "proj")}
    text_cost = m.get_cost()
    m.compute_cost_mixed(None, pb); m.compute_gradients()
    pair_grad, pair_cost = m.get_tensor("grad_pair_entity"), m.get_cost()
    m.compute_cost_mixed(batch, pb, (0.7, 0.3), entity_ids=ids); m.compute_gradients()
    for n in ("grad_transform", "grad_bias", "grad_phrase", "multipliers"):
        err = rel_err(m.get_tensor(n), np.float32(0.7) * text[n])
        print("mixed (0.7, 0.3) bn=%d: %s against 0.7 x text-only rel %.2e" % (bn, n, err))
        assert err < GRAD_TOL, n
    for n in ("probs", "proj"):
        np.testing.assert_array_equal(m.get_tensor(n), text[n], err_msg=n)
    assert rel_err(m.get_tensor("grad_pair_entity"), np.float32(0.3) * pair_grad) < GRAD_TOL
    assert abs(m.get_cost() - (text_cost + pair_cost) / 2) <= FWD_TOL * abs(text_cost + pair_cost) / 2
    assert abs(m.get_tensor("text_cost")[0] - text_cost) <= FWD_TOL * abs(text_cost)
    assert m.get_tensor("pair_cost")[0] == np.float32(pair_cost)
    assert m.scaled_regularization_lambda() == pytest.approx((lam / B + lam / M) / 2, rel=1e-6)
    # ... and a text-only call afterwards is the text-only result again, bit for bit
    m.compute_cost(batch, ids); m.compute_gradients()
    for n in text:
        np.testing.assert_array_equal(m.get_tensor(n), text[n], err_msg=n)
    assert m.get_cost() == text_cost


# ---- 5. the mixed update --------------------------------------------------------------------------------------------------
def test_mixed_sgd_update_is_the_weighted_sum_of_the_updates():
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
            m.compute_cost_mixed(None, pb)
        else:
            m.compute_cost_mixed(batch, pb, (0.7, 0.3), entity_ids=ids)
        m.compute_gradients(); m.update(0.1)
        after[kind] = {p: m.get_param(p).astype(np.float64) - params[p].ravel() for p in PARAMS}
    want = 0.7 * after["text"][E_NAME] + 0.3 * after["pairs"][E_NAME]
    print("mixed sgd: dE against 0.7 dE_text + 0.3 dE_pairs rel %.2e" % rel_err(after["mixed"][E_NAME], want))
    assert rel_err(after["mixed"][E_NAME], want) < UPD_TOL["sgd"]
    for p in PARAMS:
        if p != E_NAME:
            assert rel_err(after["mixed"][p], 0.7 * after["text"][p]) < UPD_TOL["sgd"], p
            assert not after["pairs"][p].any(), p


@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_mixed_documents_update_against_the_helper(method, lam):
    """The helper takes the GPU's own text-side entry gradients (grad_entity, the mixture scale included — the text path is held
    to the oracle elsewhere) and its own pair gradients: one decay, one Adam step, both lists."""
    spec, params, _, _ = mixed_case(method, lam)
    nD, de, B, M = spec["num_entities"], spec["entity_dim"], 600, 400
    m = gpu_model(spec, B)
    load_params(m, params, True)
    E0 = params[E_NAME].reshape(nD, de)
    opt = ref.TableOptimizer(E0, method)
    rs = np.random.RandomState(9)
    for step in range(3):
        words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
        pairs, pw = random_pairs(rs, nD, M)
        m.compute_cost_mixed(ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw), (0.7, 0.3), entity_ids=ids)
        m.compute_gradients()
        f = ref.pair_forward(m.get_param(E_NAME).reshape(nD, de), pairs, pw, scale=np.float32(0.3) / (np.float32(0.7) + np.float32(0.3)))
        assert rel_err(m.get_tensor("grad_pair_entity"), f["grad"]) < GRAD_TOL
        opt.P[...] = m.get_param(E_NAME).reshape(nD, de)           # (follow the GPU's table: this checks one update at a time)
        before = opt.P.copy()
        opt.update([(m.get_tensor("grad_entity").reshape(-1, de), ids), (f["grad"], f["ids"])], LR[method], ref.scaled_lambda(lam, B, M))
        m.update(LR[method])
        err = rel_err(m.get_param(E_NAME).reshape(nD, de) - before, opt.P - before)
        print("mixed %s lambda %.1f step %d: documents change rel %.2e" % (method, lam, step, err))
        assert err < UPD_TOL[method]


# ---- 6. structure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_one_document_in_20000_pairs_takes_both_chunk_levels(mixed):
    nD, de, M = 3000, 32, 20000
    spec = make_spec(nD, de, "sgd", 0.05)
    rs = np.random.RandomState(13)
    params = random_params(spec, rs)
    m = gpu_model(spec, M)
    load_params(m, params, True)
    pairs = np.stack([np.full(M, 7), rs.randint(0, nD, M)], axis=1)
    pairs[::3] = pairs[::3, ::-1]                       # the hot document on either side
    pw = rs.uniform(0, 2, M).astype(np.float32)
    E0 = params[E_NAME].reshape(nD, de)
    opt = ref.TableOptimizer(E0, "sgd")
    if mixed:
        B = 512
        words, ww, labels, iw, ids = random_batch(spec, rs, B)
        ids[::5] = 7
        m.compute_cost_mixed(ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw), (0.5, 0.5), entity_ids=ids)
        m.compute_gradients()
        f = ref.pair_forward(E0, pairs, pw, scale=0.5)
        lists = [(m.get_tensor("grad_entity").reshape(-1, de), ids), (f["grad"], f["ids"])]
        sl = ref.scaled_lambda(0.05, B, M)
    else:
        m.compute_cost_mixed(None, ca.PairBatch(pairs, pw))
        m.compute_gradients()
        f = ref.pair_forward(E0, pairs, pw)
        lists = [(f["grad"], f["ids"])]
        sl = ref.scaled_lambda(0.05, M=M)
    assert np.bincount(np.concatenate([l[1] for l in lists]))[7] > 64 * 32      # more than kFan level-1 chunks: level 2 is taken
    opt.update(lists, 0.1, sl)
    m.update(0.1)
    E = m.get_param(E_NAME).reshape(nD, de)
    print("hot document (mixed %d): row 7 change rel %.2e, table change rel %.2e" % (mixed, rel_err(E[7] - E0[7], opt.P[7] - E0[7]), rel_err(E - E0, opt.P - E0)))
    assert rel_err(E[7] - E0[7], opt.P[7] - E0[7]) < UPD_TOL["sgd"]
    err, change, floor = change_error(E, E0, opt.P)
    print("hot document (mixed %d): table error %.3e, change %.3e, float32 floor %.3e" % (mixed, err, change, floor))
    assert err <= UPD_TOL["sgd"] * change + floor
    assert not m.get_tensor("arrival_counters").any()


@pytest.mark.parametrize("entry_walk_min", [None, "0"])
@pytest.mark.parametrize("method", ["sgd", "sparse_adam"])
def test_table_much_larger_than_the_batch(method, entry_walk_min, monkeypatch):
    """The rows with entries of a table much larger than the batch are walked by list or by sorted entry (update.hip): the pair
    entries' ids are not 0 .. n - 1, which both walks must not mind."""
    if entry_walk_min is not None:
        monkeypatch.setenv("NVSM_ENTRY_WALK_MIN", entry_walk_min)
    nD, de, M = 120000, 64, 3000
    spec = make_spec(nD, de, method, 0.02)
    rs = np.random.RandomState(17)
    m = gpu_model(spec, M)
    E0 = (rs.uniform(-1, 1, (nD, de)) * 0.2).astype(np.float32)
    m.set_param(E_NAME, E0)
    opt = ref.TableOptimizer(E0, method)
    m.profile_enable(True)
    for step in range(2):
        pairs, pw = random_pairs(rs, nD, M)
        pairs[:40, 0] = 11                              # a row of a few dozen entries among rows of one or two
        f = ref.pair_forward(opt.P, pairs, pw)
        opt.update([(f["grad"], f["ids"])], LR[method], ref.scaled_lambda(0.02, M=M))
        m.step_mixed(None, ca.PairBatch(pairs, pw), LR[method])
    prof = m.profile()
    assert "pair_loss" in prof and "row_pass_entities_mixed" in prof and "row_pass_entities" not in prof
    if entry_walk_min == "0":
        assert "entry_walk_entities" in prof
    E = m.get_param(E_NAME).reshape(nD, de)
    touched = np.unique(f["ids"])
    err, change, floor = change_error(E[touched], E0[touched], opt.P[touched], updates=2)
    print("large table %s entry_walk_min %s: touched rows' error %.3e, change %.3e, float32 floor %.3e" % (method, entry_walk_min, err, change, floor))
    assert err <= UPD_TOL[method] * change + floor
    assert rel_err(E, opt.P) < 1e-6


def mixed_run(m, spec, steps, seed, method, fused=lambda s: s % 2 == 0, text_only=lambda s: False, pairs_only=lambda s: False,
              B=40, M=24, weights=(0.6, 0.4)):
    rs = np.random.RandomState(seed)
    for s in range(steps):
        b, mm = int(rs.choice([1, 7, B])), int(rs.choice([1, 5, M]))
        words, ww, labels, iw, ids = random_batch(spec, rs, b, zipf=True)
        pairs, pw = random_pairs(rs, spec["num_entities"], mm)
        lr = float(rs.choice([1e-3, 5e-3, 2e-2]))
        batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
        if text_only(s):
            if fused(s):
                m.step(batch, lr, entity_ids=ids)
            else:
                m.compute_cost(batch, ids); m.compute_gradients(); m.update(lr)
        elif pairs_only(s):
            if fused(s):
                m.step_mixed(None, pb, lr)
            else:
                m.compute_cost_mixed(None, pb); m.compute_gradients(); m.update(lr)
        elif fused(s):
            m.step_mixed(batch, pb, lr, weights, entity_ids=ids)
        else:
            m.compute_cost_mixed(batch, pb, weights, entity_ids=ids); m.compute_gradients(); m.update(lr)
    return m


@pytest.mark.parametrize("method,pairs_only", [("sgd", False), ("sgd", True), ("adagrad", True), ("sparse_adam", True)])
def test_lazily_decayed_tables_equal_the_eager_twin(method, pairs_only, monkeypatch):
    spec = make_spec(5000, 16, method, 0.05, num_words=3000)
    params = random_params(spec, np.random.RandomState(2))
    monkeypatch.setenv("NVSM_LAZY_DECAY", "0")
    eager = gpu_model(spec, 40)
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    lazy = gpu_model(spec, 40)
    for m in (eager, lazy):
        load_params(m, params, True)
        mixed_run(m, spec, 6, 31, method, pairs_only=lambda s: pairs_only)
    assert "lazy decay" in lazy.describe() and "documents lazy" in lazy.describe() and "documents eager" in eager.describe()
    assert_same_bits(all_state(eager, method), all_state(lazy, method))
    # ... and over more than one of the periodic whole-table refreshes
    for m in (eager, lazy):
        mixed_run(m, spec, 140, 32, method, pairs_only=lambda s: pairs_only)
    assert_same_bits(all_state(eager, method), all_state(lazy, method))


@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_three_launch_pass_equals_the_one_launch_pass(method, monkeypatch):
    spec = make_spec(300, 16, method, 0.05)
    params = random_params(spec, np.random.RandomState(2))
    results = []
    for merged in ("1", "0"):
        monkeypatch.setenv("NVSM_MERGED_PASS", merged)
        m = gpu_model(spec, 256)
        load_params(m, params, True)
        mixed_run(m, spec, 8, 33, method, B=256, M=256)
        results.append(all_state(m, method, words=True))
    assert_same_bits(*results)


# ---- 7. reproducibility ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_200_mixed_steps_twice_are_bit_equal(method):
    spec = make_spec(400, 32, method, 0.05, word_dim=16)
    params = random_params(spec, np.random.RandomState(4))
    results = []
    for run in range(2):
        m = gpu_model(spec, 128)
        load_params(m, params, True)
        mixed_run(m, spec, 200, 41, method, fused=lambda s: True, B=128, M=128)
        results.append(all_state(m, method, words=True))
        assert not m.get_tensor("arrival_counters").any()
    assert_same_bits(*results)


@pytest.mark.parametrize("B,M", [(64, 48), (2048, 3000)])
@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_fused_step_equals_the_three_calls(method, B, M):
    spec = make_spec(500, 32, method, 0.05, word_dim=16)
    params = random_params(spec, np.random.RandomState(4))
    results = []
    for fused in (True, False):
        m = gpu_model(spec, max(B, M))
        load_params(m, params, True)
        mixed_run(m, spec, 12, 43, method, fused=lambda s: fused, B=B, M=M)
        results.append(all_state(m, method, words=True))
    assert_same_bits(*results)


def test_costs_of_the_fused_step_equal_the_three_calls():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case(lam=0.1)
    costs = []
    for fused in (True, False):
        m = gpu_model(spec, labels.size)
        load_params(m, params, True)
        batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
        if fused:
            costs.append(m.step_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids, want_cost=True))
        else:
            m.compute_cost_mixed(batch, pb, (0.7, 0.3), entity_ids=ids); m.compute_gradients()
            costs.append(m.get_cost()); m.update(0.01)
    assert costs[0] == costs[1]


@pytest.mark.parametrize("method", ["sgd", "dense_adam", "full_adam"])
def test_text_steps_interleaved_with_mixed_steps(method):
    """One handle through text-only, mixed and pairs-only steps equals the same sequence on a fresh handle."""
    spec = make_spec(400, 32, method, 0.05, word_dim=16)
    params = random_params(spec, np.random.RandomState(4))
    results = []
    for run in range(2):
        m = gpu_model(spec, 96)
        load_params(m, params, True)
        mixed_run(m, spec, 60, 47, method, text_only=lambda s: s % 3 == 0, pairs_only=lambda s: s % 7 == 5, B=96, M=96)
        results.append(all_state(m, method, words=True))
    assert_same_bits(*results)


@pytest.mark.parametrize("method", ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"])
def test_text_only_after_pair_calls_equals_a_handle_that_never_made_one(method):
    """The first pair call replaces the handle's larger buffers and its documents CSR workspace; text-only steps afterwards must
    produce the bits of a handle that never made a pair call. The pair calls here are forward / backward passes (they leave the
    parameters, the optimiser state and its step counters alone); with sgd, which has no state, whole mixed steps as well, the
    parameters loaded again afterwards."""
    spec = make_spec(400, 32, method, 0.05, word_dim=16)
    params = random_params(spec, np.random.RandomState(4))
    rs = np.random.RandomState(8)
    words, ww, labels, iw, ids = random_batch(spec, rs, 96, zipf=True)
    pairs, pw = random_pairs(rs, 400, 80)
    seen, fresh = gpu_model(spec, 96), gpu_model(spec, 96)
    load_params(seen, params, True)
    seen.compute_cost_mixed(None, ca.PairBatch(pairs, pw)); seen.compute_gradients(); seen.get_cost()
    if method in ("sgd", "dense_adam", "full_adam"):
        seen.compute_cost_mixed(ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw), (0.5, 0.5), entity_ids=ids)
        seen.compute_gradients(); seen.get_cost()
    if method == "sgd":
        mixed_run(seen, spec, 5, 48, method, B=96, M=96)
    for m in (seen, fresh):
        load_params(m, params, True)
        mixed_run(m, spec, 30, 49, method, text_only=lambda s: True, B=96, M=96)
    names = list(PARAMS) + STATE[method] + [n.replace("entity_", "word_") for n in STATE[method]]
    for n in names:
        np.testing.assert_array_equal(seen.get_param(n), fresh.get_param(n), err_msg=n)


# ---- 8. memory ------------------------------------------------------------------------------------------------------------
def test_memory_growth_at_the_headline_shape_stays_under_400_mb():
    """|V| = 50 k, |D| = 100 k, 300 -> 256, window 10, 16 negatives, batch 51 200, M = 51 200: the pair rows are 105 MB, plus
    coefficients and CSR growth; materialising the text objective's gradient rows would take 891 MB."""
    import torch
    spec = dict(num_words=50000, num_entities=100000, word_dim=300, entity_dim=256, window=10, num_random=16, batch_norm=True,
                nonlinearity="hard_tanh", update_method="dense_adam")
    spec["lambda"] = 0.01
    B = M = 51200
    m = gpu_model(spec, B, sampler=ca.SAMPLER_DEVICE)
    m.initialize(1)
    rs = np.random.RandomState(0)
    words, ww, labels, iw, _ = random_batch(spec, rs, B, zipf=True)
    pairs, pw = random_pairs(rs, spec["num_entities"], M)
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    for _ in range(2):
        m.step(batch, 1e-3)
    m.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        m.step_mixed(batch, pb, 1e-3, (0.8, 0.2))
    m.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print("pairs-memory: device memory in use grew by %.1f MB from the first mixed call on" % ((free0 - free1) / 1e6))
    assert np.isfinite(m.get_param(E_NAME)).all()
    assert free0 - free1 < 400e6, (free0 - free1) / 1e6


# ---- 9. errors ------------------------------------------------------------------------------------------------------------
def status_of(fn):
    with pytest.raises(ca.NvsmError) as e:
        fn()
    return e.value.status, str(e.value)


def test_a_bad_pair_id_is_reported_at_the_next_wait_and_the_handle_recovers():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case()
    B = labels.size
    batch = ca.Batch(words, labels, ww, iw)
    bad = pairs.copy()
    bad[17, 1] = spec["num_entities"]
    worse = pairs.copy()
    worse[3, 0] = -1
    hit, fresh = gpu_model(spec, B), gpu_model(spec, B)
    load_params(hit, params, True)
    hit.step_mixed(batch, ca.PairBatch(bad, pw), 0.01, (0.7, 0.3), entity_ids=ids)
    st, msg = status_of(hit.synchronize)
    assert st == 1 and "document id" in msg
    hit.compute_cost_mixed(None, ca.PairBatch(worse, pw))
    st, msg = status_of(hit.get_cost)
    assert st == 1
    for m in (hit, fresh):
        load_params(m, params, True)
        for _ in range(3):
            m.step_mixed(batch, ca.PairBatch(pairs, pw), 0.01, (0.7, 0.3), entity_ids=ids)
        m.step(batch, 0.01, entity_ids=ids)
    assert_same_bits(all_state(hit, "sgd"), all_state(fresh, "sgd"))
    assert not hit.get_tensor("arrival_counters").any()


def test_refused_configurations_leave_the_handle_usable():
    spec, params, (words, ww, labels, iw, ids), (pairs, pw) = mixed_case()
    B = labels.size
    batch, pb = ca.Batch(words, labels, ww, iw), ca.PairBatch(pairs, pw)
    L = ca.lib()
    import ctypes as C

    def raw_mixed(m, st, ps, mix):
        return L.nvsm_compute_cost_mixed(m._h, C.byref(st) if st is not None else None, ids.ctypes.data, C.byref(ps), C.byref(mix) if mix is not None else None)

    for method, sentence in (("adagrad", "Adagrad currently does not implement multiple gradients."),
                             ("sparse_adam", "Sparse Adam currently does not implement multiple gradients.")):
        m = gpu_model(dict(spec, update_method=method), B)
        load_params(m, params, True)
        for call in (lambda: m.compute_cost_mixed(batch, pb, (0.7, 0.3), entity_ids=ids), lambda: m.step_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids)):
            st, msg = status_of(call)
            assert st == 2 and sentence in msg
        m.step_mixed(None, pb, 0.01)                       # the pair objective alone exists for every method
        m.step(batch, 0.01, entity_ids=ids)
        assert np.isfinite(m.get_cost())
    m = gpu_model(dict(spec, l2_entity=True), B)
    st, msg = status_of(lambda: m.compute_cost_mixed(None, pb))
    assert st == 2 and "l2_normalize_entity_reprs" in msg
    m.step(batch, 0.01, entity_ids=ids)
    m = gpu_model(spec, B, world_size=2, rank=0)
    st, msg = status_of(lambda: m.compute_cost_mixed(None, pb))
    assert st == 2 and "world_size" in msg
    # invalid arguments: mixture weights, pair counts
    m = gpu_model(spec, B)
    load_params(m, params, True)
    st_b, ps = batch.as_struct(), pb.as_struct()
    for wt, wp in ((0.0, 1.0), (1.0, 0.0), (-0.5, 1.5)):
        assert raw_mixed(m, st_b, ps, ca.NvsmMixture(wt, wp)) == 1 and "must both be > 0" in L.nvsm_last_error().decode()
    for n in (0, -3, B + 1):
        ps_bad = pb.as_struct()
        ps_bad.num_pairs = n
        assert raw_mixed(m, None, ps_bad, None) == 1 and "num_pairs" in L.nvsm_last_error().decode()
    assert raw_mixed(m, st_b, ps, None) == 1 and "mix" in L.nvsm_last_error().decode()
    with pytest.raises(ca.NvsmError):
        m.get_tensor("pair_probs")                         # no forward result with pairs yet
    m.step_mixed(batch, pb, 0.01, (0.7, 0.3), entity_ids=ids)
    assert "pairs: pair_loss" in m.describe()


# ---- 10. training effect --------------------------------------------------------------------------------------------------
def test_planted_pairs_pull_linked_documents_together():
    """Documents come in linked pairs (2i, 2i + 1) whose texts share nothing; only the similarity pairs say they belong together.
    After the same number of steps from the same seed the linked documents are closer (mean cosine, Model.similarity) in the mixed
    run than in the text-only run, and the text cost falls in both."""
    nD, nV, w, B, M = 400, 800, 4, 512, 256
    spec = dict(num_words=nV, num_entities=nD, word_dim=32, entity_dim=32, window=w, num_random=4, batch_norm=True,
                nonlinearity="hard_tanh", update_method="dense_adam")
    spec["lambda"] = 0.0
    rs = np.random.RandomState(1)
    vocab_of = [rs.choice(nV, 12, replace=False) for _ in range(nD)]       # every document writes with its own dozen words
    links = np.stack([np.arange(0, nD, 2), np.arange(1, nD, 2)], axis=1)

    def run(mixed):
        m = gpu_model(spec, B, sampler=ca.SAMPLER_DEVICE)
        m.initialize(77)
        r = np.random.RandomState(5)
        text_costs = []
        for step in range(150):
            labels = r.randint(0, nD, B).astype(np.int64)
            words = np.stack([r.choice(vocab_of[d], w) for d in labels]).astype(np.int64).ravel()
            batch = ca.Batch(words, labels)
            pairs = links[r.randint(0, len(links), M)]
            if mixed:
                m.compute_cost_mixed(batch, ca.PairBatch(pairs), (0.5, 0.5))
                text_costs.append(float(m.get_tensor("text_cost")[0]))
            else:
                m.compute_cost(batch)
                text_costs.append(m.get_cost())
            m.compute_gradients(); m.update(0.01)
        return float(m.similarity("entities", links[:, 0], links[:, 1]).mean()), text_costs

    cos_text, costs_text = run(False)
    cos_mixed, costs_mixed = run(True)
    print("planted pairs: mean cosine of linked documents %.3f mixed, %.3f text only; text cost %.3f -> %.3f mixed, %.3f -> %.3f text only" % (
        cos_mixed, cos_text, np.mean(costs_mixed[:10]), np.mean(costs_mixed[-10:]), np.mean(costs_text[:10]), np.mean(costs_text[-10:])))
    assert cos_mixed > cos_text
    assert np.mean(costs_mixed[-10:]) < np.mean(costs_mixed[:10]) and np.mean(costs_text[-10:]) < np.mean(costs_text[:10])
