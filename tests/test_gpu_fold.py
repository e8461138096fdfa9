"""-m gpu: document fold-in (nvsm_step_fold, nvsm_get_param_rows / nvsm_set_param_rows).

A fold step trains rows [n0, |D|) of the documents table against a frozen model. What is checked: frozen means frozen (bit for bit,
lazily decayed tables included), the forward pass is compute_cost's, the new rows track "the oracle's full step, then the frozen
parameters put back" (tests/fold_reference.py) at test_update_parity's tolerances, the summation's boundaries row by row, the edges
of first_document, reproducibility across max_batch_size, the row-ranged parameter access, and that ranking sees a folded document.

Entity ids are given explicitly throughout, so row lengths are chosen, not sampled."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import fold_reference as fr
from tests.helpers import PARAMS, gpu_model, load_params, oracle_model, random_batch, random_params, rel_err

pytestmark = pytest.mark.gpu

UPD_TOL = 2e-4          # tests/test_gpu_parity.py test_update_parity: the same quantities, the same bounds
STATE_TOL = 5e-4
B = 512
ND = 30
SHAPES = {"nvsm": dict(word_dim=300, entity_dim=256, window=10), "odd": dict(word_dim=7, entity_dim=5, window=3)}
METHODS = fr.METHOD_NAMES
LR = {"sgd": 0.1, "adagrad": 0.01}
# a table much larger than the batch (tests/test_gpu_parity.py SPECS["sparse_touch"]): with NVSM_LAZY_MIN_MB=0 its documents table decays lazily
SPARSE_TOUCH = dict(num_words=30000, num_entities=40000, word_dim=16, entity_dim=12, window=3, num_random=4, nonlinearity="hard_tanh",
                    batch_norm=True)
STATE_CANDIDATES = ["word_representations/m", "word_representations/v", "word_representations/a", "entity_representations/m",
                    "entity_representations/v", "entity_representations/a", "word_entity_mapping/s0_transform", "word_entity_mapping/s0_bias",
                    "word_entity_mapping/s1_transform", "word_entity_mapping/s1_bias"]


def make_spec(shape, k, method, lam, nD=ND):
    spec = dict(SHAPES[shape], num_words=200, num_entities=nD, num_random=k, nonlinearity="hard_tanh", batch_norm=True, update_method=method)
    spec["lambda"] = lam
    return spec


def lr_of(method):
    return LR.get(method, 0.001)


def state_names(m):
    out = []
    for n in STATE_CANDIDATES:
        try:
            m.get_param(n)
            out.append(n)
        except ca.NvsmError:
            pass
    return out


def snapshot(m):
    return {n: m.get_param(n).copy() for n in list(PARAMS) + state_names(m)}


def entity_rows(m, name, arr):
    """[|D|][width] view of a documents-table array"""
    return arr.reshape(m.cfg.num_entities, -1)


def assert_frozen(m, before, n0):
    after = snapshot(m)
    for n, a in after.items():
        if n.startswith("entity_representations"):
            np.testing.assert_array_equal(entity_rows(m, n, a)[:n0], entity_rows(m, n, before[n])[:n0], err_msg=n)
        else:
            np.testing.assert_array_equal(a, before[n], err_msg=n)
    return after


def batch_of(spec, rs, ids_fn=None, b=B):
    words, ww, labels, iw, ids = random_batch(spec, rs, b, zipf=True)
    if ids_fn is not None:
        ids = ids_fn(ids.reshape(b, -1).copy()).ravel()
        labels = ids.reshape(b, -1)[:, 0].copy()
    return words, ww, labels, iw, ids


def fresh(spec, seed, max_batch=B, **extra):
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    g = gpu_model(spec, max_batch, **extra)
    load_params(g, params, True)
    return g, params, rs


# ---- 1. frozen means frozen --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.01])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape,k", [("nvsm", 16), ("nvsm", 1), ("odd", 16), ("odd", 1)])
def test_frozen_means_frozen(shape, k, method, lam):
    spec = make_spec(shape, k, method, lam)
    g, _, rs = fresh(spec, 3)
    n0 = 20
    words, ww, labels, iw, ids = batch_of(spec, rs)
    g.step(ca.Batch(words, labels, ww, iw), lr_of(method), entity_ids=ids)          # optimiser state that is not all zero
    before = snapshot(g)
    for _ in range(3):
        words, ww, labels, iw, ids = batch_of(spec, rs)
        g.step_fold(ca.Batch(words, labels, ww, iw), lr_of(method), n0, entity_ids=ids)
    after = assert_frozen(g, before, n0)
    e0, e1 = (entity_rows(g, PARAMS[1], x[PARAMS[1]]) for x in (before, after))
    assert np.all(np.any(e0[n0:] != e1[n0:], axis=1))                               # every new row trained (each has entries at these shapes)


@pytest.mark.parametrize("method", ["sgd", "adagrad", "sparse_adam"])
def test_frozen_on_a_lazily_decayed_table_and_an_ordinary_step_behind(method, monkeypatch):
    """Two ordinary steps leave pending factors on the rows they did not touch; three fold steps must leave every frozen row's LOGICAL
    value alone, and an ordinary step behind them must do what it does on a twin handle that was given the same parameters and state
    through set_param. (The twin comparison needs equal Adam step counters, which set_param cannot give: SGD and Adagrad only.)"""
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(SPARSE_TOUCH, update_method=method)
    spec["lambda"] = 0.01
    nD = spec["num_entities"]
    n0 = nD - 10
    g, _, rs = fresh(spec, 4)
    g.profile_enable(True)
    for _ in range(2):
        words, ww, labels, iw, ids = batch_of(spec, rs)
        g.step(ca.Batch(words, labels, ww, iw), lr_of(method), entity_ids=ids)
    assert "lazy_stamp_entities" in set(g.profile())                                 # the documents table does decay lazily
    g.profile_enable(False)
    # (get_param flushes the table, which is not what a trainer does between steps: the first fold step below must meet the pending
    #  factors, so the snapshot is taken from a twin that ran the same two steps)
    t0, _, rs0 = fresh(spec, 4)
    for _ in range(2):
        words, ww, labels, iw, ids = batch_of(spec, rs0)
        t0.step(ca.Batch(words, labels, ww, iw), lr_of(method), entity_ids=ids)
    before = snapshot(t0)

    def new_positives(ids):
        ids[:, 0] = n0 + np.arange(ids.shape[0]) % 9                                 # nine of the ten new rows get positives, one nothing
        return ids
    for _ in range(3):
        words, ww, labels, iw, ids = batch_of(spec, rs, new_positives)
        g.step_fold(ca.Batch(words, labels, ww, iw), lr_of(method), n0, entity_ids=ids)
    after = assert_frozen(g, before, n0)
    e0, e1 = (entity_rows(g, PARAMS[1], x[PARAMS[1]]) for x in (before, after))
    changed = np.any(e0[n0:] != e1[n0:], axis=1)
    assert changed[:9].all()
    # the row without entries decays by 1 − λ/B·lr: 1 − 2e-6 (SGD), 1 − 2e-7 (Adagrad); at Adam's lr = 1e-3 the factor is 1.0f
    assert changed[9] == (method != "sparse_adam")
    if method == "sparse_adam":
        return
    twin = gpu_model(spec, B)
    for n, a in after.items():
        twin.set_param(n, a)
    words, ww, labels, iw, ids = batch_of(spec, rs)
    for m in (g, twin):
        m.step(ca.Batch(words, labels, ww, iw), lr_of(method), entity_ids=ids)
    a, b = snapshot(g), snapshot(twin)
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)


# ---- 2. same forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [("nvsm", 16), ("odd", 1)])
def test_cost_is_compute_costs(shape, k):
    spec = make_spec(shape, k, "sparse_adam", 0.01)
    a, _, rs = fresh(spec, 5)
    b, _, _ = fresh(spec, 5)
    for step in range(2):                                                            # the second pass starts from folded rows on both
        words, ww, labels, iw, ids = batch_of(spec, rs)
        batch = ca.Batch(words, labels, ww, iw)
        b.compute_cost(batch, ids)
        want = b.get_cost()
        got = a.step_fold(batch, 0.001, 20, entity_ids=ids)
        assert got == want, (step, got, want)
        b.step_fold(batch, 0.001, 20, entity_ids=ids)


# ---- 3. new rows track the reference -----------------------------------------------------------------------------------------
def check_against(g, o, spec, method, n0, start):
    nD, de = spec["num_entities"], spec["entity_dim"]
    ref = o.get(fr.E).reshape(nD, de)[n0:]
    got = g.get_param(fr.E).astype(np.float64).reshape(nD, de)[n0:]
    delta = np.linalg.norm(ref - start.reshape(nD, de)[n0:])
    err = np.linalg.norm(got - ref)
    assert err <= UPD_TOL * max(delta, 1e-12) + 2e-7 * np.linalg.norm(ref), (err, delta)
    for gn, on, _ in fr.oracle_state_names(method):
        a = g.get_param(gn).reshape(nD, -1)[n0:]
        b = o.get(on).reshape(nD, -1)[n0:]
        assert rel_err(a, b) < STATE_TOL, (gn, rel_err(a, b))


@pytest.mark.parametrize("lam", [0.0, 0.01])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape,k", [("nvsm", 16), ("nvsm", 1), ("odd", 16), ("odd", 1)])
def test_new_rows_track_full_step_then_restore(shape, k, method, lam):
    spec = make_spec(shape, k, method, lam)
    g, params, rs = fresh(spec, 6)
    o = oracle_model(spec)
    load_params(o, params, False)
    n0 = 20
    start = o.get(fr.E).copy()
    frozen = {p: g.get_param(p).copy() for p in PARAMS}
    for step in range(3):
        words, ww, labels, iw, ids = batch_of(spec, rs)
        co = fr.oracle_fold_step(o, words, ww, ids, iw, n0, lr_of(method))
        cg = g.step_fold(ca.Batch(words, labels, ww, iw), lr_of(method), n0, entity_ids=ids)
        assert abs(cg - co) <= 5e-5 * abs(co), (step, cg, co)
    check_against(g, o, spec, method, n0, start)
    for p in fr.FROZEN:
        np.testing.assert_array_equal(g.get_param(p), frozen[p])


# ---- 4. row lengths at the summation's boundaries ----------------------------------------------------------------------------
def boundary_counts(total):
    C, G = ca.fold_summation()                       # the kernel's own constants (nvsm_fold_summation)
    counts = [0, 1, C - 1, C, C + 1, 2 * C + 1, G * C + 1]
    rest = total - sum(counts)
    assert rest > G * C + 1, "the batch is too small for these row lengths"
    return counts, (rest * 4) // 5                    # "all the rest" of the new rows' share; a fifth of what is left goes to frozen rows


@pytest.mark.parametrize("lam", [0.0, 0.01])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", ["nvsm", "odd"])
def test_row_lengths_at_the_boundaries(shape, method, lam):
    k = 16
    spec = make_spec(shape, k, method, lam)
    R, nD, de = k + 1, ND, spec["entity_dim"]
    n0 = nD - 8
    counts, last = boundary_counts(B * R)
    g, _, rs = fresh(spec, 7)
    words, ww, labels, iw, ids = batch_of(spec, rs)
    g.step(ca.Batch(words, labels, ww, iw), lr_of(method), entity_ids=ids)          # m, v, a of the new rows are not zero
    flat = np.concatenate([np.full(c, n0 + i, np.int64) for i, c in enumerate(counts + [last])])
    flat = np.concatenate([flat, rs.randint(0, n0, B * R - flat.size).astype(np.int64)])
    rs.shuffle(flat)
    words, ww, labels, iw, _ = batch_of(spec, rs)
    labels = flat.reshape(B, R)[:, 0].copy()
    P = g.get_param(fr.E).astype(np.float64).reshape(nD, de)
    P32 = g.get_param(fr.E).reshape(nD, de).copy()
    state = {}
    for gn, _, scalar in fr.oracle_state_names(method):
        a = g.get_param(gn).astype(np.float64)
        state[gn[-1]] = a.copy() if scalar else a.reshape(nD, de).copy()
    before = {key: v.copy() for key, v in state.items()}
    lr = lr_of(method)
    g.step_fold(ca.Batch(words, labels, ww, iw), lr, n0, entity_ids=flat)
    proj = g.get_tensor("proj").astype(np.float64).reshape(B, de)
    coef = g.get_tensor("multipliers").astype(np.float64)
    pp = (proj * proj).mean(axis=1)
    gsum, q, cnt = fr.row_sums(proj, coef, pp, flat, R, nD)
    assert list(cnt[n0:].astype(int)) == counts + [last]
    sl = lam / B
    want = P.copy()
    fr.fold_update(method, want, state, gsum, q, cnt, n0, lr, sl, 2)                # the ordinary step above was the table's first update
    got = g.get_param(fr.E).astype(np.float64).reshape(nD, de)
    for r in range(n0, nD):
        delta = np.linalg.norm(want[r] - P[r])
        err = np.linalg.norm(got[r] - want[r])
        assert err <= UPD_TOL * max(delta, 1e-12) + 2e-7 * np.linalg.norm(want[r]), (r, int(cnt[r]), err, delta)
    for gn, _, scalar in fr.oracle_state_names(method):
        a = g.get_param(gn).astype(np.float64).reshape(nD, -1)
        b = state[gn[-1]].reshape(nD, -1)
        for r in range(n0, nD):
            assert np.linalg.norm(a[r] - b[r]) <= STATE_TOL * np.linalg.norm(b[r]), (gn, r, int(cnt[r]))
        np.testing.assert_array_equal(a[:n0], before[gn[-1]].reshape(nD, -1)[:n0].astype(np.float64))
    if method == "sgd":                              # the row without entries: decay · P, exactly
        decay = np.float32(1.0 - float(np.float32(lam) / np.float32(B)) * float(np.float32(lr))) if lam > 0 else np.float32(1)
        np.testing.assert_array_equal(g.get_param(fr.E).reshape(nD, de)[n0], P32[n0] * decay)
    np.testing.assert_array_equal(g.get_param(fr.E).reshape(nD, de)[:n0], P32[:n0])


# ---- 5. edges of first_document ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["sgd", "sparse_adam", "full_adam"])
def test_first_document_zero_trains_every_row_like_a_step(method):
    spec = make_spec("nvsm", 16, method, 0.01)
    a, _, rs = fresh(spec, 8)
    b, _, _ = fresh(spec, 8)
    words, ww, labels, iw, ids = batch_of(spec, rs)
    batch = ca.Batch(words, labels, ww, iw)
    before = snapshot(a)
    a.step_fold(batch, lr_of(method), 0, entity_ids=ids)
    b.step(batch, lr_of(method), entity_ids=ids)
    ea, eb = a.get_param(fr.E).astype(np.float64), b.get_param(fr.E).astype(np.float64)
    delta = np.linalg.norm(eb - before[fr.E])
    assert np.linalg.norm(ea - eb) <= UPD_TOL * max(delta, 1e-12) + 2e-7 * np.linalg.norm(eb)
    assert delta > 0
    for p in fr.FROZEN:
        np.testing.assert_array_equal(a.get_param(p), before[p])


@pytest.mark.parametrize("method", ["adagrad", "sparse_adam"])
@pytest.mark.parametrize("shape", ["nvsm", "odd"])
def test_one_row_takes_every_positive(shape, method):
    spec = make_spec(shape, 16, method, 0.01)
    g, params, rs = fresh(spec, 9)
    o = oracle_model(spec)
    load_params(o, params, False)
    n0 = ND - 1
    start = o.get(fr.E).copy()

    def all_on_the_last(ids):
        ids[:, 0] = n0
        return ids
    words, ww, labels, iw, ids = batch_of(spec, rs, all_on_the_last)
    fr.oracle_fold_step(o, words, ww, ids, iw, n0, lr_of(method))
    g.step_fold(ca.Batch(words, labels, ww, iw), lr_of(method), n0, entity_ids=ids)
    check_against(g, o, spec, method, n0, start)
    np.testing.assert_array_equal(g.get_param(fr.E)[:n0 * spec["entity_dim"]], params[fr.E][:n0 * spec["entity_dim"]])


def test_first_document_at_and_beyond_the_table():
    spec = make_spec("nvsm", 16, "sparse_adam", 0.01)
    a, _, rs = fresh(spec, 10)
    b, _, _ = fresh(spec, 10)
    words, ww, labels, iw, ids = batch_of(spec, rs)
    batch = ca.Batch(words, labels, ww, iw)
    a.step(batch, 0.001, entity_ids=ids)
    b.step(batch, 0.001, entity_ids=ids)
    before = snapshot(a)
    b.compute_cost(batch, ids)
    assert a.step_fold(batch, 0.001, ND, entity_ids=ids) == b.get_cost()             # nothing trains, the cost is still produced
    after = snapshot(a)
    for n in before:
        np.testing.assert_array_equal(after[n], before[n], err_msg=n)
    for bad in (ND + 1, -1):
        with pytest.raises(ca.NvsmError) as e:
            a.step_fold(batch, 0.001, bad, entity_ids=ids)
        assert e.value.status == 1 and "first_document" in str(e.value)
    a.step_fold(batch, 0.001, 20, entity_ids=ids)                                    # the handle is usable afterwards


def test_refusals_are_status_codes():
    spec = make_spec("odd", 1, "sgd", 0.0)
    rs = np.random.RandomState(0)
    words, ww, labels, iw, ids = batch_of(spec, rs, b=8)
    batch = ca.Batch(words, labels, ww, iw)
    dp = gpu_model(spec, 8, world_size=2, rank=0)
    with pytest.raises(ca.NvsmError) as e:
        dp.step_fold(batch, 0.1, 20, entity_ids=ids)
    assert e.value.status == 2 and "world_size" in str(e.value)
    l2 = gpu_model(dict(spec, l2_entity=True), 8)
    with pytest.raises(ca.NvsmError) as e:
        l2.step_fold(batch, 0.1, 20, entity_ids=ids)
    assert e.value.status == 2 and "l2_normalize_entity_reprs" in str(e.value)


# ---- 6. reproducible ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,method", [("nvsm", "sgd"), ("nvsm", "adagrad"), ("nvsm", "sparse_adam"), ("odd", "dense_adam"), ("nvsm", "full_adam"),
                                          ("odd", "sparse_adam")])
def test_same_bits_whatever_max_batch_size(shape, method):
    spec = make_spec(shape, 16, method, 0.01)
    n0 = ND - 3
    models = [fresh(spec, 11, max_batch=mb)[0] for mb in (512, 2048)]
    rs = np.random.RandomState(12)
    C, G = ca.fold_summation()

    def hot(ids):                                    # row n0: several groups; row n0 + 1: several chunks; row n0 + 2: what the negatives give it
        ids[:, :6] = n0
        ids[::4, 6] = n0 + 1
        assert 6 * ids.shape[0] > C * G and ids.shape[0] // 4 > C
        return ids
    for _ in range(5):
        words, ww, labels, iw, ids = batch_of(spec, rs, hot)
        costs = [m.step_fold(ca.Batch(words, labels, ww, iw), lr_of(method), n0, entity_ids=ids) for m in models]
        assert costs[0] == costs[1]
    a, b = (snapshot(m) for m in models)
    assert set(a) == set(b)
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)


# ---- 7. row-ranged access ----------------------------------------------------------------------------------------------------
def check_row_access(g, spec, rs):
    nD, de = spec["num_entities"], spec["entity_dim"]
    rows = rs.uniform(-1, 1, (5, de)).astype(np.float32)
    whole = g.get_param(fr.E).reshape(nD, de).copy()
    g.set_param_rows(fr.E, nD - 7, rows)
    np.testing.assert_array_equal(g.get_param_rows(fr.E, nD - 7, 5), rows)
    whole[nD - 7:nD - 2] = rows
    np.testing.assert_array_equal(g.get_param(fr.E).reshape(nD, de), whole)
    np.testing.assert_array_equal(g.get_param_rows(fr.E, 0, nD), whole)
    np.testing.assert_array_equal(g.get_param_rows("word_representations-representations", 3, 2).ravel(),
                                  g.get_param("word_representations-representations")[3 * spec["word_dim"]:5 * spec["word_dim"]])
    v = rs.uniform(0, 1, (4, 1)).astype(np.float32)
    g.set_param_rows("entity_representations/v", 2, v)
    np.testing.assert_array_equal(g.get_param("entity_representations/v")[2:6], v.ravel())
    m = rs.uniform(-1, 1, (2, de)).astype(np.float32)
    g.set_param_rows("entity_representations/m", nD - 2, m)
    np.testing.assert_array_equal(g.get_param_rows("entity_representations/m", nD - 2, 2), m)
    assert g.get_param_rows(fr.E, nD, 0).shape == (0, de)
    for first, n in ((nD - 1, 2), (-1, 1), (nD + 1, 0), (0, nD + 1)):
        with pytest.raises(ca.NvsmError) as e:
            g.get_param_rows(fr.E, first, n)
        assert e.value.status == 1
    with pytest.raises(ca.NvsmError) as e:
        g.set_param_rows(fr.E, nD - 1, np.zeros((2, de), np.float32))
    assert e.value.status == 1
    with pytest.raises(ca.NvsmError) as e:
        g.get_param_rows("word_entity_mapping-transform", 0, 1)
    assert e.value.status == 1


def test_row_access_round_trips_on_an_eager_table():
    spec = make_spec("nvsm", 16, "sparse_adam", 0.01)
    g, _, rs = fresh(spec, 13)
    words, ww, labels, iw, ids = batch_of(spec, rs)
    g.step(ca.Batch(words, labels, ww, iw), 0.001, entity_ids=ids)
    check_row_access(g, spec, rs)


def test_row_access_round_trips_on_a_lazily_decayed_table(monkeypatch):
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(SPARSE_TOUCH, update_method="sparse_adam")
    spec["lambda"] = 0.01
    g, _, rs = fresh(spec, 14)
    t, _, rs_t = fresh(spec, 14)
    for m, r in ((g, rs), (t, rs_t)):
        for _ in range(2):                           # pending factors on the rows the batches did not touch
            words, ww, labels, iw, ids = batch_of(spec, r)
            m.step(ca.Batch(words, labels, ww, iw), 0.001, entity_ids=ids)
    nD, de = spec["num_entities"], spec["entity_dim"]
    # a ranged read meets the pending factors and returns the logical values: those of the twin's whole-table read
    np.testing.assert_array_equal(g.get_param_rows(fr.E, nD - 100, 100), t.get_param(fr.E).reshape(nD, de)[nD - 100:])
    check_row_access(g, spec, rs)


# ---- 8. ranking sees the result ----------------------------------------------------------------------------------------------
def test_rank_returns_a_folded_document():
    """New documents 25..29 each consist of three words of their own; after fold steps on windows of those words, the query made of
    document 27's words must retrieve a new document among the top k."""
    spec = dict(num_words=60, num_entities=ND, word_dim=16, entity_dim=16, window=3, num_random=4, nonlinearity="tanh", batch_norm=False,
                update_method="sgd")
    spec["lambda"] = 0.0
    n0, b = 25, 60
    g, _, rs = fresh(spec, 15, max_batch=b)
    doc_words = {d: np.array([3 * (d - n0), 3 * (d - n0) + 1, 3 * (d - n0) + 2]) + 10 for d in range(n0, ND)}
    labels = n0 + np.arange(b) % (ND - n0)
    words = np.stack([rs.permutation(doc_words[d]) for d in labels]).astype(np.int64).ravel()
    ones_w, ones_i = np.ones(b * 3, np.float32), np.ones(b, np.float32)
    before = g.get_param(fr.E).copy()
    for _ in range(40):
        ids = rs.randint(0, ND, (b, 5)).astype(np.int64)
        ids[:, 0] = labels
        g.step_fold(ca.Batch(words, labels.astype(np.int64), ones_w, ones_i), 20.0, n0, entity_ids=ids.ravel())
    k = 5
    ids, scores, counts = g.rank([list(doc_words[27])], top_k=k)
    assert counts[0] == k
    assert np.any(ids[0] >= n0), (ids, scores)
    np.testing.assert_array_equal(g.get_param(fr.E)[:n0 * 16], before[:n0 * 16])
