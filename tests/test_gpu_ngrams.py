"""-m gpu: n-grams of terms in document space (nvsm_ngram_search, csrc/ngram.hip; TermBruteforcer, py/nvsm/base.py:106-162) against
the numpy restatement of tests/ngram_reference.py.

1. The generator alone, through nvsm_debug_ngram_rows: with the identity or hard-tanh and c in {0, 0.5, 1} every operation of a
   phrase row is a single float32 rounding whether or not the compiler contracts it (ngram_reference.generator_rows says why), so the
   rows equal the float32 numpy expression BIT FOR BIT; with tanh a 1-gram row equals, bit for bit, what the same G row becomes on
   nvsm_infer's query side (launch_rank_bias_act: the one __device__ bias-and-activation function both kernels call).
2. The RANK CORRECTNESS RULE of tests/test_gpu_rank.py, unchanged, end to end: s64 and err32 come from the REFERENCE chain (mean,
   @ T, + c·b, f) in fp64 and in float32 numpy, tol = 4·err32, never from the GPU result. tests/test_ngram_reference.py vets every
   case of CASES on the CPU: the float32 library chain passes the rule and the bands are narrow with the tolerance doubled.
3. Ties and zeros, lazily decayed tables and neutrality, determinism, refusals, profile names.

Every case prints `ngram-error` lines: err32 and the observed max|s − s64| / err32 (DESIGN.md §18 quotes them)."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import ngram_reference as ref
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE, band_is_narrow, check_result, ref_scores, same_bits

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
ACTS = {"identity": ca.ACT_IDENTITY, "tanh": ca.TANH, "hard_tanh": ca.HARD_TANH}
GUARD = np.float32(12345.0)


# ---- 1. the generator, element by element ---------------------------------------------------------------------------------------------
def hook_rows(G, bias, c, act, p0, S, guard_rows=2):
    """rows [p0, p0 + S) by one launch into a guard-filled buffer; the guard rows must come back untouched"""
    m, de = G.shape
    out = np.full((S + 2 * guard_rows, de), GUARD, np.float32)
    ca._lib.check(ca.lib().nvsm_debug_ngram_rows(G.ctypes.data, m, de, bias.ctypes.data, c, ACTS[act], p0, S, out.ctypes.data,
                                                 out.shape[0], guard_rows))
    assert (out[:guard_rows] == GUARD).all() and (out[guard_rows + S:] == GUARD).all(), "rows outside [p0, p0 + S) were written"
    return out[guard_rows:guard_rows + S]


def run_start(a, m):
    return m + a * (2 * m - a - 1) // 2


def slabs_of(m):
    """(p0, S): the whole stack, its first row, inside the 1-grams, exactly at m, mid-run, a run's last row, the last row alone, and
    slabs that begin at each of those places and reach the last row R − 1 or straddle what follows"""
    R = ca.ngram_rows(m, 2)
    starts = {0, m // 2, m - 1, min(m, R - 1), R - 1}
    if m >= 3:
        a = m // 3
        starts |= {run_start(a, m) + (m - a - 1) // 2, run_start(a + 1, m) - 1, run_start(a, m)}
    out = {(0, R)}
    for p0 in sorted(starts):
        for S in (1, 2, 17, 70, R - p0):
            if 1 <= S <= R - p0:
                out.add((p0, S))
    return sorted(out)


@pytest.mark.parametrize("de", [1, 6, 36, 64, 100, 256])
@pytest.mark.parametrize("m", [1, 2, 5, 100])
def test_generator_rows_equal_the_float32_expression_bit_for_bit(m, de):
    rs = np.random.RandomState(31 * m + de)
    G = rs.uniform(-1.5, 1.5, (m, de)).astype(np.float32)
    bias = rs.uniform(-0.5, 0.5, de).astype(np.float32)
    combos = [(act, c) for act in ("identity", "hard_tanh") for c in (0.0, 0.5, 1.0)]
    R = ca.ngram_rows(m, 2)
    full = {ac: ref.generator_rows(G, bias, ac[1], ac[0], 0, R) for ac in combos}
    if m * de >= 30:
        assert (np.abs(ref.generator_rows(G, bias, 1.0, "identity", 0, R)) > 1).any(), "some units leave hard_tanh's linear region"
    for i, (p0, S) in enumerate(slabs_of(m)):
        for act, c in (combos if (p0, S) == (0, R) else [combos[i % len(combos)]]):
            got = hook_rows(G, bias, c, act, p0, S)
            np.testing.assert_array_equal(got.view(np.uint32), full[act, c][p0:p0 + S].view(np.uint32), err_msg=str((m, de, p0, S, act, c)))


def test_the_hook_refuses_rows_outside_the_stack():
    G, bias, out = np.zeros((5, 4), np.float32), np.zeros(4, np.float32), np.zeros((20, 4), np.float32)
    L = ca.lib()
    args = lambda m, p0, S, rows, row0: (G.ctypes.data, m, 4, bias.ctypes.data, 1.0, ca.TANH, p0, S, out.ctypes.data, rows, row0)  # noqa: E731
    assert L.nvsm_debug_ngram_rows(*args(5, 0, 15, 20, 0)) == 0
    assert L.nvsm_debug_ngram_rows(*args(5, 0, 16, 20, 0)) == 1          # R = 15
    assert L.nvsm_debug_ngram_rows(*args(5, 14, 2, 20, 0)) == 1
    assert L.nvsm_debug_ngram_rows(*args(5, -1, 2, 20, 0)) == 1
    assert L.nvsm_debug_ngram_rows(*args(5, 0, 15, 20, 6)) == 1          # does not fit the buffer
    assert L.nvsm_debug_ngram_rows(*args(65536, 0, 1, 20, 0)) == 1
    assert L.nvsm_debug_ngram_rows(*args(0, 0, 1, 20, 0)) == 1


@pytest.mark.parametrize("de,nonlin", [(256, "tanh"), (36, "hard_tanh"), (6, "tanh")])
def test_a_one_gram_row_is_the_query_side_of_infer_bit_for_bit(de, nonlin):
    """G = T·W[w] as nvsm_infer's query side leaves it (c = 0, identity: gather, product, the factored function as a no-op); the
    generator's 1-gram row of that G and infer's f(G + c·b) are the same bits, tanh included: one __device__ function, no libm tolerance"""
    spec = dict(num_words=50, num_entities=8, word_dim=20, entity_dim=de, window=1, num_random=1, nonlinearity=nonlin, update_method="sgd")
    rs = np.random.RandomState(de)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 4).astype(np.float32)
    m = gpu_model(spec, 8)
    load_params(m, params, True)
    words = np.arange(50)
    G = m.infer([[w] for w in words], bias_coefficient=0.0, activation="identity")
    for act in ("tanh", "hard_tanh", "identity"):
        for c in (0.0, 0.3, 1.0):
            want = m.infer([[w] for w in words], bias_coefficient=c, activation=act)
            got = hook_rows(G, params[B_NAME], c, act, 0, 50)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str((act, c)))
    m.close()


# ---- 2. the rule, end to end -------------------------------------------------------------------------------------------------------------
#         V    m    dw  de   Q    k    act          c    sim       slab  vocabulary  card  queries       seed offset
CASES = [(100, 100, 24, 64,  64,  20,  "tanh",      1.0, "cosine", 1,    "all",      2,    "entity_ids", 0),   # 5 050 rows, two slabs of 4 096:
         #                                           the 1-gram / 2-gram boundary inside the first, the slab boundary inside the run of a = 55
         (300, 40,  30, 6,   5,   1,   "hard_tanh", 0.0, "dot",    None, "subset",   2,    "vectors",    0),   # the plain scan; k = 1
         (300, 40,  30, 36,  7,   820, "model",     0.5, "cosine", None, "subset",   2,    "word_ids",   0),   # the MFMA tail; k = R
         (60,  60,  16, 100, 5,   20,  "identity",  1.0, "cosine", None, "all",      2,    "entity_ids", 0),   # the MFMA tail, three chunks + 4
         (500, 500, 20, 256, 3,   20,  "tanh",      1.0, "cosine", None, "all",      1,    "vectors",    0),   # 1-grams only
         (200, 30,  50, 256, 4,   20,  "tanh",      0.0, "dot",    None, "subset",   2,    "entity_ids", 0),
         (50,  50,  12, 64,  300, 20,  "hard_tanh", 1.0, "cosine", None, "all",      2,    "vectors",    0),   # two rounds of queries
         (300, 40,  30, 36,  5,   40,  "tanh",      1.0, "dot",    None, "subset",   1,    "word_ids",   0),   # 1-grams of a subset; k = R
         (30,  1,   8,  64,  2,   1,   "tanh",      1.0, "cosine", None, "subset",   2,    "entity_ids", 0)]   # one word: a stack of one row


def expected_slabs(R, de, Q, slab_mb):
    S = min(R, max(4096, ((slab_mb or 256) << 18) // min(Q, 256) // 4096 * 4096), max(4096, (64 << 20) // (de * 4) // 4096 * 4096))
    return [min(S, R - p0) for p0 in range(0, R, S)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "V%d-m%d-de%d-Q%d-k%d-%s-%s-card%d-%s" % (c[0], c[1], c[3], c[4], c[5], c[6], c[8], c[11], c[12]))
def test_ngram_rule(case, monkeypatch):
    V, m, dw, de, Q, k, act, c, sim, slab_mb, vkind, card, qkind, offset = case
    if slab_mb:
        monkeypatch.setenv("NVSM_RANK_SLAB_MB", str(slab_mb))          # read by nvsm_create
    spec, params, vocabulary, queries = ref.case_inputs(case)
    s64, err32, tol, _ = ref.case_scores(case, spec, params, vocabulary, queries, ref_scores)
    R = ca.ngram_rows(m, card)
    assert s64.shape == (Q, R)
    for q in range(Q):
        band_is_narrow(s64[q], np.arange(R), k, tol)                   # the test's own inputs, before the GPU result is read
    model = gpu_model(spec, 8)
    load_params(model, params, True)
    model.profile_enable(True)
    voc = None if vkind == "all" else vocabulary
    rows, terms, scores, counts = model.nearest_ngrams(vocabulary=voc, max_cardinality=card, top_k=k, similarity=sim, bias_coefficient=c,
                                                       activation=act, **{qkind: queries[qkind]})
    prof = model.profile()
    worst = check_result((rows, scores, counts), s64, k, tol)
    print("ngram-error V=%d m=%d dw=%d de=%d Q=%d k=%d %s c=%g %s card=%d by %s slab=%s: err32 %.3g, max|s-s64|/err32 %.2f"
          % (V, m, dw, de, Q, k, act, c, sim, card, qkind, slab_mb, err32, worst / max(err32, 1e-45)))
    # terms = the decoded rows mapped through the vocabulary
    assert terms.shape == (Q, k, card) and terms.dtype == np.int64
    pos = ca.ngram_decode(rows, m, card)
    np.testing.assert_array_equal(terms, np.where(pos >= 0, vocabulary[np.maximum(pos, 0)], -1))
    np.testing.assert_array_equal(ca.ngram_encode(pos, m), rows)
    # one generator launch and one scan per slab and round; the scan by nvsm_neighbors' dispatch
    rounds = -(-Q // 256)
    slabs = expected_slabs(R, de, Q, slab_mb)
    if slab_mb:
        assert slabs == [4096, 954]
    assert prof["ngram_rows"][1] == rounds * len(slabs) and prof["ngram_scan"][1] == rounds * len(slabs), prof
    assert ("ngram_scan_mfma" if de % 4 == 0 and de >= 32 else "ngram_scan_plain") in prof
    assert not any(n.startswith(("rank_scan", "nbr_scan", "rank_query", "rank_infer")) for n in prof), sorted(prof)
    model.close()


def test_the_case_table_covers_what_the_issue_lists():
    col = lambda i: {c[i] for c in CASES}      # noqa: E731
    assert {"all", "subset"} <= col(10) and col(11) == {1, 2} and {6, 36, 100, 64, 256} <= col(3)
    assert col(12) == {"entity_ids", "word_ids", "vectors"} and {1, 20} <= col(5)
    assert any(c[5] == ca.ngram_rows(c[1], c[11]) and c[5] > 1 for c in CASES), "k = R"
    assert any(c[1] == 100 and c[4] == 64 and c[9] == 1 for c in CASES)


# ---- 3. ties and zeros -------------------------------------------------------------------------------------------------------------------
def identity_model(W):
    """d_w = d_e, T = I: G is W bit for bit, so that the test knows the phrase rows exactly (identity activation, c = 0)"""
    V, d = W.shape
    spec = dict(num_words=V, num_entities=4, word_dim=d, entity_dim=d, window=1, num_random=1, update_method="sgd")
    m = gpu_model(spec, 8)
    m.set_param(W_NAME, W)
    m.set_param(T_NAME, np.eye(d, dtype=np.float32))
    m.set_param(B_NAME, np.zeros(d, np.float32))
    return m


EXACT = dict(bias_coefficient=0.0, activation="identity")


@pytest.mark.parametrize("d", [64, 6])
def test_ties_zero_phrases_and_the_zero_query(d):
    rs = np.random.RandomState(d)
    V = 12
    W = rs.standard_normal((V, d)).astype(np.float32)
    W[7] = W[2]                                  # duplicate word rows: (2, j) and (7, j) are one vector for every j, (2) and (7) too
    W[9] = -W[4]                                 # (4, 9) is the zero phrase
    W[11] = 0.0                                  # the zero word: the 1-gram (11) is zero, (a, 11) = 0.5·W[a] is parallel to the 1-gram (a)
    m = identity_model(W)
    R = ca.ngram_rows(V, 2)
    pos = ref.phrase_positions(V, 2)
    X = np.where(pos[:, 1:] < 0, W[pos[:, 0]], np.float32(0.5) * (W[pos[:, 0]] + W[np.maximum(pos[:, 1], 0)])).astype(np.float32)
    vec = rs.standard_normal((3, d)).astype(np.float32)
    zero_rows = ca.ngram_encode(np.array([[4, 9], [11, -1]]), V)
    assert not X[zero_rows].any()
    for sim in ("cosine", "dot"):
        s64 = ref_scores(vec, X, sim, np.float64)
        tol = 4 * float(np.abs(ref_scores(vec, X, sim, np.float32).astype(np.float64) - s64).max())
        rows, terms, sc, cnt = m.nearest_ngrams(vectors=vec, top_k=R, similarity=sim, **EXACT)
        assert (cnt == R).all() and not np.isnan(sc).any()
        for q in range(3):
            assert np.array_equal(np.sort(rows[q]), np.arange(R))
            by_row = np.empty(R, np.float32)
            by_row[rows[q]] = sc[q]
            assert np.abs(by_row.astype(np.float64) - s64[q]).max() <= tol
            assert (by_row[zero_rows] == 0).all() and not np.signbit(by_row[zero_rows]).any(), "a zero phrase scores exactly +0"
            twins = [([2, -1], [7, -1])] + [(sorted([2, j]), sorted([7, j])) for j in range(V) if j not in (2, 7)]
            for x, y in twins:                   # equal vectors: one score, bit for bit
                rx, ry = ca.ngram_encode(np.array([x, y]), V)
                assert by_row[rx].view(np.uint32) == by_row[ry].view(np.uint32), (x, y)
            dd = np.diff(sc[q])
            assert (dd <= 0).all() and (np.diff(rows[q])[dd == 0] > 0).all(), "equal scores in ascending phrase-row order"
            assert (dd == 0).sum() >= len(twins)
        for k in (1, 5, 30):                     # a smaller k is a prefix of the full order
            r_k, t_k, s_k, c_k = m.nearest_ngrams(vectors=vec, top_k=k, similarity=sim, **EXACT)
            np.testing.assert_array_equal(r_k, rows[:, :k])
            np.testing.assert_array_equal(s_k.view(np.uint32), sc[:, :k].view(np.uint32))
            np.testing.assert_array_equal(t_k, terms[:, :k])
        # the zero query vector: every score 0, so the rows come out 0 .. k − 1
        for k in (1, 20, R):
            r0, t0, s0, c0 = m.nearest_ngrams(vectors=np.zeros((1, d), np.float32), top_k=k, similarity=sim, **EXACT)
            assert c0[0] == k and (s0 == 0).all() and not np.signbit(s0).any()
            np.testing.assert_array_equal(r0[0], np.arange(k))
    m.close()


# ---- 4. lazily decayed tables, and neutrality ---------------------------------------------------------------------------------------------
def rule_at(params, spec, vocabulary, card, c, act, P, sim, res, k, what):
    X64 = ref.reference_rows(params, spec, vocabulary, card, c, act, np.float64)
    X32 = ref.reference_rows(params, spec, vocabulary, card, c, act, np.float32)
    s64 = ref_scores(P, X64, sim, np.float64)
    err32 = float(np.abs(ref_scores(P, X32, sim, np.float32).astype(np.float64) - s64).max())
    worst = check_result((res[0], res[2], res[3]), s64, k, 4 * err32)
    print("ngram-error %s %s: err32 %.3g, max|s-s64|/err32 %.2f" % (what, sim, err32, worst / err32))


@pytest.mark.parametrize("method", ["sparse_adam", "dense_adam"])
def test_lazy_tables_are_searched_at_their_logical_values_and_training_goes_on_unchanged(method, monkeypatch):
    monkeypatch.setenv("NVSM_LAZY_DECAY", "1")
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    spec = dict(num_words=3000, num_entities=500, word_dim=12, entity_dim=36, window=3, num_random=2, nonlinearity="tanh", batch_norm=False,
                update_method=method)
    spec["lambda"] = 0.02
    rs = np.random.RandomState(12)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    a, b = gpu_model(spec, 40), gpu_model(spec, 40)
    for m in (a, b):
        load_params(m, params, True)
    batches = [random_batch(spec, rs, 40, zipf=True) for _ in range(20)]
    # rare words: rows that sit out all ten updates carry ten pending factors when they are searched
    vocabulary = np.sort(rs.choice(3000, 60, replace=False)).astype(np.int64)
    eids = rs.choice(500, 9, replace=False).astype(np.int64)
    k = 25

    def ten(lo):
        for words, ww, labels, iw, ids in batches[lo:lo + 10]:
            for m in (a, b):
                m.step(ca.Batch(words, labels, ww, iw), 2e-2, entity_ids=ids)
    ten(0)
    got = {sim: a.nearest_ngrams(entity_ids=eids, vocabulary=vocabulary, top_k=k, similarity=sim) for sim in ("cosine", "dot")}      # straight behind nvsm_step
    logical = {n: a.get_param(n) for n in PARAMS}
    assert np.abs(logical[E_NAME] - params[E_NAME]).max() > 0 and np.abs(logical[W_NAME] - params[W_NAME]).max() > 0
    P = logical[E_NAME].reshape(-1, 36)[eids]
    for sim in ("cosine", "dot"):
        rule_at(logical, spec, vocabulary, 2, 1.0, "tanh", P, sim, got[sim], k, "lazy " + method)
    ten(10)
    for n in list(PARAMS) + ADAM_STATE:                       # b never searched
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    if method == "sparse_adam":
        a.profile_enable(True)
        words, ww, labels, iw, ids = batches[0]
        a.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids)
        assert {"lazy_stamp_words", "lazy_stamp_entities"} <= set(a.profile()), "the handle's tables do decay lazily"
    a.close()
    b.close()


# ---- 5. same call, same bits ---------------------------------------------------------------------------------------------------------------
def small_trained_like(seed, de=64, V=400, D=300, dw=40, nonlin="tanh"):
    spec = dict(num_words=V, num_entities=D, word_dim=dw, entity_dim=de, window=4, num_random=3, nonlinearity=nonlin, batch_norm=True,
                update_method="sparse_adam")
    spec["lambda"] = 0.01
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    m = gpu_model(spec, 64)
    load_params(m, params, True)
    return spec, params, m


def test_same_call_same_bits_on_two_handles_and_across_a_repeat():
    spec, params, a = small_trained_like(3)
    _, _, b = small_trained_like(3)
    rs = np.random.RandomState(4)
    eids = rs.choice(300, 70, replace=False).astype(np.int64)
    wids = rs.choice(400, 5, replace=False).astype(np.int64)
    vec = rs.standard_normal((6, 64)).astype(np.float32)
    voc = np.sort(rs.choice(400, 80, replace=False))
    calls = [lambda m: m.nearest_ngrams(entity_ids=eids, vocabulary=voc),
             lambda m: m.nearest_ngrams(word_ids=wids, vocabulary=voc, top_k=3240, similarity="dot", bias_coefficient=0.0),
             lambda m: m.nearest_ngrams(vectors=vec, max_cardinality=1, top_k=400, activation="hard_tanh"),
             lambda m: m.nearest_ngrams(vectors=vec, vocabulary=voc[:1], top_k=1)]
    for call in calls:
        r1, r2, r3 = call(a), call(a), call(b)
        same_bits(r1, r2)
        same_bits(r1, r3)
    # max_cardinality 1 over every word is nearest_terms' search: the same rows, the same score bits
    r1 = a.nearest_ngrams(entity_ids=eids, max_cardinality=1, top_k=20)
    n1 = a.nearest_terms(entity_ids=eids, top_k=20)
    np.testing.assert_array_equal(r1[0], n1[0])
    np.testing.assert_array_equal(r1[1][:, :, 0], n1[0])
    np.testing.assert_array_equal(r1[2].view(np.uint32), n1[1].view(np.uint32))
    a.close()
    b.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = -77


def raw_search(m, top_k=5, card=2, ids=None, source=ca.SPACE_ENTITIES, vectors=None, dim=0, vocabulary=None, vocabulary_size=None,
               similarity=ca.SIM_COSINE, activation=ca.ACT_MODEL, bias=1.0):
    """(status, outputs untouched) of a nvsm_ngram_search filled by hand"""
    q, o = ca.NvsmNeighborQueries(), ca.NvsmNgramOptions()
    ca.lib().nvsm_ngram_options_default(C.byref(o))
    keep, n = [], 0
    if ids is not None:
        keep.append(np.asarray(ids, np.int64))
        q.ids, n = keep[-1].ctypes.data, keep[-1].size
    if vectors is not None:
        keep.append(np.ascontiguousarray(vectors, np.float32))
        q.vectors, n = keep[-1].ctypes.data, keep[-1].shape[0]
    q.num_queries, q.source_space, q.dim = n, source, dim
    if vocabulary is not None:
        keep.append(np.asarray(vocabulary, np.int64))
        o.vocabulary, o.vocabulary_size = keep[-1].ctypes.data, keep[-1].size
    if vocabulary_size is not None:
        o.vocabulary_size = vocabulary_size
    o.max_cardinality, o.top_k, o.similarity, o.activation, o.bias_coefficient = card, top_k, similarity, activation, bias
    k, c = max(top_k, 1), max(card, 1)
    rows, terms = np.full((max(n, 1), k), SENTINEL, np.int64), np.full((max(n, 1), k, c), SENTINEL, np.int64)
    sc, cnt = np.full((max(n, 1), k), SENTINEL, np.float32), np.full(max(n, 1), SENTINEL, np.int64)
    st = ca.lib().nvsm_ngram_search(m._h, C.byref(q), C.byref(o), rows.ctypes.data, terms.ctypes.data, sc.ctypes.data, cnt.ctypes.data)
    untouched = all((x == SENTINEL).all() for x in (rows, terms, sc, cnt))
    return st, untouched


def test_bad_arguments_are_status_codes_nothing_is_written_and_the_handle_still_trains():
    spec, params, m = small_trained_like(2, de=64, V=300, D=500, dw=16)
    V, D = 300, 500
    err = ca.lib().nvsm_last_error
    ok = dict(ids=[1, 2], vocabulary=[3, 5, 9, 200])      # R = 4 + 6 = 10
    assert raw_search(m, **ok) == (0, False)

    def refused(status, word, **kw):
        st, untouched = raw_search(m, **dict(ok, **kw))
        assert st == status and untouched and word in err(), (kw, st, untouched, err())
    refused(1, b"max_cardinality", card=0)
    refused(1, b"max_cardinality", card=3)
    refused(1, b"ascending", vocabulary=[3, 3, 9])
    refused(1, b"ascending", vocabulary=[3, 9, 5])
    refused(1, b"outside", vocabulary=[3, 9, V])
    refused(1, b"outside", vocabulary=[-1, 9])
    refused(1, b"vocabulary_size", vocabulary_size=0)
    refused(1, b"vocabulary_size", vocabulary_size=-4)
    refused(1, b"top_k", top_k=0)
    refused(1, b"top_k", top_k=11)
    refused(1, b"top_k", top_k=5, card=1)                  # R = 4
    refused(1, b"similarity", similarity=7)
    refused(1, b"activation", activation=9)
    refused(1, b"finite", bias=float("nan"))
    refused(1, b"finite", bias=float("inf"))
    refused(1, b"exactly one", ids=None)
    refused(1, b"exactly one", vectors=np.zeros((2, 64)), dim=64)
    refused(1, b"dim", ids=None, vectors=np.zeros((2, 16)), dim=16)
    refused(1, b"dimension", source=ca.SPACE_WORDS)        # d_w = 16 is not document space
    refused(1, b"space", source=7)
    refused(1, b"outside", ids=[1, D])
    refused(1, b"outside", ids=[V], source=ca.SPACE_PROJECTED_WORDS)
    assert raw_search(m, top_k=10, **ok) == (0, False)
    assert raw_search(m, top_k=4, card=1, **ok) == (0, False)
    assert raw_search(m, top_k=3, ids=[1], source=ca.SPACE_PROJECTED_WORDS, vocabulary=[3, 5]) == (0, False)      # R = 2 + 1
    assert raw_search(m, top_k=V, card=1, ids=[1]) == (0, False)                      # no vocabulary: every word
    with pytest.raises(ValueError):
        m.nearest_ngrams(entity_ids=[1], vocabulary=[3, 3])
    words, ww, labels, iw, ids = random_batch(spec, np.random.RandomState(1), 64)
    cost = m.step(ca.Batch(words, labels, ww, iw), 1e-3, entity_ids=ids, want_cost=True)
    assert np.isfinite(cost)
    m.synchronize()
    m.close()


def test_the_row_limit_is_unsupported_before_anything_runs():
    spec = dict(num_words=65536, num_entities=4, word_dim=4, entity_dim=4, window=1, num_random=1, update_method="sgd")
    m = gpu_model(spec, 8)
    m.profile_enable(True)
    st, untouched = raw_search(m, ids=[1], card=2)
    assert st == 2 and untouched and b"2^31" in ca.lib().nvsm_last_error()
    assert not any(n.startswith(("ngram_", "nbr_", "rank_")) for n in m.profile()), "nothing ran"
    assert ca.lib().nvsm_ngram_rows(65536, 2) == -1 and ca.lib().nvsm_ngram_rows(65535, 2) == 65535 + 65535 * 65534 // 2
    st, untouched = raw_search(m, ids=[1], card=1, top_k=3)                           # 1-grams of the same vocabulary are fine
    assert (st, untouched) == (0, False)
    st, untouched = raw_search(m, ids=[1], card=2, top_k=3, vocabulary=np.arange(0, 65536, 1024))
    assert (st, untouched) == (0, False)
    m.close()


# ---- 7. profile names --------------------------------------------------------------------------------------------------------------------
def test_only_the_ngram_call_records_the_ngram_names():
    spec, params, m = small_trained_like(5, de=64, V=400, D=300)
    m.profile_enable(True)
    m.related_terms([1, 2], top_k=30)
    m.nearest_terms(entity_ids=[3], top_k=20)
    m.rank([[1, 2]], top_k=10)
    assert not any(n.startswith("ngram_") for n in m.profile())
    before = {n for n in m.profile() if n.startswith(("rank_scan", "rank_query", "nbr_scan"))}
    m.nearest_ngrams(entity_ids=[3, 4], vocabulary=np.arange(0, 400, 7))
    names = set(m.profile())
    assert {n for n in names if n.startswith("ngram_")} == {"ngram_rows", "ngram_scan", "ngram_scan_mfma"}
    assert {n for n in names if n.startswith(("rank_scan", "rank_query", "nbr_scan"))} == before
    m.close()
