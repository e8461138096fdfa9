"""No GPU: the numpy reference of the table pass (tests/table_pass_reference.py) checked against itself, for every case that
tests/test_gpu_table_pass.py runs - the sums it calls exact are exact, its float32 row formulas agree with float64, and the chunk
counts it expects are those of a plain loop over the rows."""
import numpy as np
import pytest

from tests import table_pass_reference as tp

IDS = [c.name for c in tp.CASES]


@pytest.mark.parametrize("case", tp.CASES, ids=IDS)
def test_sums_are_exact_in_float32(case):
    """Largest possible |partial sum| over granularity < 2^24, from the case's own lengths and values: float32 holds every partial sum
    of g and q exactly, whatever the order and the chunking."""
    ug, uq = case.exactness()
    assert ug < 2 ** 24 and uq < 2 ** 24, (ug, uq)
    assert max(case.lengths) <= 65537
    assert case.max_entries < 2 ** 26 and case.div <= 2048      # the range of the kernels' multiply-shift division


@pytest.mark.parametrize("case", tp.CASES, ids=IDS)
def test_float32_formulas_agree_with_float64(case):
    case.build()
    ref = case.reference32()
    vis, touch = case.visited()
    st = case.start()      # what the formulas start from: the inputs, or (lazy decay) the inputs with the pending factors applied
    if case.kind in tp.SQRT_DIV_KINDS:
        new, tol = case.reference64(ref)
        assert np.all(np.abs(ref["P"].astype(np.float64) - new) <= tol)
        np.testing.assert_array_equal(ref["P"][~touch], case.P[~touch])
    if case.kind == tp.SGD:      # two products and a sum: an ulp and a half of the larger side
        exact = np.where(touch[:, None], st["P"].astype(np.float64) * float(case.decay) + float(case.lr) * case.g, case.P)
        assert np.all(np.abs(ref["P"] - exact) <= 2.0 ** -22 * np.maximum(np.abs(exact), np.abs(float(case.lr) * case.g)))
    if case.kind in (tp.ADAGRAD_ENT, tp.SCALAR_ACC):
        exact = st["sc"].astype(np.float64) + case.q
        assert np.all(np.abs(ref["sc"][vis] - exact[vis]) <= 2.0 ** -24 * np.abs(exact[vis]))
        assert np.all(ref["sc"][vis] > 0)
    if case.kind in (tp.ADAM_MV, tp.ADAM_SPARSE_ENT, tp.ADAM_DENSE):
        exact = st["sc"].astype(np.float64) * float(tp.S_V) + float(tp.ONE_M_B2) * case.q
        assert np.all(np.abs(ref["sc"][vis] - exact[vis]) <= 2.0 ** -22 * (np.abs(st["sc"][vis]) + np.abs(case.q[vis])))
        assert np.all(ref["sc"][vis] > 0)
    if case.kind in tp.USES_M and case.kind != tp.ADAM_FULL:
        exact = st["m"].astype(np.float64) * float(tp.S_M) + float(tp.ONE_M_B1) * case.g
        assert np.all(np.abs(ref["m"] - exact)[vis] <= (2.0 ** -22 * (np.abs(st["m"]) + np.abs(float(tp.ONE_M_B1) * case.g)))[vis])
    for name in ("P", "m", "v", "sc"):
        assert ref[name] is None or np.all(np.isfinite(ref[name]))
    # rows the pass does not visit keep everything
    for name, before in (("P", case.P), ("m", case.m), ("v", case.v)):
        if before is not None:
            np.testing.assert_array_equal(ref[name][~vis], before[~vis])
    if case.lazy:      # ... the stored scalar and the stamp too, however stale the row is
        assert (~vis).any() and (case.lags[~vis] > 0).any()
        if ref["sc"] is not None:
            np.testing.assert_array_equal(ref["sc"][~vis], case.sc_in[~vis])
        np.testing.assert_array_equal(case.stamps_after()[~vis], case.stamp[~vis])
        assert np.all(case.stamps_after()[vis] == case.now + 1)


@pytest.mark.parametrize("case", tp.CASES, ids=IDS)
def test_chunk_counts_and_regime(case):
    for lengths, n in ((case.lengths, case.n),) + (((case.prev_lengths, case.prev_n),) if case.prev_lengths is not None else ()):
        c = tp.chunk_entries(case.adam, case.dim, n)
        n1 = n2 = 0
        for L in lengths:      # the plain loop
            if L > c:
                nch = (L + c - 1) // c
                n1 += nch
                if nch > tp.K_FAN:
                    n2 += (nch + tp.K_FAN - 1) // tp.K_FAN
        assert (n1, n2) == tp.expected_chunks(lengths, c)
        assert n <= case.max_entries
    assert tp.chunk_entries(case.adam, case.dim, case.n) == case.chunk
    # the path the case was built for (launch_table_pass)
    split = case.n > 0 and 2 * case.rows >= case.n and case.kind not in (tp.ADAM_DENSE, tp.ADAM_FULL)
    nvec = case.dim // 4 if case.dim % 4 == 0 else case.dim
    walk = split and case.one_launch and nvec <= 128 and case.n >= case.entry_walk_min and case.kind in tp.ENTRY_WALK_KINDS
    assert case.path == (tp.PATH_ENTRY_WALK if walk else tp.PATH_LIST_WALK if split else tp.PATH_DENSE)


def test_cases_cover_what_they_claim():
    names = " ".join(IDS)
    for word in ("ladder64", "ladder32", "only-row", "adjacent", "merge-n262143", "merge-n262144", "order-no-long-row", "cap-", "geometry-dim1-",
                 "geometry-dim1028-", "regime-list", "regime-shallow", "regime-entry-walk", "leftover"):
        assert word in names
    # the ladder holds every boundary length for both chunk sizes
    for c in (32, 64):
        L = tp.ladder(c)
        for x in (0, 1, c, c + 1, tp.K_FAN * c, tp.K_FAN * c + 1, tp.K_FAN ** 2 * c, tp.K_FAN ** 2 * c + 1):
            assert x in L
    # the entry-walk cases reach the wave ranges of 4, 8 and 16 positions
    sizes = [c.n for c in tp.CASES if c.path == tp.PATH_ENTRY_WALK]
    assert min(sizes) < 65536 and any(65536 <= n < 131072 for n in sizes) and max(sizes) >= 131072


# =====================================================================================================================
# Lazy decay: refresh32 / scalar32 and the cases of tests/test_gpu_lazy_rows.py
# =====================================================================================================================
LAZY = [c for c in tp.CASES if c.lazy]
LAZY_IDS = [c.name for c in LAZY]


def test_refresh_by_hand():
    """3 rows, dim 2, lags 0, 1 and 2 at now = 129: the row one behind sat out update 129, whose factor is at [128 % 128] = [0]; the row
    two behind sat out 128 and 129: slots 127, then 0."""
    f = np.float32
    ring = np.ones(128, f)
    ring[127], ring[0], ring[1], ring[126] = f(0.5), f(0.75), f(0.125), f(0.0625)      # (1 and 126: the slots an off-by-one would read)
    x = np.array([[1.0, -2.0], [3.0, 4.0], [-5.0, 6.0]], f)
    got = tp.refresh32(x, stamp=[129, 128, 127], now=129, ring=ring)
    np.testing.assert_array_equal(got, np.array([[1.0, -2.0], [3.0 * 0.75, 4.0 * 0.75], [-5.0 * 0.5 * 0.75, 6.0 * 0.5 * 0.75]], f))
    assert got.dtype == f and x[1, 0] == 3.0      # (the input is left alone)
    # the order is ascending u: with factors whose product rounds differently in the other order the two orders differ
    a, b = f(1.0 - 2.0 ** -12), f(1.0 + 2.0 ** -12 + 2.0 ** -23)
    ring[127], ring[0] = a, b
    v = np.array([[f(1.0 + 2.0 ** -23)]], f)
    assert tp.refresh32(v, [127], 129, ring)[0, 0] == f(f(v[0, 0] * a) * b)
    # the wrong slot, either way
    np.testing.assert_array_equal(tp.refresh32(x, [129, 128, 127], 129, ring, shift=1)[1], x[1] * f(0.125))
    np.testing.assert_array_equal(tp.refresh32(x, [129, 128, 127], 129, ring, shift=-1)[2], x[2] * f(0.0625) * a)
    # the scalar: lag products of one constant, nothing at all for s = 1
    s = f(0.999)
    np.testing.assert_array_equal(tp.scalar32([2.0, 3.0, 5.0], [0, 1, 2], s), np.array([2.0, f(3.0) * s, f(f(5.0) * s) * s], f))
    np.testing.assert_array_equal(tp.scalar32([2.0, 3.0], [0, 128], 1.0), np.array([2.0, 3.0], f))


@pytest.mark.parametrize("now", tp.LAZY_NOWS)
def test_refresh32_against_the_float64_product(now):
    """lag roundings of half an ulp each: within lag 2^-24 (and a hundredth for the second-order terms) of the float64 product of the
    same factors, for every lag up to the ring's length on either side of the wrap."""
    rs = np.random.RandomState(now % 1000)
    lags = np.minimum(np.repeat(np.arange(0, 129), 3), now)
    stamp = now - lags
    ring = tp.lazy_ring(now % 1000)
    x = rs.standard_normal((lags.size, 7)).astype(np.float32)
    got = tp.refresh32(x, stamp, now, ring).astype(np.float64)
    want = x.astype(np.float64)
    for r in range(lags.size):
        for u in range(stamp[r], now):
            want[r] *= float(ring[u % 128])
    rel = np.abs(got - want) / np.abs(want)
    worst = (rel / np.maximum(lags, 1)[:, None]).max() / 2.0 ** -24
    print("worst error %.3f of lag * 2^-24" % worst)
    assert np.all(rel <= (lags * 2.0 ** -24 * 1.01)[:, None])
    np.testing.assert_array_equal(got[lags == 0], x[lags == 0])
    # the scalar, by the constant of Adam's second moment
    v = rs.uniform(0.5, 2.0, lags.size).astype(np.float32)
    sv = tp.scalar32(v, lags, tp.S_V).astype(np.float64)
    assert np.all(np.abs(sv - v.astype(np.float64) * float(tp.S_V) ** lags) <= lags * 2.0 ** -24 * 1.01 * sv)


@pytest.mark.parametrize("case", LAZY, ids=LAZY_IDS)
def test_a_wrong_ring_slot_or_a_missing_refresh_would_show(case):
    """The sensitivity condition. In every row with entries that is at least one update behind: P refreshed from the neighbouring
    ring slots (u - 1 instead of u) differs from P refreshed properly in at least one element, P and m refreshed differ from P and m
    as stored, and so does the scalar where its factor is not 1. With lambda = 0 the ring holds ones and P has nothing to show: the
    refresh must then leave it bit for bit, which the GPU test asserts anyway. A condition on the drawn case, not a measurement."""
    case.build()
    stale = (case.cnt > 0) & (case.lags > 0)
    assert stale.any() and ((case.cnt > 0) & (case.lags == 0)).any()
    ref_p, ref_m = case.refreshes()
    st = case.start()
    differs = lambda a, b: (a != b).reshape(a.shape[0], -1).any(axis=1)
    if ref_p and case.decay != np.float32(1.0):
        wrong = tp.refresh32(case.P, case.stamp, case.now, case.ring, shift=-1)
        assert differs(wrong, st["P"])[stale].all()
        wrong = tp.refresh32(case.P, case.stamp, case.now, case.ring, shift=1)
        assert differs(wrong, st["P"])[stale].all()
        assert differs(case.P, st["P"])[stale].all()
    if ref_p and case.decay == np.float32(1.0):
        np.testing.assert_array_equal(st["P"], case.P)
    if not ref_p:
        assert st["P"] is case.P
    if ref_m:
        assert differs(case.m, st["m"])[stale].all()
    else:
        assert st["m"] is case.m
    if case.kind in (tp.ADAM_MV, tp.ADAM_SPARSE_ENT):
        assert np.all(st["sc"][stale] != case.sc_in[stale])
    if case.kind == tp.ADAGRAD_ENT:
        np.testing.assert_array_equal(st["sc"], case.sc_in)
    # rows without entries: as stored
    for name, before in (("P", case.P), ("m", case.m), ("sc", case.sc_in)):
        if before is not None:
            np.testing.assert_array_equal(st[name][case.cnt == 0], before[case.cnt == 0])


def test_lazy_cases_cover_every_refresh_site():
    """Every kind, lambda, table, dim, chunk length and `now` class - every kind on each of its tables with lambda > 0 and with
    lambda = 0, and at every `now` with distinct factors - reaches each of the four call sites of refresh_row_state, by the path the
    case was built for (the GPU test asserts that path); the lags of every case are those of LAZY_LAGS cut to `now`, on rows of every
    ladder length."""
    missing = tp.lazy_coverage_wanted() - tp.lazy_coverage(LAZY)
    assert not missing, sorted(missing, key=str)
    # said once more without the table: no kind meets a table, or a kind that refreshes P a `now`, only with a ring of ones
    for name, kind, _, tables in tp.LAZY_VARIANTS:
        mine = [c for c in LAZY if tp.lazy_variant(c) == name]
        for form in tp.LAZY_FORMS:
            sub = [c for c in mine if c.name.startswith("lazy-%s-" % form)]
            assert {(c.table, c.lam > 0) for c in sub} == {(t, lam) for t in tables for lam in (True, False)}
            assert {c.now for c in sub if c.lam > 0} == set(tp.LAZY_NOWS)
    for c in LAZY:
        assert c.path in (tp.PATH_LIST_WALK, tp.PATH_ENTRY_WALK) and 2 * c.rows >= c.n
        assert (c.rows >= c.n) == c.name.endswith("-shallow")
        lengths, lags = np.asarray(c.lengths), c.lags
        want = sorted(set(min(l, c.now) for l in tp.LAZY_LAGS))
        assert sorted(set(lags[lengths > 0])) == want and sorted(set(lags[lengths == 0])) == want
        if c.path == tp.PATH_LIST_WALK:
            top = tp.K_FAN * c.chunk + 1 if c.dim >= 256 else 2 * tp.K_FAN * c.chunk + 1
            for lag in want:
                assert set(lengths[lags == lag]) >= {1, c.chunk, c.chunk + 1, tp.K_FAN * c.chunk + 1, top}
        else:
            assert lengths.max() <= c.chunk
        stamp = c.now - lags
        if c.now == 5:
            assert (stamp == 0).any()
        if c.now == 421:      # a lag range that crosses the wrap of the ring
            assert ((stamp % 128 > c.now % 128) & (lengths > 0)).any()
