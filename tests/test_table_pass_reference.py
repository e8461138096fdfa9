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
    if case.kind in tp.SQRT_DIV_KINDS:
        new, tol = case.reference64(ref)
        assert np.all(np.abs(ref["P"].astype(np.float64) - new) <= tol)
        np.testing.assert_array_equal(ref["P"][~touch], case.P[~touch])
    if case.kind == tp.SGD:      # two products and a sum: an ulp and a half of the larger side
        exact = np.where(touch[:, None], case.P.astype(np.float64) * float(case.decay) + float(case.lr) * case.g, case.P)
        assert np.all(np.abs(ref["P"] - exact) <= 2.0 ** -22 * np.maximum(np.abs(exact), np.abs(float(case.lr) * case.g)))
    if case.kind in (tp.ADAGRAD_ENT, tp.SCALAR_ACC):
        exact = case.sc_in.astype(np.float64) + case.q
        assert np.all(np.abs(ref["sc"][vis] - exact[vis]) <= 2.0 ** -24 * np.abs(exact[vis]))
        assert np.all(ref["sc"][vis] > 0)
    if case.kind in (tp.ADAM_MV, tp.ADAM_SPARSE_ENT, tp.ADAM_DENSE):
        exact = case.sc_in.astype(np.float64) * float(tp.S_V) + float(tp.ONE_M_B2) * case.q
        assert np.all(np.abs(ref["sc"][vis] - exact[vis]) <= 2.0 ** -22 * (np.abs(case.sc_in[vis]) + np.abs(case.q[vis])))
        assert np.all(ref["sc"][vis] > 0)
    if case.kind in tp.USES_M and case.kind != tp.ADAM_FULL:
        exact = case.m.astype(np.float64) * float(tp.S_M) + float(tp.ONE_M_B1) * case.g
        assert np.all(np.abs(ref["m"] - exact)[vis] <= (2.0 ** -22 * (np.abs(case.m) + np.abs(float(tp.ONE_M_B1) * case.g)))[vis])
    for name in ("P", "m", "v", "sc"):
        assert ref[name] is None or np.all(np.isfinite(ref[name]))
    # rows the pass does not visit keep everything
    for name, before in (("P", case.P), ("m", case.m), ("v", case.v)):
        if before is not None:
            np.testing.assert_array_equal(ref[name][~vis], before[~vis])


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
