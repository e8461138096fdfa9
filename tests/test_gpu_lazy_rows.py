"""-m gpu: lazy dense decay (csrc/kernels.h) row by row - the pending factors a row pass applies before the optimiser's formula,
the refresh kernels, and the lazy word gather - each on its own through a hook, against tests/table_pass_reference.py.

tests/test_gpu_lazy.py trains an eager and a lazy handle side by side: the lags there are whatever the drawn batches produce, and a
wrong factor is one multiplication by a number near 1 somewhere in a table. Here every row's lag, its length in the chunk tree and
the place of `now` in the factor ring are chosen:

  a. nvsm_debug_table_pass with stamps: refresh_row_state at its four call sites (row_pass_kernel, the short rows of
     table_pass_body, the long-row finish behind the chunk tree, entry_walk_kernel), for the six passes the model runs lazily, on
     rows of every boundary length at lags 0, 1, 64, 127 and 128, `now` = 5 (a young table), 128, 421 (the lag range crosses the
     ring's wrap) and 1 000 003 - each kind at each of them with lambda > 0, on both tables, and with lambda = 0 (a ring of ones) on
     both; split passes and shallow ones (rows >= entries, what a table of millions of rows runs); thread groups of 3 and 75 lanes
     that straddle waves (dim 12, 300). P of SGD, m, the stored
     scalar and the stamps bit for bit, P behind sqrtf / a division within Case.reference64's allowance; rows without entries keep
     every bit, stamp included. The factor ring holds 128 distinct factors (test_table_pass_reference.py: a neighbouring slot would
     change every stale row). The sparse-Adam words sequence - moments pass, then the wide SGD pass on the same stamps - refreshes m
     once and P once.
  b. nvsm_debug_lazy_refresh: lazy_refresh_kernel<1 / 4> and lazy_scalar_snapshot_kernel bit for bit against refresh32 / scalar32,
     all rows or a list whose count is read from the device; rows that are not listed, the guards and (scalars_only) everything
     but the snapshot untouched.
  c. nvsm_debug_gather_mean_lazy bit-equal to the eager gather on refresh32(table) - "round alike", gather_gemm.hip - and the table
     unwritten.
  d. the hooks refuse stamps outside the contract before anything is launched.

The closing test is bookkeeping, not observation: which call site a case reaches follows from the launch form the case asks for, the
path and chunk length the hook reports (both asserted) and the case's row lengths - the kernels do not report where they refreshed.
It says that no case failed or was deselected, and so that the plan test_table_pass_reference.py checks without a GPU was carried out.

What five deliberately broken builds (never committed) do to this file is recorded in profiles/NOTES_lazy_rows.md."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import LazyRefreshArgs
from tests import table_pass_reference as tp
from tests.test_gpu_table_pass import check_case, run_table_pass

pytestmark = pytest.mark.gpu

F32 = np.float32
LAZY = [c for c in tp.CASES if c.lazy]
SEEN = set()                    # (site, axis, value) of the cases that passed in this session
WORST = {}                      # worst P error as a share of the reference64 allowance, per kind
REFRESH_LAGS = (0, 1, 2, 63, 64, 65, 127, 128)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ptr(a):
    return a.ctypes.data if a is not None else None


# =====================================================================================================================
# a. the table pass with pending decay
# =====================================================================================================================
def _form(form):
    cases = [c for c in LAZY if c.name.startswith("lazy-%s-" % form)]
    assert len(cases) == len(tp.LAZY_VARIANTS) * len(tp.LAZY_PLAN)
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


def _check(case):
    got, rep = check_case(case)      # (asserts the path the case was built for)
    SEEN.update(tp.lazy_coverage([case], sites=case.sites(path=rep["path"], chunk=rep["chunk"])))
    if "p_share" in rep:
        WORST[tp.KIND_NAMES[case.kind]] = max(WORST.get(tp.KIND_NAMES[case.kind], 0.0), rep["p_share"])
    return got


@_form("one")
def test_list_walk_one_launch(case):
    """table_pass_body: the rows of at most a chunk, and the long-row finish behind the chunk tree - c, c + 1, kFan c + 1, 2 kFan c + 1
    entries at every lag."""
    assert case.sites() == {tp.SITE_BODY_SHORT, tp.SITE_LONG_FINISH}
    _check(case)


@_form("three")
def test_list_walk_three_launches(case):
    """row_pass_kernel behind chunk_pass_kernel / chunk2_pass_kernel."""
    assert case.sites() == {tp.SITE_ROW_PASS}
    _check(case)


@_form("walk")
def test_entry_walk(case):
    """entry_walk_kernel at the short-row lengths."""
    assert case.sites() == {tp.SITE_ENTRY_WALK}
    _check(case)


@pytest.mark.parametrize("dim,now,one_launch", [(300, 421, 1), (12, 128, 0), (128, 1000003, 1), (7, 5, 1)])
def test_sparse_adam_words_sequence(dim, now, one_launch):
    """Model::update_words, sparse Adam: the moments pass (ROW_ADAM_MV) and the wide SGD pass behind it carry the SAME pending view -
    the stamps are set after the second. The first must refresh m and leave P alone, the second refresh P and leave m alone: after
    both, each has had its factors exactly once."""
    lengths, lags = tp.lazy_layout(tp.lazy_lengths("one", tp.CHUNK, dim))
    kw = dict(table=0, dim=dim, div=10, adam=True, one_launch=one_launch, dense=1, lam=0.01, path=tp.PATH_LIST_WALK, lags=lags, now=now, seed=300 + dim)
    mv = tp.Case("seq-mv-dim%d" % dim, lengths, tp.ADAM_MV, **kw)
    got_mv = check_case(mv)[0]      # (m and the scalar against the reference bit for bit, P bit-identical to what went in, stale rows included)
    stale = (np.asarray(lengths) > 0) & (mv.lags > 0)
    assert (got_mv["m"][stale] != mv.m[stale]).any(axis=1).all()
    table, stamp, ring = mv.P.copy(), mv.stamp.copy(), mv.ring.copy()      # (one case's arrays are alive at a time)
    # the second pass: another source (the window-averaged direction), the table as the moments pass left it, the stamps as they WERE
    u = tp.Case("seq-u-dim%d" % dim, lengths, tp.SGD, wide=1, **kw).build()
    u.P = table      # (both cases describe one table)
    assert np.array_equal(u.stamp, stamp) and np.array_equal(u.ring, ring)
    got, rep = run_table_pass(u, state=dict(P=got_mv["P"], m=got_mv["m"]))      # (the model hands this pass the moments too: RowPassArgs::m)
    assert rep["path"] == tp.PATH_LIST_WALK
    # P: the factors once, from the bits the table held before the update, then the step; m: not once more
    np.testing.assert_array_equal(_bits(got["P"]), _bits(u.reference32()["P"]))
    np.testing.assert_array_equal(_bits(got["m"]), _bits(got_mv["m"]))
    np.testing.assert_array_equal(got["stamp"], u.stamps_after())
    # refreshed twice would be this, and must differ wherever a row was stale
    twice = tp.refresh32(u.start()["P"], u.stamp, u.now, u.ring)
    assert (twice[stale] != u.start()["P"][stale]).any(axis=1).all()


# =====================================================================================================================
# b. launch_lazy_refresh
# =====================================================================================================================
def run_refresh(dim, now, listed, with_m, s_v, scalars_only, seed):
    rows = 300
    rs = np.random.RandomState(seed)
    lags = np.minimum(np.array([REFRESH_LAGS[r % len(REFRESH_LAGS)] for r in range(rows)]), now)
    stamp = (now - lags).astype(np.int32)
    ring = tp.lazy_ring(seed)
    P = rs.standard_normal((rows + 1, dim)).astype(F32)
    m = rs.standard_normal((rows + 1, dim)).astype(F32) if with_m else None
    sc = rs.uniform(0.5, 2.0, rows + 1).astype(F32)
    snap = np.zeros(rows + 1, F32)
    lst = None
    if listed:
        lst = np.ascontiguousarray(rs.permutation(rows)[: rows // 3].astype(np.int32))
    before = dict(P=P.copy(), m=None if m is None else m.copy(), sc=sc.copy())
    stamp_out = np.full(rows, -7, np.int32)
    a = LazyRefreshArgs(rows=rows, dim=dim, P=_ptr(P), m=_ptr(m), sc=_ptr(sc), sc_snapshot=_ptr(snap), stamp=_ptr(stamp), stamp_out=_ptr(stamp_out),
                        list=_ptr(lst), n_list=0 if lst is None else lst.size, now=now, s_m=float(tp.S_M), s_v=float(s_v), decay=_ptr(ring),
                        scalars_only=int(scalars_only))
    ca._lib.check(ca.lib().nvsm_debug_lazy_refresh(C.byref(a)))
    on = np.zeros(rows, bool)
    on[lst if listed else slice(None)] = True
    return dict(P=P, m=m, sc=sc, snap=snap, stamp=stamp_out), before, dict(on=on, lags=lags, stamp=stamp, ring=ring, rows=rows)


@pytest.mark.parametrize("scalars_only", [0, 1], ids=["full", "scalars_only"])
@pytest.mark.parametrize("listed", [0, 1], ids=["all", "list"])
@pytest.mark.parametrize("dim,now,with_m,s_v", [(3, 5, 1, tp.S_V), (7, 128, 0, 1.0), (64, 421, 1, 1.0), (256, 1000003, 1, tp.S_V),
                                                (260, 421, 0, tp.S_V), (300, 128, 1, tp.S_V), (300, 5, 0, 1.0), (260, 1000003, 1, 1.0)])
def test_lazy_refresh(dim, now, with_m, s_v, listed, scalars_only):
    """300 rows with lags 0, 1, 2, 63, 64, 65, 127, 128 in turn (cut to `now`); dim 260 and 300 take the column loop past 64 V columns."""
    got, before, x = run_refresh(dim, now, listed, with_m, s_v, scalars_only, seed=dim + now % 1000 + 17 * listed)
    rows, on, nan = x["rows"], x["on"], np.uint32(0xFFFFFFFF)
    on1 = np.r_[on, False]      # (the guard row is never listed)
    want_sc = np.where(on, tp.scalar32(before["sc"][:rows], x["lags"], s_v), before["sc"][:rows])
    # the snapshot: the refreshed scalar of the listed rows, 0xFF bytes everywhere else
    np.testing.assert_array_equal(_bits(got["snap"][:rows])[on], _bits(want_sc)[on])
    assert np.all(_bits(got["snap"])[~on1] == nan)
    if scalars_only:
        np.testing.assert_array_equal(_bits(got["P"]), _bits(before["P"]))
        if with_m:
            np.testing.assert_array_equal(_bits(got["m"]), _bits(before["m"]))
        np.testing.assert_array_equal(_bits(got["sc"]), _bits(before["sc"]))      # (the stored scalar stays: the row pass writes the new one)
        np.testing.assert_array_equal(got["stamp"], x["stamp"])
        return
    want_P = np.where(on[:, None], tp.refresh32(before["P"][:rows], x["stamp"], now, x["ring"]), before["P"][:rows])
    np.testing.assert_array_equal(_bits(got["P"][:rows]), _bits(want_P))
    if with_m:
        want_m = np.where(on[:, None], tp.refresh32(before["m"][:rows], x["stamp"], now, np.full(128, tp.S_M, F32)), before["m"][:rows])
        np.testing.assert_array_equal(_bits(got["m"][:rows]), _bits(want_m))
        np.testing.assert_array_equal(_bits(got["m"][rows]), _bits(before["m"][rows]))
    np.testing.assert_array_equal(_bits(got["sc"][:rows]), _bits(want_sc))
    np.testing.assert_array_equal(got["stamp"], np.where(on, now, x["stamp"]))
    # the guards
    np.testing.assert_array_equal(_bits(got["P"][rows]), _bits(before["P"][rows]))
    assert _bits(got["sc"])[rows] == _bits(before["sc"])[rows]
    # the case can tell: every stale listed row moved
    stale = on & (x["lags"] > 0)
    assert (want_P[stale] != before["P"][:rows][stale]).any(axis=1).all()


# =====================================================================================================================
# c. the lazy word gather
# =====================================================================================================================
@pytest.mark.parametrize("weighted", [0, 1], ids=["plain", "weighted"])
@pytest.mark.parametrize("window", list(range(1, 12)) + [16])
@pytest.mark.parametrize("dim,now", [(3, 5), (7, 128), (12, 421), (128, 1000003), (300, 421)])
def test_lazy_gather_rounds_like_the_eager_gather_of_the_refreshed_table(dim, now, window, weighted):
    """Windows 1 .. 11 and 16: U = 1 .. 5 rows in flight with whole and short last rounds, either side of 5, 10 and 15 words."""
    rows, n_out = 64, 70
    rs = np.random.RandomState(1000 * dim + 10 * window + weighted)
    lags = np.minimum(np.array([REFRESH_LAGS[r % len(REFRESH_LAGS)] for r in range(rows)]), now)
    stamp = (now - lags).astype(np.int32)
    ring = tp.lazy_ring(dim + window)
    table = rs.uniform(-1, 1, (rows, dim)).astype(F32)
    idx = rs.randint(0, rows, (n_out, window)).astype(np.int64)
    hot = 7                                  # lag 128 (row 7 of the cycle): twice within a window, and in several outputs
    assert lags[hot] == min(128, now)
    idx[::5, 0] = hot
    if window > 1:
        idx[::10, window - 1] = hot
    w = rs.uniform(0, 2, (n_out, window)).astype(F32) if weighted else None
    out, table_out = np.zeros((n_out, dim), F32), np.zeros((rows, dim), F32)
    ca._lib.check(ca.lib().nvsm_debug_gather_mean_lazy(rows, dim, _ptr(table), _ptr(idx), _ptr(w), window, n_out, _ptr(stamp), _ptr(ring), now,
                                                       _ptr(out), _ptr(table_out)))
    fresh = tp.refresh32(table, stamp, now, ring)
    want = np.zeros((n_out, dim), F32)
    ca._lib.check(ca.lib().nvsm_debug_gather_mean(rows, dim, _ptr(fresh), _ptr(idx), _ptr(w), window, n_out, _ptr(want)))
    np.testing.assert_array_equal(_bits(out), _bits(want))
    np.testing.assert_array_equal(_bits(table_out), _bits(table))      # (a reader writes nothing back)
    assert (fresh[lags > 0] != table[lags > 0]).any(axis=1).all() and np.isfinite(out).all()


# =====================================================================================================================
# d. refusals
# =====================================================================================================================
def _refused(case, status):
    with pytest.raises(ca._lib.NvsmError) as e:
        run_table_pass(case)
    assert e.value.status == status, e.value


def _small(kind=tp.SGD, lags=(0, 1, 2, 3), now=200, **kw):
    return tp.Case("refusal", [3, 0, 2, 1], kind, dim=4, dense=1, lam=0.01, path=tp.PATH_LIST_WALK, chunk=32, lags=list(lags), now=now, **kw).build()


def test_hooks_refuse_stamps_outside_the_contract():
    """The row pass does not clamp: a row further behind than the ring is long would read a stale slot. Refused on the host."""
    INVALID, UNSUPPORTED = 1, 2
    run_table_pass(_small())      # (the case itself is fine)
    for stamp0 in (200 - 129, 201, -1):      # a lag of 129; ahead of now; negative
        bad = _small()
        bad.stamp = bad.stamp.copy()
        bad.stamp[0] = stamp0
        _refused(bad, INVALID)
    # a kind the model never runs lazily, with stamps
    ok = _small()
    stamp, ring, now = ok.stamp.copy(), ok.ring.copy(), ok.now      # (one case's arrays are alive at a time)
    for kind in (tp.ADAM_DENSE, tp.ADAM_FULL, tp.SCALAR_ACC):
        other = tp.Case("refusal-kind", [3, 0, 2, 1], kind, dim=4, dense=0 if kind == tp.SCALAR_ACC else 1, adam=kind != tp.SCALAR_ACC,
                        chunk=32 if kind == tp.SCALAR_ACC else 64).build()
        other.lazy, other.stamp, other.ring, other.now = True, stamp, ring, now
        _refused(other, UNSUPPORTED)
    # the two other hooks
    ring, table = tp.lazy_ring(1), np.ones((4, 4), F32)
    idx, out = np.zeros((2, 2), np.int64), np.zeros((2, 4), F32)
    for stamps in ([71, 200, 200, 200], [201, 200, 200, 200], [-1, 200, 200, 200]):
        st = np.array(stamps, np.int32)
        assert ca.lib().nvsm_debug_gather_mean_lazy(4, 4, _ptr(table), _ptr(idx), None, 2, 2, _ptr(st), _ptr(ring), 200, _ptr(out), _ptr(table.copy())) == INVALID
        P, so = np.ones((5, 4), F32), np.zeros(4, np.int32)
        a = LazyRefreshArgs(rows=4, dim=4, P=_ptr(P), stamp=_ptr(st), stamp_out=_ptr(so), now=200, s_m=1.0, s_v=1.0, decay=_ptr(ring))
        assert ca.lib().nvsm_debug_lazy_refresh(C.byref(a)) == INVALID
        assert np.all(P == 1.0)


# =====================================================================================================================
def test_every_refresh_site_was_reached_by_every_kind_at_every_now():
    """The table the cases above filled in as they passed: every kind, lambda, table, dim, chunk length and `now`, shallow or not,
    every kind on each of its tables with lambda > 0 and with lambda = 0, and every kind at every `now` with distinct factors, at each
    of the four call sites of refresh_row_state (the entry walk takes no dim 300). The sites are derived, not observed: see the
    module docstring."""
    want = tp.lazy_coverage_wanted()
    assert len({s for s, _, _ in want}) == 4
    if SEEN:                                                       # (empty when this test is selected on its own)
        assert want <= SEEN, sorted(want - SEEN, key=str)
        print("lazy rows: %d of %d (site, axis, value) planned and passed; worst P error as a share of the allowance: %s" % (
            len(want & SEEN), len(want), " ".join("%s %.3f" % kv for kv in sorted(WORST.items()))))
