"""-m gpu: ONE table pass of the update (csrc/update.hip) on its own - sort, CSR build, chunk order, chunk tree, row formula -
through nvsm_debug_table_pass, row by row against tests/table_pass_reference.py.

Every other check of these kernels goes through whole training steps and compares a norm over the whole table, or two forms of the
same code with each other. Here the row lengths are chosen, not drawn: every boundary of the chunk tree (chunk, chunk + 1,
kFan·chunk + 1, kFan²·chunk + 1, ...) for both chunk lengths, the placements at which csr_bounds_kernel's bisection and wave
ballots end differently, both sides of kCsrMergeMaxEntries, the batch that asks for the most chunks a workspace can be asked for,
thread groups of every shape, and the three walks in both launch forms. The inputs are small dyadic numbers, so the gradient sum g
and the scalar sum q of every row are exact in float32 whatever the order of the additions (test_table_pass_reference.py proves
that per case): one entry dropped, doubled or given to another row changes a row's result, however long the row.

Asserted per case: the path launch_table_pass took and the chunk length; the CSR build's chunk counts against the row lengths and
against the workspace's caps; the arrival counters back at zero; state that is only multiplied and added (P of SGD, m, the per-row
scalar, v) bit for bit; P behind a sqrtf or a division within the allowance of table_pass_reference.Case.reference64; rows without
entries untouched bit for bit (a pass that is not dense) or taken through the same formula with g = q = cnt = 0 (a dense one).
A case with pending lazy decay (tests/test_gpu_lazy_rows.py runs those) also has its stamps compared, and its rows without entries
must keep every bit of P, m, the stored scalar and the stamp, however stale they are."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import TablePassArgs
from tests import table_pass_reference as tp

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data if a is not None else None


def run_table_pass(case, state=None):
    """The case through the hook: (state after the pass, what the hook reports). state: P, m and stamps to start from instead of the
    case's own (the second pass of a sequence)."""
    case.build()
    state = state or {}
    P = state.get("P", case.P).copy()
    m = state.get("m", case.m)      # (given to a kind that has no use for it, it must come back as it went in)
    m = m.copy() if m is not None else None
    v = case.v.copy() if case.v is not None else None
    sc_in = sc_out = None
    if case.kind in tp.USES_SC:
        sc_in = case.sc_in.copy()
        sc_out = sc_in if case.kind == tp.SCALAR_ACC else np.full(case.rows, tp.SENTINEL, np.float32)      # the accumulator pass works in place
    stamp = ring = stamp_out = None
    if case.lazy:
        stamp, ring = case.stamp.copy(), case.ring.copy()
        stamp_out = np.full(case.rows, -7, np.int32)
    path, chunk, max1, max2, left = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    num_chunks = (C.c_int * 2)(-1, -1)
    a = TablePassArgs(
        table=case.table, kind=case.kind, rows=case.rows, dim=case.dim, n=case.n, keys=_ptr(case.keys), div=case.div, num_src=case.num_src,
        X=_ptr(case.X), coef=_ptr(case.coefs), sq_src=_ptr(case.sq_src), src_scale=_ptr(case.scale),
        P=_ptr(P), m=_ptr(m), v=_ptr(v), sc_in=_ptr(sc_in), sc_out=_ptr(sc_out),
        lr=float(case.lr), lambda_=float(np.float32(case.lam)), decay=float(case.decay), bc=float(case.bc), dense=case.dense, wide=case.wide, nt=case.nt,
        max_entries=case.max_entries, adam=int(case.adam), one_launch=case.one_launch, chunk_order=case.chunk_order,
        fill_in_bounds=case.fill_in_bounds, entry_walk_min=case.entry_walk_min,
        prev_n=case.prev_n, prev_keys=_ptr(case.prev_keys),
        path=C.pointer(path), chunk=C.pointer(chunk), num_chunks=num_chunks, max_chunks=C.pointer(max1), max_chunks2=C.pointer(max2),
        arrive_left=C.pointer(left), stamp=_ptr(stamp), lazy_decay=_ptr(ring), now=case.now, stamp_out=_ptr(stamp_out))
    ca._lib.check(ca.lib().nvsm_debug_table_pass(C.byref(a)))
    report = dict(path=path.value, chunk=chunk.value, num_chunks=(num_chunks[0], num_chunks[1]), max_chunks=max1.value, max_chunks2=max2.value,
                  arrive_left=left.value)
    if case.lazy:
        assert np.array_equal(stamp, case.stamp) and np.array_equal(ring, case.ring), "the hook wrote to its inputs"
    return dict(P=P, m=m, v=v, sc=sc_out, stamp=stamp_out), report


def _rows_that_differ(got, want):
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    return bad


def check_case(case):
    got, rep = run_table_pass(case)
    ref = case.reference32()
    print("%s: n %d rows %d chunk %d path %d chunks %s of (%d, %d)" % (case.name, case.n, case.rows, rep["chunk"], rep["path"], rep["num_chunks"],
                                                                       rep["max_chunks"], rep["max_chunks2"]))
    # ---- structure ----
    assert rep["path"] == case.path, "the case was built for another path"
    assert rep["chunk"] == case.chunk
    want_chunks = tp.expected_chunks(case.lengths, case.chunk)
    assert rep["num_chunks"] == want_chunks
    assert want_chunks[0] <= rep["max_chunks"] and want_chunks[1] <= rep["max_chunks2"], "the workspace's caps are below what the batch asks for"
    assert rep["arrive_left"] == 0
    # ---- bit for bit ----
    lengths = np.asarray(case.lengths)
    exact = ["sc", "m", "v"] + (["P"] if case.kind not in tp.SQRT_DIV_KINDS else [])
    for name in exact:
        if ref[name] is None:
            continue
        bad = _rows_that_differ(got[name], ref[name])
        assert bad.size == 0, "%s differs in %d rows, the first of %d entries (rows %s, lengths %s)" % (
            name, bad.size, lengths[bad[0]], bad[:8], lengths[bad[:8]])
    # ---- bounded: P behind sqrtf / a division ----
    if case.kind in tp.SQRT_DIV_KINDS:
        want, tol = case.reference64(ref)
        err = np.abs(got["P"].astype(np.float64) - want)
        over = err > tol      # (a NaN fails: the comparison is false for it only when negated)
        ok = err <= tol
        assert ok.all(), "P outside its allowance in rows %s (lengths %s): worst %.3g of the allowance" % (
            np.flatnonzero(~ok.all(axis=1))[:8], lengths[np.flatnonzero(~ok.all(axis=1))[:8]], np.nanmax(err[over] / tol[over]) if over.any() else np.nan)
        _, touch = case.visited()
        np.testing.assert_array_equal(got["P"][~touch], case.P[~touch])
        rep["p_share"] = float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0
        print("   P: worst error %.3f of the allowance" % rep["p_share"] if (tol > 0).any() else "   P: untouched")
    # ---- rows without entries of a pass that is not dense: nothing moves (also implied above; said once more, on the inputs) ----
    if not case.dense or case.lazy:
        empty = lengths == 0
        for name, before in (("P", case.P), ("m", case.m), ("v", case.v)):
            if before is not None:
                np.testing.assert_array_equal(got[name][empty], before[empty])
        if got["sc"] is not None and case.kind != tp.SCALAR_ACC and not case.lazy:
            assert np.all(got["sc"][empty] == tp.SENTINEL)
    # ---- pending lazy decay: the stamps; rows without entries keep the stored scalar and the stamp; a pass that has no use for P
    #      (the moments pass of sparse Adam's words update) leaves all of it alone, stale rows included ----
    if case.lazy:
        empty = lengths == 0
        np.testing.assert_array_equal(got["stamp"], case.stamps_after())
        np.testing.assert_array_equal(got["stamp"][empty], case.stamp[empty])
        if got["sc"] is not None:
            np.testing.assert_array_equal(got["sc"][empty], case.sc_in[empty])
        if case.kind not in tp.USES_P:
            np.testing.assert_array_equal(got["P"], case.P)
    return got, rep


def _select(prefix):
    cases = [c for c in tp.CASES if c.name.startswith(prefix)]
    assert cases
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


@_select("ladder")
def test_length_ladder(case):
    """Rows of 0, 1, 2, c-1, c, c+1, 2c-1, 2c, 2c+1, kFan·c-1, kFan·c, kFan·c+1, (kFan+1)·c, (kFan+1)·c+1, 2·kFan·c, 2·kFan·c+1, kFan²·c and
    kFan²·c+1 entries, c = 64 and 32, longest row first or last, every kind, both tables, wts / no wts / src_scale, div 1, 10, 17."""
    check_case(case)


@_select("only-row")
def test_single_long_row(case):
    check_case(case)


@_select("empty-batch")
def test_batch_without_entries(case):
    check_case(case)


@_select("two-c32+1")
def test_two_long_rows_end_in_one_wave(case):
    check_case(case)


@_select("merge")
def test_either_side_of_the_merged_csr_build(case):
    """n = 262 143: the bounds kernel reserves the chunks; n = 262 144: csr_chunks_kernel does."""
    check_case(case)


@_select("order")
def test_chunk_order(case):
    check_case(case)


@_select("fill-in-bounds")
def test_descriptors_written_by_the_bounds_kernel(case):
    check_case(case)


@_select("cap")
def test_most_chunks_a_workspace_can_be_asked_for(case):
    """floor(max_entries / (c + 1)) rows of c + 1 entries, two chunks each: 2 / (c + 1) chunks per entry, which no other row length
    reaches. Beyond max_chunks the kernels drop descriptors silently - every row exact means none was dropped."""
    check_case(case)


@_select("geometry")
def test_thread_group_geometry(case):
    check_case(case)


@_select("regime")
def test_walks(case):
    """Dense walk, list walk, shallow list walk and entry walk, one launch and three, dense or not - the path is asserted."""
    check_case(case)


@_select("leftover")
def test_counters_left_by_the_previous_batch(case):
    check_case(case)


def test_the_form_comes_from_the_case_alone():
    """The entry walk exists in the one-launch form only: whatever nvsm_debug_set_table_pass_form last said, the case's field decides."""
    walk = next(c for c in tp.CASES if c.path == tp.PATH_ENTRY_WALK and c.n < 10000)
    try:
        for form in (0, 1):
            ca._lib.check(ca.lib().nvsm_debug_set_table_pass_form(form))
            check_case(walk)
    finally:
        ca._lib.check(ca.lib().nvsm_debug_set_table_pass_form(1))


def test_hook_refuses_keys_outside_the_table():
    bad = tp.Case("bad-key", [3, 2], tp.SGD, dim=4).build()
    bad.keys = bad.keys.copy()
    bad.keys[0] = 2
    with pytest.raises(ca._lib.NvsmError):
        run_table_pass(bad)
