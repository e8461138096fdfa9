"""The round layout of the retrieval calls (rank_layout / rank_layout_candidates of ranking.cpp, through nvsm_debug_rank_layout of the
test-hooks library: host arithmetic only, no GPU) against a restatement of DESIGN.md §9 "Dispatch by Q and k", against the rule's
invariants over a sweep, and against fixed values computed from the rule as it stood before the rounds shared one function."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import check

ROUND, ROUND_CANDIDATES = 256, 4096        # queries a round starts from
ALIGN = 4096                               # rows of a slab: a multiple of this, unless one slab holds every row or the cap decides
KEYS = 1 << 25                             # sort keys of a round, unless one query alone has more


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def restated(rows, k, queries, mb, cap=0):
    """(qn, S, ld, n_keys, npad)"""
    floats = mb << 18
    qn = min(ROUND, queries)
    while True:
        S = min(rows, max(ALIGN, floats // qn // ALIGN * ALIGN))
        if cap:
            S = min(S, cap)
        n_keys = sum(min(k, min(S, rows - d0)) for d0 in range(0, rows, S))
        npad = pow2_at_least(n_keys)
        if qn * npad <= KEYS or qn == 1:
            return qn, S, (S + 3) // 4 * 4, n_keys, npad
        qn = (qn + 1) // 2


def restated_candidates(lengths):
    qn = min(ROUND_CANDIDATES, len(lengths))
    while True:
        npad = pow2_at_least(max([1] + list(lengths[:qn])))
        if qn * npad <= KEYS or qn == 1:
            return qn, npad
        qn = (qn + 1) // 2


def layout(rows, k, queries, mb, cap=0, lengths=None):
    out = (C.c_int64 * 5)()
    arr = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
    ptr = None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_int64))
    check(ca.lib().nvsm_debug_rank_layout(rows, k, queries, mb, cap, ptr, out))
    return tuple(out)


# (rows, k, queries, MB[, cap]) -> (qn, S, n_keys, npad)
FIXED = [
    ((9001, 10, 256, 1), (256, 4096, 30, 32)),
    ((9001, 9001, 256, 1), (256, 4096, 9001, 16384)),
    ((200000, 131073, 256, 256), (128, 200000, 131073, 262144)),
    ((200000, 200000, 256, 1), (128, 4096, 200000, 262144)),
    ((2000000, 1000, 256, 256), (256, 262144, 8000, 8192)),
    ((1, 1, 1, 256), (1, 1, 1, 1)),
    ((4097, 5, 44, 1), (44, 4096, 6, 8)),
    ((40000000, 40000000, 1, 256), (1, 40000000, 40000000, 67108864)),
    ((50000, 7, 256, 1, 16384), (256, 4096, 91, 128)),
]


@pytest.mark.parametrize("args,expected", FIXED)
def test_fixed_values(args, expected):
    qn, S, ld, n_keys, npad = layout(*args)
    assert (qn, S, n_keys, npad) == expected
    assert ld == (S + 3) // 4 * 4
    if args[0] <= 2000000:                 # (the restatement walks the slabs one by one)
        assert restated(*args) == (qn, S, ld, n_keys, npad)


def test_invariants_and_the_restatement_over_a_sweep():
    rows_ = (1, 3, 4095, 4096, 4097, 9001, 65537, 200000, 2000000)
    queries_ = (1, 2, 31, 32, 33, 255, 256, 257, 300, 5000)
    mbs = (1, 3, 64, 256)
    caps = (0, 1000, 4096, 16384, 65536, 218453)
    seen_halving = seen_cap = 0
    for rows, queries, mb, cap in itertools.product(rows_, queries_, mbs, caps):
        for k in sorted({1, 2, 10, 1000, 4096, 4097, 131072, 131073, rows // 2, rows - 1, rows}):
            if not 1 <= k <= rows:
                continue
            qn, S, ld, n_keys, npad = got = layout(rows, k, queries, mb, cap)
            assert got == restated(rows, k, queries, mb, cap), (rows, k, queries, mb, cap)
            assert 1 <= qn <= min(256, queries) and 1 <= S <= rows
            assert S == rows or S % 4096 == 0 or S == cap
            assert n_keys == sum(min(k, min(S, rows - d0)) for d0 in range(0, rows, S))
            assert npad >= n_keys and npad & (npad - 1) == 0 and (npad == 1 or npad // 2 < n_keys)
            assert qn * npad <= 1 << 25 or qn == 1
            assert ld == (S + 3) // 4 * 4
            seen_halving += qn < min(256, queries)
            seen_cap += S == cap and S != rows and S % 4096 != 0
    assert seen_halving > 0 and seen_cap > 0      # the sweep reaches the halving branch and a slab that the cap alone decides


def test_candidate_lists():
    lengths = np.ones(4096, np.int64)
    lengths[2047] = 10000                  # the longest list, among the first 2048
    lengths[3000] = 9000
    assert layout(0, 0, 4096, 0, lengths=lengths) == (2048, 0, 0, 0, 16384) and restated_candidates(lengths) == (2048, 16384)
    lengths[2047], lengths[2048] = 1, 10000          # ... behind them: the halved round no longer holds it
    assert layout(0, 0, 4096, 0, lengths=lengths) == (2048, 0, 0, 0, 1)
    cases = [np.zeros(3, np.int64), np.array([5]), np.full(5000, 8192), np.full(4096, 8193), np.array([1 << 26, 3]),
             np.random.RandomState(1).randint(0, 70000, 4096)]
    for lengths in cases:
        qn, S, ld, n_keys, npad = layout(0, 0, len(lengths), 0, lengths=lengths)
        assert (qn, npad) == restated_candidates(lengths) and (S, ld, n_keys) == (0, 0, 0)
        assert qn * npad <= 1 << 25 or qn == 1


def test_refusals():
    L = ca.lib()
    out = (C.c_int64 * 5)()
    for args in ((0, 1, 1, 1, 0), (5, 0, 1, 1, 0), (5, 6, 1, 1, 0), (5, 1, 0, 1, 0), (5, 1, 1, 0, 0), (5, 1, 1, 1, -1)):
        assert L.nvsm_debug_rank_layout(*args, None, out) == 1 and b"rank_layout" in L.nvsm_last_error()
    assert L.nvsm_debug_rank_layout(5, 1, 1, 1, 0, None, None) == 1
