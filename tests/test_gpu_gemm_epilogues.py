"""-m gpu: the epilogues the four batch-sized projection kernels fuse into their product (gemm_rows / gemm_rsplit / gemm_split /
gemm_tstat .hip, and the tiled kernel they fall back to), one named launcher at a time through nvsm_debug_gemm_epilogue, at every
shape of the table in tests/test_gemm_plans.py (its docstring says why those shapes, and proves without a GPU that they reach every
instantiation and both sides of every refusal edge).

References are fp64 numpy; none is the code under test. Bounds are derived, not fitted (u = 2^-24, the fp32 unit roundoff):
  C          against alpha · A·B + bias. Exact-fp32 kernels (rows, tstat, tiled): rel-L2 < 2e-6. Split-bf16 kernels (rsplit, split):
             |C − ref| < 1.5e-6 · |alpha| Σ|a||b| with six and with nine partial products (tests/test_gpu_parity.py's bounds) — and,
             with a bias only, + 2·u·|ref|: the two roundings that follow the product, alpha · acc and + bias, are relative to the
             stored value, which the bias can make far larger than the row's Σ|a||b| (K = 16, operands over sixteen binades:
             3.2e-6 · Σ|a||b| measured on gemm_split at N = 256, from the rounding of the sum alone). The product's own term is
             the suite's, unchanged.
  colstats   against fp64 Σ and Σ² over the rows of the RETURNED fp32 C (the unit under test is the summation): t·u·Σ|C| and
             t·u·ΣC², t = the rows a kernel adds in fp32 before it goes to fp64 (t_rows below cites each epilogue). Padding
             columns and rows >= M must add nothing: M is ragged, the buffers start as NaN.
  rowsq      against fp64 rowsq_scale · Σ_n C² of the returned C: (N + 2)·u relative — N − 1 additions in any order, the squares,
             the scale.
  fused BN   dx (A after the launch) against invσ·(dy − (dβ + x̂·dγ)/n) in fp64 from the same inputs, dβ = fl32(sums[0]),
             dγ = fl32(sums[1]): 8·u·Σ|terms|. The kernels write  xhat = (x − μ)·is;  is·(dy − (dβ + xhat·dγ)·inv_n)  with
             inv_n = fl32(1/n): the longest chain, the dγ term's, passes 8 roundings — x − μ, ·is, ·dγ, dβ +, inv_n itself,
             ·inv_n, dy −, is· . dbeta, dgamma, grad_bias == fl32(sums) exactly; C against the fp64 product of the RETURNED dx.
             Bias-gradient-only: A comes back bit-identical, grad_bias == fl32(sums[0]).
  gather     the phrases (A after the launch) bit-equal to nvsm_debug_gather_mean's; C against the fp64 product of those phrases.
  refusals   "launched" is false and every output still holds its NaN fill (A untouched); and for EVERY case run,
             nvsm_debug_gemm_plan agrees with what the launcher did.
Each bound's observed / allowed ratio is printed (-s) as a MARGIN line: DESIGN.md §4.1 keeps the worst per kernel.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.helpers import rel_err
from tests.test_gemm_plans import (BIAS, BIAS_GRAD, BIG_CASES, BN, COLSTATS, GATHER, KERNEL_NAMES, M_OF, MODES, REFUSAL_EDGES, REFUSED_EPILOGUES, ROWS,
                                   ROWSQ, RSPLIT, SPLIT, TILED, TSTAT, TSTAT_TABLE, WINDOWS, big_m, case_id, edge_id, plan, table_cases)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ALPHA = -0.75
ROWSQ_SCALE = 1.0 / 3.0
TABLE_ROWS = 53          # rows of the gathered word table: far fewer than ids, so ids repeat (inside a window too)
BF16_KERNELS = (RSPLIT, SPLIT)


@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def t_rows(kernel, M, N, K):
    """Rows a kernel's column sums add in fp32 before they continue in fp64.
    rows / rsplit: the workgroup's 32-row tile, summed per column in fp32, handed to the ordered grid sum as doubles (epilogues of
        gemm_rows_kernel / gemm_rsplit_kernel: `for r < SM`, then grid_sum_ordered's fp64 lambda).
    tiled: a 128-row tile — a lane's 32 rows, the two half-waves, the two row-waves, all fp32 (gather_gemm.hip, red_plain).
    split: the plain sums stay fp32 across all passes of a workgroup (st_plain +=): its share of the 16-row blocks.
    tstat: a wave's slot merges block after block in fp32 (mean, M2): the blocks ONE wave multiplies for one column."""
    if kernel in (ROWS, RSPLIT):
        return 32
    if kernel == TILED:
        return 128
    nblocks = (M + 15) // 16
    if kernel == SPLIT:
        return 16 * math.ceil(nblocks / min(_cus(), nblocks))
    parts, NT = next((r[2], r[3]) for r in TSTAT_TABLE if (r[0], r[1]) == (N, K))
    tiles = (N + 15) // 16
    wide, wgs, t0, w0, blocks = tiles - parts * (NT - 1), max(_cus(), parts), 0, 0, 0
    for p in range(parts):          # launch_gemm_tstat: workgroups in proportion to the tiles of a part ...
        nt = NT if p < wide else NT - 1
        t0 += nt
        share = max(1, wgs - w0 if p + 1 == parts else wgs * t0 // tiles - w0)
        w0 += share
        # ... gemm_tstat_kernel: a workgroup's nb blocks go one whole block per wave and round; the nb % 8 left over are cut into
        # single tiles, block-major, an eighth of them per wave. A slot of a wave (one per column) sees the wave's whole blocks and
        # those of its single tiles that are this column's tile.
        for nb in {nblocks // share, -(-nblocks // share)}:
            full, units = nb // 8, (nb % 8) * nt
            for w in range(8):
                mine = range(units * w // 8, units * (w + 1) // 8)
                blocks = max(blocks, full + max([sum(1 for u in mine if u % nt == tt) for tt in range(nt)] + [0]))
    return 16 * blocks


@functools.lru_cache(maxsize=64)
def operands(M, N, K, offset=False):
    """The existing GEMM tests' operands: values over many binades, an asymmetric B. offset: a column of ones in A against a row of
    B that lifts every column of C to 50 of its standard deviations (the pivot branch of the tile sums)."""
    rs = np.random.RandomState(M + 3 * N + 7 * K)
    A = (rs.standard_normal((M, K)) * np.exp2(rs.randint(-12, 4, (M, K)))).astype(np.float32)
    Bm = (rs.standard_normal((K, N)) * 0.1 * np.exp2(rs.randint(-6, 3, (K, N))) + np.arange(N)[None, :] * 1e-3).astype(np.float32)
    if offset:
        A[:, 0] = 1.0
        Bm[0, :] = 0.0
        Bm[0, :] = (50.0 * (A.astype(np.float64) @ Bm.astype(np.float64)).std(axis=0)).astype(np.float32)
    A.setflags(write=False); Bm.setflags(write=False)
    return A, Bm


def is_fill(x):
    return bool(np.isnan(x).all())


MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def report_margins():
    """Behind the module's last test: the worst observed / allowed per kernel and bound (the table of DESIGN.md §4.1)."""
    yield
    for (kernel, name), r in sorted(MARGINS.items()):
        print("\nWORST %-7s %-18s %.3f" % (kernel, name, r), end="")
    print()


def margin(kernel, name, observed, allowed):
    r = float(observed) / float(allowed)
    key = (KERNEL_NAMES[kernel], name)
    MARGINS[key] = max(MARGINS.get(key, 0.0), r)
    print("MARGIN %-7s %-18s %.4f" % (key[0], name, r))
    return r


def launch(kernel, b_layout, M, N, K, flags, window=0, weighted=True, offset=False):
    """One launch with inputs made from the flags; returns inputs and outputs. Nothing here judges."""
    A, Bm = operands(M, N, K, offset)
    rs = np.random.RandomState(M + N + K + flags + window)
    Bh = np.ascontiguousarray(Bm.T) if b_layout else Bm
    a = ca._lib.GemmEpilogueArgs()
    r = dict(A=A, Bm=Bm, launched=C.c_int(-1), C=np.zeros((M, N), np.float32), A_out=np.zeros((M, K), np.float32))
    a.kernel, a.b_layout, a.M, a.N, a.K = kernel, b_layout, M, N, K
    a.A, a.B, a.C, a.A_out, a.alpha = A.ctypes.data, Bh.ctypes.data, r["C"].ctypes.data, r["A_out"].ctypes.data, ALPHA
    a.launched = C.pointer(r["launched"])
    if flags & BIAS:
        r["bias"] = (0.1 * rs.standard_normal(N)).astype(np.float32)
        a.bias = r["bias"].ctypes.data
    if flags & COLSTATS:
        r["stats"] = np.zeros((2, N), np.float64)
        a.colstats = r["stats"].ctypes.data
    if flags & ROWSQ:
        r["rowsq"] = np.zeros(M, np.float32)
        a.rowsq, a.rowsq_scale = r["rowsq"].ctypes.data, ROWSQ_SCALE
    if flags & (BN | BIAS_GRAD):
        r["sums"] = rs.standard_normal((2, K)) * M * np.exp2(rs.randint(-6, 2, (2, K)))
        r["n"] = float(3 * M + 1)
        for n in ("dbeta", "dgamma", "grad_bias"):
            r[n] = np.zeros(K, np.float32)
            setattr(a, n, r[n].ctypes.data)
        a.sums, a.n_global = r["sums"].ctypes.data, r["n"]
    if flags & BN:          # trained-model magnitudes: units off zero by a few standard deviations, deviations from 0.05 to 4
        sd = np.exp2(rs.uniform(-4.3, 2, K))
        r["mean"] = (3.0 * rs.standard_normal(K)).astype(np.float32)
        r["inv_std"] = (1.0 / sd).astype(np.float32)
        r["pre"] = (r["mean"] + sd * rs.standard_normal((M, K))).astype(np.float32)
        a.pre, a.mean, a.inv_std = r["pre"].ctypes.data, r["mean"].ctypes.data, r["inv_std"].ctypes.data
    if flags & GATHER:
        r["table"] = (rs.standard_normal((TABLE_ROWS, K)) * np.exp2(rs.randint(-8, 3, (TABLE_ROWS, K)))).astype(np.float32)
        r["idx"] = rs.randint(0, TABLE_ROWS, (M, window)).astype(np.int64)
        r["idx"][::5, -1] = r["idx"][::5, 0]          # (a repeat inside the window, whatever its length)
        r["wts"] = rs.uniform(0.1, 2.0, (M, window)).astype(np.float32) if weighted else None
        r["window"] = window
        a.table, a.table_rows, a.idx, a.window = r["table"].ctypes.data, TABLE_ROWS, r["idx"].ctypes.data, window
        a.wts = r["wts"].ctypes.data if weighted else None
    ca._lib.check(ca.lib().nvsm_debug_gemm_epilogue(C.byref(a)))
    r["launched"] = r["launched"].value
    assert r["launched"] in (0, 1)
    return r


def check_refused(r, flags):
    assert is_fill(r["C"])
    assert is_fill(r["A_out"]) if flags & GATHER else np.array_equal(r["A_out"], r["A"])
    for n in ("stats", "rowsq", "dbeta", "dgamma", "grad_bias"):
        assert n not in r or is_fill(r[n]), n


def check_launched(kernel, M, N, K, flags, r):
    """Every output of a launch that took place against its fp64 reference."""
    A64, B64, Cg = r["A"].astype(np.float64), r["Bm"].astype(np.float64), r["C"]
    assert np.isfinite(Cg).all()                                      # every element of C written
    # ---- what the product multiplied: A, dx, or the phrases ----
    if flags & BN:
        dx = r["A_out"]
        assert np.isfinite(dx).all()
        db, dg = r["sums"][0].astype(np.float32), r["sums"][1].astype(np.float32)
        for n, want in (("dbeta", db), ("dgamma", dg), ("grad_bias", db)):
            assert np.array_equal(r[n], want), n
        is64, xhat = r["inv_std"].astype(np.float64), (r["pre"].astype(np.float64) - r["mean"]) * r["inv_std"].astype(np.float64)
        t2, t3 = db.astype(np.float64) / r["n"], xhat * dg.astype(np.float64) / r["n"]
        ref = is64 * (A64 - t2 - t3)
        terms = np.abs(is64) * (np.abs(A64) + np.abs(t2) + np.abs(t3))
        err = np.abs(dx.astype(np.float64) - ref) / terms
        assert margin(kernel, "bn dx", err.max(), 8 * U) < 1.0
        A64 = dx.astype(np.float64)
    elif flags & GATHER:
        phrase = np.zeros((M, K), np.float32)
        ca._lib.check(ca.lib().nvsm_debug_gather_mean(TABLE_ROWS, K, r["table"].ctypes.data, r["idx"].ctypes.data,
                                                      r["wts"].ctypes.data if r["wts"] is not None else None, r["window"], M, phrase.ctypes.data))
        assert np.array_equal(r["A_out"].view(np.uint32), phrase.view(np.uint32))
        # (the gather hook itself, loosely, against fp64: a window of fp32 fmas and a division)
        w = r["wts"].astype(np.float64)[:, :, None] if r["wts"] is not None else 1.0
        rows = r["table"].astype(np.float64)[r["idx"]] * w
        assert (np.abs(phrase - rows.sum(axis=1) / r["window"]) <= (r["window"] + 2) * U * np.abs(rows).sum(axis=1) / r["window"]).all()
        A64 = phrase.astype(np.float64)
    else:
        assert np.array_equal(r["A_out"], r["A"])                    # (bias-gradient-only included: A comes back bit-identical)
    if flags & BIAS_GRAD:
        assert np.array_equal(r["grad_bias"], r["sums"][0].astype(np.float32))
        assert is_fill(r["dbeta"]) and is_fill(r["dgamma"])          # (not this mode's to write)
    # ---- C ----
    ref = ALPHA * (A64 @ B64) + (r["bias"].astype(np.float64) if "bias" in r else 0.0)
    if kernel in BF16_KERNELS:
        # (+ 2 u |ref| with a bias only: the two roundings behind the product, alpha · acc and + bias, which Σ|a||b| does not carry)
        allowed = 1.5e-6 * abs(ALPHA) * (np.abs(A64) @ np.abs(B64)) + (2 * U * np.abs(ref) if "bias" in r else 0.0)
        assert margin(kernel, "C max/sum|ab|", (np.abs(Cg - ref) / allowed).max(), 1.0) < 1.0
    else:
        assert margin(kernel, "C rel-L2", rel_err(Cg, ref), 2e-6) < 1.0
    C64 = Cg.astype(np.float64)
    # ---- column sums of the returned C ----
    if flags & COLSTATS:
        assert np.isfinite(r["stats"]).all()
        t = t_rows(kernel, M, N, K)
        e1 = np.abs(r["stats"][0] - C64.sum(axis=0)) / (t * U * np.abs(C64).sum(axis=0))
        e2 = np.abs(r["stats"][1] - (C64 * C64).sum(axis=0)) / (t * U * (C64 * C64).sum(axis=0))
        assert margin(kernel, "colsum", e1.max(), 1.0) < 1.0
        assert margin(kernel, "colsum of squares", e2.max(), 1.0) < 1.0
    # ---- row sums of squares of the returned C ----
    if flags & ROWSQ:
        assert np.isfinite(r["rowsq"]).all()
        want = ROWSQ_SCALE * (C64 * C64).sum(axis=1)
        assert margin(kernel, "rowsq", (np.abs(r["rowsq"] - want) / want).max(), (N + 2) * U) < 1.0


def run_case(kernel, N, K, mode, M, window=0, weighted=True, offset=False):
    b_layout, flags = MODES[mode]
    covers, _ = plan(kernel, b_layout, M, N, K, flags, window)
    r = launch(kernel, b_layout, M, N, K, flags, window, weighted, offset)
    assert bool(r["launched"]) == covers                              # the plan and the launcher agree
    assert r["launched"], "a row of the table must be covered"
    check_launched(kernel, M, N, K, flags, r)


def test_m_sizes_reach_the_full_block_paths():
    """big_m on this device: gemm_split's workgroups run two passes, gemm_tstat's waves a full-width block each and single tiles."""
    cus = _cus()
    for b_layout, rbp in ((0, 13), (1, 7)):
        nblocks = (big_m(SPLIT, b_layout, cus=cus) + 15) // 16
        assert rbp < nblocks // min(cus, nblocks) <= 2 * rbp
    for parts in (1, 2, 3):
        nblocks = (big_m(TSTAT, 0, parts, cus=cus) + 15) // 16
        nb = nblocks // -(-cus // parts)          # (a workgroup of the part owns nb or nb + 1: a whole block per wave and a remainder)
        assert nb >= 8 and nb % 8 and (nb + 1) % 8


@pytest.mark.parametrize("case", BIG_CASES, ids=lambda c: "%s-%dx%d-%s" % (KERNEL_NAMES[c[0]], c[1], c[2], c[3]))
def test_epilogue_many_blocks_per_workgroup(case):
    """The two large-batch kernels with enough rows that a workgroup owns many 16-row blocks (big_m, from this device's CU count):
    gemm_split's row-block loop over two uneven passes with the sums carried across them, gemm_tstat's full-width blocks — the
    narrow parts' <KG, NT - 1> form of a mixed split included — and the merge of a wave's column statistics over blocks. Same
    references and bounds; t (t_rows) follows the rows a workgroup / a wave now adds in fp32."""
    kernel, N, K, mode = case
    parts = next(r[2] for r in TSTAT_TABLE if (r[0], r[1]) == (N, K)) if kernel == TSTAT else 1
    run_case(kernel, N, K, mode, big_m(kernel, MODES[mode][0], parts, cus=_cus()))


CASES = [c for c in table_cases() if c[3] not in "WV"]
GATHER_CASES = [c for c in table_cases() if c[3] in "WV"]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_epilogue(case, monkeypatch):
    kernel, N, K, mode, _ = case
    ragged, full = M_OF[kernel]
    if kernel in BF16_KERNELS:
        run_case(kernel, N, K, mode, full)
        run_case(kernel, N, K, mode, ragged)
        monkeypatch.setenv("NVSM_GEMM_SPLIT", "9")
        run_case(kernel, N, K, mode, ragged)
    else:
        run_case(kernel, N, K, mode, full)
        run_case(kernel, N, K, mode, ragged)


@pytest.mark.parametrize("case", GATHER_CASES, ids=case_id)
def test_gather_epilogue(case, monkeypatch):
    kernel, N, K, mode, _ = case
    ragged, full = M_OF[kernel]
    for window in WINDOWS:
        for weighted in (True, False):
            run_case(kernel, N, K, mode, ragged, window, weighted)
    run_case(kernel, N, K, mode, full, 10, True)
    monkeypatch.setenv("NVSM_GEMM_SPLIT", "9")
    run_case(kernel, N, K, mode, ragged, 10, True)


OFFSET_CASES = [(ROWS, 36, 20), (ROWS, 256, 300), (RSPLIT, 36, 20), (RSPLIT, 256, 300), (RSPLIT, 320, 320), (SPLIT, 244, 20), (SPLIT, 256, 300),
                (TSTAT, 116, 292), (TSTAT, 256, 300), (TILED, 100, 148)]


@pytest.mark.parametrize("kernel,N,K", OFFSET_CASES, ids=["%s-%dx%d" % (KERNEL_NAMES[k], n, kk) for k, n, kk in OFFSET_CASES])
def test_colstats_of_columns_far_from_zero(kernel, N, K):
    """Every column of C lifted to 50 of its standard deviations: the tile sums take their pivot branch. Same bound."""
    run_case(kernel, N, K, "C", M_OF[kernel][0], offset=True)


@pytest.mark.parametrize("edge", REFUSAL_EDGES, ids=edge_id)
def test_refusal_edges(edge):
    _, kernel, b_layout, flags, window, inside, outside = edge
    M = M_OF[kernel][0]
    r = launch(kernel, b_layout, M, inside[0], inside[1], flags, window)
    assert r["launched"] and plan(kernel, b_layout, M, inside[0], inside[1], flags, window)[0]
    check_launched(kernel, M, inside[0], inside[1], flags, r)
    (N, K), w = (outside, window) if isinstance(outside, tuple) else (inside, outside)
    r = launch(kernel, b_layout, M, N, K, flags, w)
    assert not r["launched"] and not plan(kernel, b_layout, M, N, K, flags, w)[0]
    check_refused(r, flags)


@pytest.mark.parametrize("probe", REFUSED_EPILOGUES, ids=lambda p: "%s-%d-%d" % (KERNEL_NAMES[p[0]], p[1], p[2]))
def test_refused_epilogues_touch_nothing(probe):
    kernel, b_layout, flags, N, K = probe
    M, window = M_OF[kernel][0], 10 if flags & GATHER else 0
    r = launch(kernel, b_layout, M, N, K, flags, window)
    assert not r["launched"] and not plan(kernel, b_layout, M, N, K, flags, window)[0]
    check_refused(r, flags)


def test_below_the_large_batch_minimum_is_refused():
    for kernel, b_layout, flags, N, K in ((SPLIT, 1, ROWSQ, 300, 256), (TSTAT, 1, ROWSQ, 256, 256)):
        r = launch(kernel, b_layout, 1023, N, K, flags)
        assert not r["launched"] and not plan(kernel, b_layout, 1023, N, K, flags)[0]
        check_refused(r, flags)
