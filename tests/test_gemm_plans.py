"""The shape table of the product-kernel epilogue tests (tests/test_gpu_gemm_epilogues.py), and — without a GPU — the proof that
it reaches what it is meant to reach: every instantiation in the launch switches of the four batch-sized projection kernels, and
each refusal edge from both sides. Everything here goes through nvsm_debug_gemm_plan, which is host arithmetic only and asks the
very functions the launchers decide by (rs_plan, rows_plan, gemm_split_plan, gemm_tstat_plan).

Why these shapes. A row of the table is (N, K) for one kernel with the plan that kernel must choose for it and the epilogue modes
it admits; a moved planner threshold therefore fails HERE instead of quietly sending the GPU test down another path. The rows are
chosen so that
  * every (waves, rch) pair of gemm_rsplit's switch occurs (4 / 8 / 10 waves by N <= 128 / 256 / 320; rch 4 / 5 / 8 by how many
    float4s of the 32 x K panel a thread stages), with an odd number of 16-deep k steps (one zero step of padding: K = 16, 36,
    100, 200, 300, 336, 400) and an even one, and with a full last 32-column tile and a ragged one (N = 36, 100, 132, 200, 260, 300);
  * every (waves, tiles-per-wave) pair gemm_rows can choose occurs, down to N = K = 4;
  * gemm_split sees its one forward width (16 column blocks, also with padding columns: N = 244, 252) and the ends and the
    middle of its backward range (17, 19, 20, 24 blocks: every wave with three blocks, and the 3 / 2 mix), K below one 32-deep
    tile, K not a multiple of 32, and K = 320, the largest with the fused batch-norm backward;
  * gemm_tstat sees its four compiled (KG, NT, layout, mixed) forms in one, two and three column parts, with a ragged last
    16-column tile (N = 116, 244, 292, 452);
  * the dimensions users pick that no other test runs: d_w = 200 with d_e = 100 (both products), N = 100, 36;
and they include N in {32, 36, 64, 100, 128, 132, 256, 260, 300, 320} and K in {16, 20, 36, 128, 148, 256, 300, 320}, plus
K = 336 with 8 waves for gemm_rsplit.

Epilogue modes (letters in the table; b_layout 0 = B is [K][N], the forward product; 1 = B stored [N][K], the backward one):
  P  plain product, alpha != 1, with a bias          (b_layout 0)
  N  plain product, alpha != 1, no bias              (b_layout 0)
  L  plain product, alpha != 1, no bias              (b_layout 1)
  C  ordered batch-norm column sums                  (b_layout 0)
  R  row sums of squares                             (b_layout 1)
  B  fused batch-norm backward + row sums of squares (b_layout 1)
  G  bias gradient only                              (b_layout 1)
  W  fused word gather-mean, with and without C      (b_layout 0, gemm_rsplit only)
"""
import ctypes as C

import pytest

import cunvsm_amd as ca

ROWS, RSPLIT, SPLIT, TSTAT, TILED = 0, 1, 2, 3, 4
KERNEL_NAMES = {ROWS: "rows", RSPLIT: "rsplit", SPLIT: "split", TSTAT: "tstat", TILED: "tiled"}
COLSTATS, ROWSQ, BN, BIAS, GATHER, BIAS_GRAD = 1, 2, 4, 8, 16, 32
# mode letter -> (b_layout, flags)
MODES = {"P": (0, BIAS), "N": (0, 0), "L": (1, 0), "C": (0, COLSTATS), "R": (1, ROWSQ), "B": (1, BN | ROWSQ), "G": (1, BIAS_GRAD),
         "W": (0, GATHER), "V": (0, GATHER | COLSTATS)}      # (V: what W expands to besides itself)
WINDOWS = (1, 2, 10, 32)
# the smallest M a launcher takes + 7 (a ragged last row panel), and two full panels (32-row panels; 1 024-row minimum)
M_OF = {ROWS: (519, 64), RSPLIT: (519, 64), TILED: (519, 256), SPLIT: (1031, 2048), TSTAT: (1031, 2048)}


def big_m(kernel, b_layout, parts=1, cus=256):
    """At the Ms above a workgroup of the two large-batch kernels owns ONE 16-row block at most (they spread ceil(M / 16) blocks over
    all `cus` compute units): gemm_split's row-block loop, its second pass and the sums across passes, and gemm_tstat's full-width
    blocks (tstat_block<KG, NT> and, in the narrow parts of a mixed split, <KG, NT - 1>) with the merge of a wave's statistics over
    blocks never run there. This M does: 16-row blocks enough that
      gemm_split  every workgroup owns RBP + 2 or RBP + 3 blocks (RBP = 13 forward, 7 backward: two passes, uneven),
      gemm_tstat  every workgroup of a column part owns about ten (a full-width block per wave, then single tiles of the rest),
    plus three blocks and seven rows, so that the shares differ and the last block is ragged."""
    if kernel == SPLIT:
        return 16 * (cus * ((7 if b_layout else 13) + 2) + 3) + 7
    assert kernel == TSTAT
    return 16 * (-(-cus // parts) * 10 + 3) + 7


# (kernel, N, K, mode): the cases run at big_m as well — every compiled form of the two kernels with a statistics, row-sum or
# batch-norm epilogue, with and without padding columns
BIG_CASES = [(SPLIT, 256, 300, "C"), (SPLIT, 244, 20, "C"), (SPLIT, 300, 256, "R"), (SPLIT, 300, 256, "B"), (SPLIT, 384, 128, "B"),
             (SPLIT, 260, 256, "R"),
             (TSTAT, 256, 300, "C"), (TSTAT, 116, 292, "C"), (TSTAT, 244, 116, "C"), (TSTAT, 256, 256, "R"), (TSTAT, 292, 244, "R"),
             (TSTAT, 452, 256, "R")]

# gemm_rsplit: (N, K, waves, rch, odd k steps, columns of the last 32-column tile, modes)
RSPLIT_TABLE = [
    (32, 16, 4, 4, 1, 32, "PCRBGW"), (36, 20, 4, 4, 0, 4, "PCRBGW"), (64, 36, 4, 4, 1, 32, "PCRBGW"), (128, 128, 4, 4, 0, 32, "PCRBGW"),
    (100, 148, 4, 5, 0, 4, "PCRGW"), (100, 200, 4, 8, 1, 4, "PCRG"), (128, 256, 4, 8, 0, 32, "PCRG"),
    (132, 128, 8, 4, 0, 4, "PCRBGW"), (200, 100, 8, 4, 1, 8, "PCRBGW"), (256, 300, 8, 5, 1, 32, "PCRGW"), (256, 320, 8, 5, 0, 32, "PCRGW"),
    (256, 336, 8, 8, 1, 32, "PCRG"),
    (260, 256, 10, 4, 0, 4, "PCRBG"), (300, 256, 10, 4, 0, 12, "PCRBG"), (320, 320, 10, 4, 0, 32, "PCRBG"),
    (300, 336, 10, 5, 1, 12, "PCRG"), (320, 400, 10, 8, 1, 32, "PCRG"),
]
# gemm_rows: (N, K, waves, tiles per wave, modes). B as [K][N] stops at N = 256 (no caller beyond).
ROWS_TABLE = [
    (4, 4, 4, 1, "PCRBG"), (32, 16, 4, 1, "PCRBG"), (36, 20, 4, 1, "PCRBG"), (64, 36, 4, 1, "PCRBG"), (100, 148, 4, 1, "PCRBG"),
    (128, 256, 4, 1, "PCRBG"), (132, 128, 8, 1, "PCRBG"), (200, 100, 8, 1, "PCRBG"), (256, 300, 8, 1, "PCRBG"),
    (260, 256, 10, 1, "LRBG"), (300, 256, 10, 1, "LRBG"), (320, 320, 10, 1, "LRBG"),
]
# gemm_split: (N, K, 16-column blocks, modes)
SPLIT_TABLE = [
    (256, 16, 16, "PNC"), (244, 20, 16, "PNC"), (252, 148, 16, "PNC"), (256, 128, 16, "PNC"), (256, 300, 16, "PNC"),
    (260, 256, 17, "LRBG"), (300, 36, 19, "LRBG"), (300, 256, 19, "LRBG"), (320, 320, 20, "LRBG"), (384, 128, 24, "LRBG"),
]
# gemm_tstat: (N, K, parts, NT, mixed, KG, modes)
TSTAT_TABLE = [
    (256, 300, 2, 8, 0, 19, "PNC"), (128, 300, 1, 8, 0, 19, "PNC"), (116, 292, 1, 8, 0, 19, "PNC"), (384, 300, 3, 8, 0, 19, "PNC"),
    (256, 128, 2, 8, 0, 8, "PNC"), (244, 116, 2, 8, 0, 8, "PNC"),
    (256, 256, 2, 8, 0, 16, "LR"), (128, 244, 1, 8, 0, 16, "LR"),
    (300, 256, 2, 10, 1, 16, "LR"), (292, 244, 2, 10, 1, 16, "LR"), (452, 256, 3, 10, 1, 16, "LR"),
]
# the tiled kernel (128 x 128 tiles, through launch_gemm with the others off): no plan word
TILED_TABLE = [(36, 20, "PCR"), (100, 148, "PCR"), (132, 128, "PCR"), (256, 300, "PCR"), (300, 256, "PCR")]


def plan(kernel, b_layout, M, N, K, flags, window=0):
    """(covers, plan word) of nvsm_debug_gemm_plan."""
    covers, word = C.c_int(-1), C.c_uint(0)
    ca._lib.check(ca.lib().nvsm_debug_gemm_plan(kernel, b_layout, M, N, K, flags, window, C.byref(covers), C.byref(word)))
    assert covers.value in (0, 1)
    return bool(covers.value), word.value


def table_cases():
    """Every (kernel, N, K, mode letter, expected plan word) of the table; W also yields V (the gather with column sums)."""
    out = []
    for N, K, waves, rch, odd, tailw, modes in RSPLIT_TABLE:
        for m in modes.replace("W", "WV"):
            out.append((RSPLIT, N, K, m, waves | rch << 8 | odd << 16 | tailw << 24))
    for N, K, waves, tpw, modes in ROWS_TABLE:
        for m in modes:
            out.append((ROWS, N, K, m, waves | tpw << 8))
    for N, K, cbs, modes in SPLIT_TABLE:
        for m in modes:
            out.append((SPLIT, N, K, m, cbs | cbs // 8 << 8 | -(-cbs // 8) << 16))
    for N, K, parts, NT, mixed, KG, modes in TSTAT_TABLE:
        for m in modes:
            out.append((TSTAT, N, K, m, parts | NT << 8 | mixed << 16 | KG << 24))
    for N, K, modes in TILED_TABLE:
        for m in modes:
            out.append((TILED, N, K, m, 0))
    return out


def case_id(case):
    kernel, N, K, mode, _ = case
    return "%s-%dx%d-%s" % (KERNEL_NAMES[kernel], N, K, mode)


@pytest.mark.parametrize("case", table_cases(), ids=case_id)
def test_table_rows_take_the_plan_they_name(case):
    kernel, N, K, mode, word = case
    b_layout, flags = MODES[mode]
    Ms = M_OF[kernel]
    if (kernel, N, K, mode) in BIG_CASES:
        Ms += (big_m(kernel, b_layout, word & 255),)          # (tstat's word begins with its parts)
    for M in Ms:
        for window in (WINDOWS if flags & GATHER else (0,)):
            assert plan(kernel, b_layout, M, N, K, flags, window) == (True, word), (M, window)


def test_table_holds_the_dimensions_it_must():
    for kernel, table in ((RSPLIT, RSPLIT_TABLE), (ROWS, ROWS_TABLE)):
        assert {32, 36, 64, 100, 128, 132, 256, 260, 300, 320} <= {r[0] for r in table}, KERNEL_NAMES[kernel]
        assert {16, 20, 36, 128, 148, 256, 300, 320} <= {r[1] for r in table}, KERNEL_NAMES[kernel]
    # the two large-batch kernels take a narrow range of N each: between them, every N of the list they can take at all
    assert {256, 260, 300, 320} <= {r[0] for r in SPLIT_TABLE} and {128, 256, 300} <= {r[0] for r in TSTAT_TABLE}
    assert {16, 20, 36, 128, 148, 256, 300, 320} <= {r[1] for r in SPLIT_TABLE}
    assert {128, 256, 300} <= {r[1] for r in TSTAT_TABLE}          # (gemm_tstat is compiled for K in 116-128, 244-256, 292-304 only)
    assert any(waves == 8 and 320 < K <= 512 for _, K, waves, *_ in RSPLIT_TABLE)


# ---------------------------------------------------------------------------------------------------------------------------------
# instantiations: read off the switch / if ladders of the launchers, listed here; the table must reach each of them
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rsplit_table_reaches_every_instantiation():
    """launch_gemm_rsplit: NVSM_RS_CASE (W, R) for W in 4, 8, 10 and R in 4, 5, 8 — gemm_rsplit_kernel<PRE = false, W, R> — and, with
    the fused batch-norm backward, <PRE = true, W, 4> only; NVSM_RSG_CASE (W, R) for W in 4, 8 and R in 4, 5 — <false, W, R, GATH = 1>
    (GATH = 2, the lazily decayed table, is the same switch entry: with the model-level lazy tests). NPROD 6 / 9 is the
    environment's, not the shape's: the GPU test runs both."""
    want = {(False, w, r, 0) for w in (4, 8, 10) for r in (4, 5, 8)} | {(True, w, 4, 0) for w in (4, 8, 10)}
    want |= {(False, w, r, 1) for w in (4, 8) for r in (4, 5)}
    got = set()
    for N, K, waves, rch, _, _, modes in RSPLIT_TABLE:
        for m in modes:
            got.add((m == "B", waves, rch, 1 if m == "W" else 0))
    assert want <= got, sorted(want - got)
    # both paddings and both kinds of last tile under every epilogue
    for m in "PCRBGW":
        rows = [r for r in RSPLIT_TABLE if m in r[6]]
        assert {r[4] for r in rows} == {0, 1} and any(r[5] == 32 for r in rows) and any(r[5] < 32 for r in rows), m


def test_rows_table_reaches_every_instantiation():
    """launch_gemm_rows: NVSM_ROWS_CASE (tpw, waves) = (1, 4), (2, 4), (2, 5), (1, 8), (1, 10); b_layout 0 is compiled for 4 and 8
    waves only, b_layout 1 with PRE false and true. rows_plan picks two tiles per wave only where the experiments build's
    NVSM_ROWS_TPW=2 asks for them (an A/B switch of tools/exp/, read by no other build), so no shape reaches (2, 4) and (2, 5) in
    the product: they stay for that switch, and the plan says so."""
    want = {(0, False, 1, 4), (0, False, 1, 8)} | {(1, pre, 1, w) for pre in (False, True) for w in (4, 8, 10)}
    got = set()
    for N, K, waves, tpw, modes in ROWS_TABLE:
        for m in modes:
            got.add((MODES[m][0], m == "B", tpw, waves))
    assert want <= got, sorted(want - got)
    for N in range(4, 324, 4):          # no accepted shape takes the two-tile form
        for K in (4, 128, 320):
            for b_layout, flags in ((0, 0), (1, ROWSQ), (1, BN)):
                covers, word = plan(ROWS, b_layout, 519, N, K, flags)
                assert not covers or word >> 8 == 1, (N, K, b_layout)


def test_split_table_reaches_every_instantiation():
    """launch_gemm_split: forward <CBW 2, RBP 13> with epilogue statistics / bias / none; backward <CBW 3, RBP 7, MIXED> — a wave with
    three column blocks runs split_body<3>, one with two split_body<2> — with row sums of squares or none, each with PRE (the fused
    batch-norm backward) and without."""
    want = {(0, "C", 2), (0, "P", 2), (0, "N", 2)} | {(1, m, body) for m in "RLB" for body in (2, 3)}
    got = set()
    for N, K, cbs, modes in SPLIT_TABLE:
        for m in modes:
            b_layout, flags = MODES[m]
            covers, word = plan(SPLIT, b_layout, 1031, N, K, flags)
            assert covers
            got |= {(b_layout, m, word >> 8 & 255), (b_layout, m, word >> 16 & 255)}      # the fewest and the most blocks of a wave
    assert want <= got, sorted(want - got)
    assert {r[2] for r in SPLIT_TABLE} >= {16, 17, 24}
    # the cases run with many row blocks per workgroup cover both bodies of the backward kernel too
    big = set()
    for kernel, N, K, m in BIG_CASES:
        if kernel == SPLIT:
            word = plan(SPLIT, MODES[m][0], big_m(SPLIT, MODES[m][0]), N, K, MODES[m][1])[1]
            big |= {(MODES[m][0], word >> 8 & 255), (MODES[m][0], word >> 16 & 255)}
    assert big == {(0, 2), (1, 2), (1, 3)}


def test_tstat_table_reaches_every_instantiation():
    """launch_gemm_tstat: <KG 19, NT 8, layout 0>, <8, 8, 0>, <16, 8, 1>, all unmixed, and <16, 10, 1, MIXED>; tstat_launch: layout 0
    with statistics / bias / none, layout 1 with row sums of squares / none."""
    want = {(19, 8, 0, 0, m) for m in "PNC"} | {(8, 8, 0, 0, m) for m in "PNC"} | {(16, 8, 1, 0, m) for m in "LR"} | {(16, 10, 1, 1, m) for m in "LR"}
    got = {(KG, NT, MODES[m][0], mixed, m) for N, K, parts, NT, mixed, KG, modes in TSTAT_TABLE for m in modes}
    assert want <= got, sorted(want - got)
    assert {r[2] for r in TSTAT_TABLE} == {1, 2, 3}                      # column parts
    assert any(r[4] and r[2] == 3 for r in TSTAT_TABLE)                  # the mixed split with more than one wide part
    # ... and each compiled form again with full-width blocks (BIG_CASES), the mixed one with row sums of squares
    big = {(r[5], r[3], MODES[m][0], r[4], m) for k, N, K, m in BIG_CASES if k == TSTAT for r in TSTAT_TABLE if (r[0], r[1]) == (N, K)}
    assert {b[:4] for b in big} == {(19, 8, 0, 0), (8, 8, 0, 0), (16, 8, 1, 0), (16, 10, 1, 1)} and (16, 10, 1, 1, "R") in big


# ---------------------------------------------------------------------------------------------------------------------------------
# refusal edges: one shape inside, one outside. The GPU test launches both of each pair.
# ---------------------------------------------------------------------------------------------------------------------------------
# (name, kernel, b_layout, flags, window, (N, K) inside, (N, K) or window outside)
REFUSAL_EDGES = [
    ("rsplit fused BN needs rch <= 4", RSPLIT, 1, BN | ROWSQ, 0, (128, 128), (128, 132)),
    ("rsplit gather needs rch <= 5", RSPLIT, 0, GATHER, 10, (128, 160), (128, 164)),
    ("rsplit gather needs <= 8 waves", RSPLIT, 0, GATHER, 10, (256, 128), (260, 128)),
    ("rsplit gather needs window <= 32", RSPLIT, 0, GATHER, 32, (128, 128), 33),
    ("rsplit stages at most eight float4s per thread", RSPLIT, 0, 0, 0, (128, 256), (128, 260)),
    ("rows: B as [K][N] stops at 256 columns", ROWS, 0, COLSTATS, 0, (256, 128), (260, 128)),
    ("split fused BN needs K <= 320", SPLIT, 1, BN | ROWSQ, 0, (300, 320), (300, 324)),
    ("split bias gradient needs K <= 320", SPLIT, 1, BIAS_GRAD, 0, (300, 320), (300, 324)),
    ("split forward is 16 column blocks", SPLIT, 0, COLSTATS, 0, (244, 128), (240, 128)),
    ("split backward is 17 to 24 column blocks", SPLIT, 1, ROWSQ, 0, (384, 128), (388, 128)),
    ("tstat unmixed parts of 8 tiles", TSTAT, 1, ROWSQ, 0, (256, 256), (260, 256)),
]
# epilogues a kernel has no code for: refused whatever the shape (the shape is one the kernel takes otherwise)
REFUSED_EPILOGUES = [
    (RSPLIT, 0, COLSTATS | ROWSQ, 128, 128), (RSPLIT, 0, ROWSQ, 128, 128), (RSPLIT, 0, BN, 128, 128), (RSPLIT, 1, BN | COLSTATS, 128, 128),
    (RSPLIT, 1, GATHER, 128, 128),
    (ROWS, 0, ROWSQ, 128, 128), (ROWS, 0, BN, 128, 128), (ROWS, 1, BN | COLSTATS, 128, 128), (ROWS, 0, GATHER, 128, 128),
    (SPLIT, 0, ROWSQ, 256, 128), (SPLIT, 0, COLSTATS | BIAS, 256, 128), (SPLIT, 0, BN, 256, 128), (SPLIT, 1, BIAS, 300, 256), (SPLIT, 1, COLSTATS, 300, 256),
    (TSTAT, 0, ROWSQ, 256, 128), (TSTAT, 0, COLSTATS | BIAS, 256, 128), (TSTAT, 1, BIAS, 256, 256), (TSTAT, 1, COLSTATS, 256, 256),
    (TSTAT, 1, BN | ROWSQ, 256, 256), (TSTAT, 1, BIAS_GRAD, 256, 256),
]


def edge_id(edge):
    return edge[0].replace(" ", "_")


@pytest.mark.parametrize("edge", REFUSAL_EDGES, ids=edge_id)
def test_refusal_edges_sit_where_the_table_says(edge):
    _, kernel, b_layout, flags, window, inside, outside = edge
    M = M_OF[kernel][0]
    assert plan(kernel, b_layout, M, inside[0], inside[1], flags, window)[0]
    if isinstance(outside, tuple):
        assert not plan(kernel, b_layout, M, outside[0], outside[1], flags, window)[0]
    else:
        assert not plan(kernel, b_layout, M, inside[0], inside[1], flags, outside)[0]


def test_refused_epilogues_and_sizes():
    for kernel, b_layout, flags, N, K in REFUSED_EPILOGUES:
        assert not plan(kernel, b_layout, M_OF[kernel][0], N, K, flags, 10 if flags & GATHER else 0)[0], (KERNEL_NAMES[kernel], b_layout, flags)
    # the two large-batch kernels start at 1 024 rows; N and K are multiples of 4 everywhere
    assert not plan(SPLIT, 1, 1023, 300, 256, ROWSQ)[0] and plan(SPLIT, 1, 1024, 300, 256, ROWSQ)[0]
    assert not plan(TSTAT, 1, 1023, 256, 256, ROWSQ)[0] and plan(TSTAT, 1, 1024, 256, 256, ROWSQ)[0]
    for kernel, M, b_layout, N, K in ((ROWS, 519, 1, 128, 128), (RSPLIT, 519, 1, 128, 128), (SPLIT, 1031, 1, 300, 256), (TSTAT, 1031, 1, 256, 256)):
        assert plan(kernel, b_layout, M, N, K, 0)[0]
        assert not plan(kernel, b_layout, M, N + 2, K, 0)[0] and not plan(kernel, b_layout, M, N, K + 2, 0)[0]
    assert not plan(RSPLIT, 0, 519, 28, 128, 0)[0] and not plan(RSPLIT, 0, 519, 128, 12, 0)[0]      # N >= 32, K >= 16
    assert not plan(RSPLIT, 0, 519, 324, 128, 0)[0] and not plan(ROWS, 1, 519, 324, 128, 0)[0]      # N <= 320


def test_plan_needs_no_gpu_and_follows_the_switches(monkeypatch):
    """The plan reads the same switches as the launchers: without the split-bf16 kernels (NVSM_GEMM_SPLIT=0) neither of them covers."""
    assert plan(RSPLIT, 0, 519, 256, 300, COLSTATS)[0] and plan(SPLIT, 0, 1031, 256, 300, COLSTATS)[0]
    monkeypatch.setenv("NVSM_GEMM_SPLIT", "0")
    assert not plan(RSPLIT, 0, 519, 256, 300, COLSTATS)[0] and not plan(SPLIT, 0, 1031, 256, 300, COLSTATS)[0]
    assert plan(ROWS, 0, 519, 256, 300, COLSTATS)[0] and plan(TSTAT, 0, 1031, 256, 300, COLSTATS)[0]
