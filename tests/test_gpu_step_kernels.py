"""-m gpu: the streaming kernels that run between the products, the loss and the table passes of a training step, ONE launcher at a
time through the hooks of include/cunvsm_amd_test_hooks.h, element by element against tests/step_kernels_reference.py.

Whole steps hold these kernels to the oracle by norm only (2e-4 of an update's norm at batch 512): one wrong row, the re-read of the
wrong word in a short last round of a window or a wrong low bf16 piece of T passes there. Here:

  adam_u, adagrad_scale  every rows-in-flight count of the dispatch (windows 1 - 10), windows beyond it with a short and a whole last
                         round of eight, both vector widths, a window of all-zero second moments, a grid past the 4096-workgroup cap
  gather_mean            against float64 at the windows whose last round is short (the lazy test compares it with itself)
  bn_dx, colsum_finalize both vector widths, one row, the data-parallel row count, the float casts of the sums
  row ops                row mean of squares, the L2 normaliser forward and backward (in place: the bits of out of place), the two
                         materialise kernels; dims below, at and above a wave's 64 lanes, a partly filled workgroup, a second trip
  slab sums              launch_splitk_reduce (float4 and scalar kernel) and launch_sum_parts: the BITS of the float32 emulation
  transform_update       every element of T, b, the gradients and the state for SGD / Adagrad / Adam, the in-kernel slab sum against
                         launch_splitk_reduce's, and the bf16 planes it writes against freshly cut ones, byte for byte

Tolerances (nothing of this file's own): bit equality where the order of additions is documented. Element-wise formulas - adam_u and
adagrad_scale among them: a window sum inside a quotient - within K_F32 = 4 times what a plain float32 evaluation of the same formula
loses against float64 over the tensor, plus 1e-6 of the tensor's largest magnitude. Plain sums over a window or a row within
t · 2^-24 · Σ|term| of float64, t = the float32 additions on the longest chain plus 2, stated at each use. No case is exempted: inputs
that would need it (a zero norm, a negative second moment) are not generated, and the precondition is asserted.

Every output is checked to be written where the kernel owns it and still 0xFF bytes behind. test_every_path_was_launched closes
the file. What three deliberately broken builds (never committed) do to it is recorded in profiles/NOTES_step_kernels.md."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import (ROW_L2_BACKWARD, ROW_L2_FORWARD, ROW_MATERIALIZE, ROW_MATERIALIZE_L2, ROW_MEANSQ, BnDxArgs, RowOpArgs,
                             TransformUpdateArgs)
from tests import step_kernels_reference as sk

pytestmark = pytest.mark.gpu

U32 = sk.U32
SEEN = set()                    # the paths the cases of this session launched
WORST = {}                      # quantity -> worst |g - ref64| / bound over the file
GRID_CAP_ITEMS = 4096 * 256     # stream_grid: work items of element kernels beyond which the grid-stride loop takes a second trip


def _ptr(a):
    return a.ctypes.data if a is not None else None


def is_ff(a):
    return np.all(np.ascontiguousarray(a).view(np.uint8) == 0xFF)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def hold(name, got, ref64, bound, label):
    """|got - ref64| <= bound (a scalar or an array), element by element; the worst share goes into WORST and is printed first."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    assert np.all(np.isfinite(np.asarray(got))), "%s: %s has non-finite elements" % (label, name)
    share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(share.max())
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print("step-kernels %s %s: %.3f of the allowance" % (label, name, worst))
    assert worst <= 1.0, (label, name, worst, int(np.argmax(share)))


def hold_elementwise(name, got, ref64, ref32, label):
    hold(name, got, ref64, sk.elementwise_tol(ref64, ref32), label)


# ---- window passes -----------------------------------------------------------------------------------------------------------------
TABLE_ROWS, ZERO_ROWS = 61, 3        # rows 0 .. 2 carry a second moment / accumulator of exactly 0
WINDOW_B = 37


def unroll_of(window):
    """window_unroll written down by hand: the whole window in flight up to ten words, eight at a time beyond."""
    return window if window <= 10 else 8


def window_ids(rs, B, window):
    idx = rs.randint(0, TABLE_ROWS, (B, window)).astype(np.int32)
    idx[0] = rs.randint(0, ZERO_ROWS, window)            # a whole window of zero rows: the denominator is eps
    if window >= 2 and B >= 2:
        idx[1, window - 1] = idx[1, 0]                   # a repeat inside a window
        idx[B - 1, 0] = idx[B - 1, window - 1]
    return idx


def run_adam_u(m, v, idx, bc, eps):
    B, window = idx.shape
    rows, dim = m.shape
    out = np.zeros((B + 1, dim), np.float32)
    ca._lib.check(ca.lib().nvsm_debug_adam_u(rows, dim, _ptr(m), _ptr(v), _ptr(idx), window, B, bc, eps, _ptr(out)))
    return out


def check_adam_u(window, dim, B, seed):
    rs = np.random.RandomState(seed)
    m = rs.standard_normal((TABLE_ROWS, dim)).astype(np.float32)
    v = rs.uniform(0.01, 2.0, TABLE_ROWS).astype(np.float32)
    v[:ZERO_ROWS] = 0.0
    m[:ZERO_ROWS] *= np.float32(1e-6)                    # (so that the quotient by eps = 1e-6 is of the size of the others)
    assert np.all(v >= 0)
    idx = window_ids(rs, B, window)
    assert np.all(v[idx[0]] == 0) and (window < 2 or idx[1, 0] == idx[1, -1])
    bc, eps = float(sk.adam_bc(5, np.float32)), float(sk.OPT_EPS)
    out = run_adam_u(m, v, idx, bc, eps)
    label = "adam_u window=%d dim=%d B=%d" % (window, dim, B)
    assert is_ff(out[B]), label + ": the guard row was written"
    hold_elementwise("adam_u", out[:B], sk.adam_u(m, v, idx, bc, eps), sk.adam_u(m, v, idx, bc, eps, np.float32), label)
    SEEN.add(("adam_u", 4 if dim % 4 == 0 else 1, unroll_of(window)))
    if B * (dim // 4 if dim % 4 == 0 else dim) > GRID_CAP_ITEMS:
        SEEN.add(("adam_u", "second trip"))


@pytest.mark.parametrize("dim", [3, 7, 12, 300])
@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 16, 17, 24, 33])
def test_adam_u(window, dim):
    """Windows 1 - 10: adam_u_kernel<V, window>, no tail. Beyond: <V, 8> with a last round of 3, 5, 8, 1, 8 and 1 words (11, 13, 16,
    17, 24, 33) - the clamped re-read whose words must not be added. Dims 3 and 7: V = 1; 12 and 300: V = 4."""
    check_adam_u(window, dim, WINDOW_B, 100 * window + dim)


def test_adam_u_past_the_grid_cap():
    """B · nvec = 1 048 581 work items at dim 4 (nvec 1): 4096 workgroups, the last five items on the loop's second trip."""
    check_adam_u(3, 4, GRID_CAP_ITEMS + 5, 77)


def run_adagrad_scale(acc, idx, eps):
    B, window = idx.shape
    out = np.zeros(B + 1, np.float32)
    ca._lib.check(ca.lib().nvsm_debug_adagrad_scale(acc.size, _ptr(acc), _ptr(idx), window, B, eps, _ptr(out)))
    return out


def check_adagrad_scale(window, B, seed):
    rs = np.random.RandomState(seed)
    acc = rs.uniform(1e-6, 4e-6, TABLE_ROWS).astype(np.float32)      # (of eps's size: 1 / sqrt(eps) does not dwarf the other scales)
    acc[:ZERO_ROWS] = 0.0
    assert np.all(acc >= 0)
    idx = window_ids(rs, B, window)
    eps = float(sk.OPT_EPS)
    out = run_adagrad_scale(acc, idx, eps)
    label = "adagrad_scale window=%d B=%d" % (window, B)
    assert is_ff(out[B:]), label + ": the guard was written"
    hold_elementwise("adagrad_scale", out[:B], sk.adagrad_scale(acc, idx, eps), sk.adagrad_scale(acc, idx, eps, np.float32), label)
    SEEN.add(("adagrad_scale", "tail" if window % 4 else "whole"))
    if B > GRID_CAP_ITEMS:
        SEEN.add(("adagrad_scale", "second trip"))


@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 16])
def test_adagrad_scale(window):
    """Four accumulators in flight: every window but 4, 8 and 16 ends in a short round."""
    check_adagrad_scale(window, WINDOW_B, 300 + window)


def test_adagrad_scale_past_the_grid_cap():
    check_adagrad_scale(3, GRID_CAP_ITEMS + 5, 78)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dim", [7, 300])
@pytest.mark.parametrize("window", [4, 5, 6, 7, 8, 9, 11, 13, 16])
def test_gather_mean_against_float64(window, dim, weighted):
    """launch_gather_mean keeps U = ceil(window / ceil(window / 5)) rows in flight: 4, 5, 3, 4, 4, 5, 4, 5, 4 for these windows, the
    last round short at 7, 9, 11 and 13. t = window + 2: one fused multiply-add per word and the division by the window."""
    rs = np.random.RandomState(1000 + 10 * window + dim + weighted)
    B = WINDOW_B
    table = rs.standard_normal((TABLE_ROWS, dim)).astype(np.float32)
    idx = window_ids(rs, B, window).astype(np.int64)
    wts = rs.uniform(0.25, 2.0, (B, window)).astype(np.float32) if weighted else None
    out = np.full((B, dim), np.nan, np.float32)
    ca._lib.check(ca.lib().nvsm_debug_gather_mean(TABLE_ROWS, dim, _ptr(table), _ptr(idx), _ptr(wts), window, B, _ptr(out)))
    ref, mag = sk.gather_mean(table, idx, wts)
    hold("gather_mean", out, ref, (window + 2) * U32 * mag, "gather_mean window=%d dim=%d %s" % (window, dim, "weighted" if weighted else "plain"))
    rounds = (window + 4) // 5
    SEEN.add(("gather_mean", 4 if dim % 4 == 0 else 1, (window + rounds - 1) // rounds, "tail" if window % ((window + rounds - 1) // rounds) else "whole"))


# ---- batch-norm backward -------------------------------------------------------------------------------------------------------------
def run_bn_dx(dy, pre, mean, inv_std, sums, n_global, dim):
    rows = 0 if dy is None else dy.shape[0]
    out = dict(dy_out=np.zeros((rows + 1, dim), np.float32), dbeta=np.zeros(dim + 1, np.float32), dgamma=np.zeros(dim + 1, np.float32),
               grad_bias=np.zeros(dim + 1, np.float32))
    a = BnDxArgs(rows=rows, dim=dim, dy=_ptr(dy), pre=_ptr(pre), mean=_ptr(mean), inv_std=_ptr(inv_std), sums=_ptr(sums),
                 n_global=float(n_global), **{k: _ptr(v) for k, v in out.items()})
    ca._lib.check(ca.lib().nvsm_debug_bn_dx(C.byref(a)))
    return out


BN_CASES = [(rows, dim, dp) for dim in (5, 12, 256) for rows in (1, 37) for dp in (False, True)] + [(GRID_CAP_ITEMS + 3, 4, False)]


@pytest.mark.parametrize("rows,dim,dp", BN_CASES, ids=["rows%d-dim%d-%s" % (r, d, "data-parallel" if p else "single") for r, d, p in BN_CASES])
def test_bn_dx(rows, dim, dp):
    """dims 5 (V = 1), 12 and 256 (V = 4); one row; rows · nvec past the grid cap at dim 4. Data-parallel: the statistics and the
    sums are those of 8 · rows rows, of which the launch holds the first `rows`, and n_global = 8 · rows."""
    rs = np.random.RandomState(rows % 1000 + dim + dp)
    n_all = 8 * rows if dp else rows
    allpre = (rs.standard_normal((n_all, dim)) + rs.uniform(-2, 2, dim)).astype(np.float32)
    alldy = (rs.standard_normal((n_all, dim)) * 0.1).astype(np.float32)
    mean = allpre.astype(np.float64).mean(axis=0).astype(np.float32)
    inv_std = (1.0 / np.sqrt(allpre.astype(np.float64).var(axis=0) + 1e-4)).astype(np.float32)
    sums = sk.bn_sums(alldy, allpre, mean, inv_std)
    dy, pre = np.ascontiguousarray(alldy[:rows]), np.ascontiguousarray(allpre[:rows])
    out = run_bn_dx(dy, pre, mean, inv_std, sums, n_all, dim)
    label = "bn_dx rows=%d dim=%d n=%d" % (rows, dim, n_all)
    assert is_ff(out["dy_out"][rows]) and all(is_ff(out[k][dim:]) for k in ("dbeta", "dgamma", "grad_bias")), label + ": a guard was written"
    ref, db, dg = sk.bn_dx(dy, pre, mean, inv_std, sums, n_all)
    ref32, _, _ = sk.bn_dx(dy, pre, mean, inv_std, sums, n_all, np.float32)
    hold_elementwise("bn_dx", out["dy_out"][:rows], ref, ref32, label)
    # the float casts of the sums, bit for bit, in all three
    assert same_bits(out["dbeta"][:dim], sums[0].astype(np.float32)) and same_bits(out["grad_bias"][:dim], sums[0].astype(np.float32)), label
    assert same_bits(out["dgamma"][:dim], sums[1].astype(np.float32)), label
    SEEN.add(("bn_dx", 4 if dim % 4 == 0 else 1))
    if rows * (dim // 4 if dim % 4 == 0 else dim) > GRID_CAP_ITEMS:
        SEEN.add(("bn_dx", "second trip"))


@pytest.mark.parametrize("dim", [5, 12, 256, 300])
def test_colsum_finalize(dim):
    """Without batch-norm the bias gradient is the float cast of Σ dy and nothing else is written (300: a second workgroup)."""
    rs = np.random.RandomState(dim)
    sums = rs.standard_normal((2, dim)) * 2.0 ** rs.randint(-10, 10, (2, dim))
    out = run_bn_dx(None, None, None, None, sums, 1.0, dim)
    assert same_bits(out["grad_bias"][:dim], sums[0].astype(np.float32)) and is_ff(out["grad_bias"][dim:])
    assert is_ff(out["dbeta"]) and is_ff(out["dgamma"])
    SEEN.add(("colsum_finalize",))


# ---- wave-per-row ops ----------------------------------------------------------------------------------------------------------------
ROW_DIMS = [1, 20, 63, 64, 65, 130, 300]
ROW_SHAPES = [(rows, dim) for dim in ROW_DIMS for rows in (1, 5)] + [(16389, 7)]      # 16 389 rows: a second trip of 4096 x 4 waves
MIN_NORM = 0.25


def row_values(rs, shape, dim):
    """N(0, 1) pushed 0.25 away from zero (every row norm is at least 0.25: no 0 / 0 in the normaliser). At dim 1 the normaliser's
    backward is zero but for rounding, and a relative bound on rounding noise would be an exemption: there the values are multiples
    of 1 / 4 below 8 - five significant bits, every product of three of them exact in float32 - and the result must be exactly zero."""
    if dim == 1:
        return (rs.randint(1, 32, shape) * rs.choice([-0.25, 0.25], shape)).astype(np.float32)
    x = rs.standard_normal(shape)
    return (x + np.where(x < 0, -MIN_NORM, MIN_NORM)).astype(np.float32)


def run_row_op(op, rows, dim, x, g=None, norms=None, coef=None, E=None, ids=None, R=0, scale=0.0, in_place=False, scalar=True, out=True):
    o = np.zeros((rows + 1, dim), np.float32) if out else None
    s = np.zeros(rows + 1, np.float32) if scalar else None
    a = RowOpArgs(op=op, rows=rows, dim=dim, x=_ptr(x), g=_ptr(g), norms=_ptr(norms), coef=_ptr(coef), E=_ptr(E),
                  table_rows=0 if E is None else E.shape[0], ids=_ptr(ids), R=R, scale=scale, in_place=int(in_place), out=_ptr(o),
                  out_scalar=_ptr(s))
    ca._lib.check(ca.lib().nvsm_debug_row_op(C.byref(a)))
    if o is not None:
        assert is_ff(o[rows]), "op %d rows=%d dim=%d: the guard row was written" % (op, rows, dim)
    if s is not None:
        assert is_ff(s[rows:]), "op %d rows=%d dim=%d: the guard element was written" % (op, rows, dim)
    return (None if o is None else o[:rows]), (None if s is None else s[:rows])


@pytest.mark.parametrize("rows,dim", ROW_SHAPES, ids=["rows%d-dim%d" % s for s in ROW_SHAPES])
def test_row_meansq_and_l2_normaliser(rows, dim):
    """t = ceil(dim / 64) + 6 + 2 for a wave's sum: a lane's elements, six shuffle steps, the product and the final factor. A norm
    is the root of such a sum - half its relative error and one rounding more, within the same t · 2^-24 of the norm."""
    rs = np.random.RandomState(1000 * dim + rows % 1000)
    t = sk.wave_sum_additions(dim) * U32
    label = "rows=%d dim=%d" % (rows, dim)
    x, g = row_values(rs, (rows, dim), dim), row_values(rs, (rows, dim), dim)
    scale = 0.5 if dim == 1 else 0.37
    x64 = x.astype(np.float64)
    assert np.sqrt((x64 * x64).sum(axis=1)).min() >= MIN_NORM
    # row mean of squares
    inv_dim = float(np.float32(1.0 / dim))
    _, msq = run_row_op(ROW_MEANSQ, rows, dim, g, scale=inv_dim, out=False)
    want = sk.row_meansq(g, inv_dim)
    hold("row_meansq", msq, want, t * want, label)
    # forward
    y, norms = run_row_op(ROW_L2_FORWARD, rows, dim, x)
    y64, n64 = sk.l2_forward(x)
    y32, _ = sk.l2_forward(x, np.float32)
    hold("l2_norms", norms, n64, t * n64, label)
    hold_elementwise("l2_forward", y, y64, y32, label)
    # backward on norms of the reference's own, out of place with and without the mean of squares, then in place
    nin = n64.astype(np.float32)
    gin, gmsq = run_row_op(ROW_L2_BACKWARD, rows, dim, x, g=g, norms=nin, scale=scale)
    hold_elementwise("l2_backward", gin, sk.l2_backward(g, x, nin, scale), sk.l2_backward(g, x, nin, scale, np.float32), label)
    own = (gin.astype(np.float64) ** 2).sum(axis=1) * float(sk.inv_dim_f32(dim))
    hold("l2_backward_msq", gmsq, own, t * own, label)
    gin0, _ = run_row_op(ROW_L2_BACKWARD, rows, dim, x, g=g, norms=nin, scale=scale, scalar=False)
    assert same_bits(gin0, gin), label + ": the gradient depends on whether the mean of squares is asked for"
    gin_ip, gmsq_ip = run_row_op(ROW_L2_BACKWARD, rows, dim, x, g=g, norms=nin, scale=scale, in_place=True)
    assert same_bits(gin_ip, gin) and same_bits(gmsq_ip, gmsq), label + ": in place (as Model::backward calls it) differs from out of place"
    SEEN.add(("row ops", "dim<64" if dim < 64 else "dim=64" if dim == 64 else "dim>64"))
    if rows > 4096 * 4:
        SEEN.add(("row ops", "second trip"))


@pytest.mark.parametrize("R", [1, 5, 17])
@pytest.mark.parametrize("B,dim", ROW_SHAPES, ids=["B%d-dim%d" % s for s in ROW_SHAPES])
def test_materialise_grad_entity(B, dim, R):
    """Entries j = 0 .. N - 1 read proj[j // R]; N = B · R for the small batches, 16 389 entries (no multiple of 5 or 17) for the
    large one. The plain kernel is one float32 product per element: the bits of numpy's. Through the normaliser: ids from a table of
    four rows, so every id repeats; with and without the mean of squares."""
    N = B * R if B < 100 else B
    rs = np.random.RandomState(100 * dim + 10 * R + B % 7)
    coef = row_values(rs, N, dim)
    proj = row_values(rs, ((N + R - 1) // R, dim), dim)
    E = row_values(rs, (4, dim), dim)
    ids = rs.randint(0, 4, N).astype(np.int32)
    label = "materialise N=%d dim=%d R=%d" % (N, dim, R)
    out, _ = run_row_op(ROW_MATERIALIZE, N, dim, proj, coef=coef, R=R, scalar=False)
    assert same_bits(out, sk.materialize(coef, proj, R, np.float32)), label
    e64 = E.astype(np.float64)
    assert np.sqrt((e64 * e64).sum(axis=1)).min() >= MIN_NORM
    out2, msq = run_row_op(ROW_MATERIALIZE_L2, N, dim, proj, coef=coef, E=E, ids=ids, R=R)
    hold_elementwise("materialise_l2", out2, sk.materialize_l2(coef, proj, E, ids, R), sk.materialize_l2(coef, proj, E, ids, R, np.float32), label)
    own = (out2.astype(np.float64) ** 2).sum(axis=1) * float(sk.inv_dim_f32(dim))
    hold("materialise_l2_msq", msq, own, sk.wave_sum_additions(dim) * U32 * own, label)      # t as above
    out3, _ = run_row_op(ROW_MATERIALIZE_L2, N, dim, proj, coef=coef, E=E, ids=ids, R=R, scalar=False)
    assert same_bits(out3, out2), label + ": the gradient depends on whether the mean of squares is asked for"
    SEEN.add(("materialise", R))


# ---- slab sums -----------------------------------------------------------------------------------------------------------------------
def binades(rs, shape):
    """Values over 24 binades, as the dT tests use."""
    return (rs.standard_normal(shape) * 2.0 ** rs.randint(-12, 12, shape)).astype(np.float32)


def run_slab_sum(which, parts, n):
    nparts, stride = parts.shape
    out = np.zeros(n + 1, np.float32)
    ca._lib.check(ca.lib().nvsm_debug_slab_sum(which, _ptr(parts), nparts, stride, n, _ptr(out)))
    assert is_ff(out[n:]), "slab sum %d: the guard was written" % which
    return out[:n]


def check_slab_sums(nparts, n, stride, seed):
    parts = binades(np.random.RandomState(seed), (nparts, stride))
    vec = n % 4 == 0 and stride % 4 == 0              # (both buffers are 16-byte aligned: launch_splitk_reduce's float4 kernel)
    want = sk.splitk_reduce_f32(parts[:, :n]) if vec else sk.splitk_reduce_scalar_f32(parts[:, :n])
    got = run_slab_sum(0, parts, n)
    assert same_bits(got, want), "splitk_reduce (%s) slabs=%d n=%d stride=%d: %d elements differ" % (
        "float4" if vec else "scalar", nparts, n, stride, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    got = run_slab_sum(1, parts, n)
    want = sk.sum_parts_f32(parts[:, :n])
    assert same_bits(got, want), "sum_parts parts=%d n=%d stride=%d: %d elements differ" % (
        nparts, n, stride, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    SEEN.add(("splitk_reduce", "float4" if vec else "scalar"))
    SEEN.add(("sum_parts", "clamped" if nparts % 8 else "whole"))
    if n > GRID_CAP_ITEMS:
        SEEN.add(("slab sums", "second trip"))


@pytest.mark.parametrize("n", [1000, 1003])
@pytest.mark.parametrize("nparts", [1, 2, 7, 8, 9, 15, 16, 17, 33, 128])
def test_slab_sums_bit_for_bit(nparts, n):
    """n = 1000: the float4 kernel, sixteen groups of slabs (at most one slab each up to 16 slabs, then 2, 3 and 8 deep); n = 1003:
    the scalar kernel, slab order. launch_sum_parts keeps eight parts in flight: 1, 2, 7, 9, 15, 17 and 33 end in a clamped round."""
    check_slab_sums(nparts, n, n, 10 * nparts + n)


@pytest.mark.parametrize("nparts,n,stride", [(17, 1000, 1004), (17, 1000, 1001), (33, 1003, 1004), (3, 16 * 4096 * 4 + 4, 16 * 4096 * 4 + 4),
                                            (3, 16 * 4096 * 4 + 3, 16 * 4096 * 4 + 3), (2, GRID_CAP_ITEMS + 259, GRID_CAP_ITEMS + 259)])
def test_slab_sums_strides_and_large_n(nparts, n, stride):
    """A stride beyond n (a multiple of 4: still the float4 kernel; not one: the scalar kernel); n just above 16 · 4096 · 4 on either
    kernel; and the scalar kernel and launch_sum_parts past the grid cap."""
    check_slab_sums(nparts, n, stride, nparts + n % 1000)


# ---- the dense optimiser of (T, b) -----------------------------------------------------------------------------------------------------
TU_SHAPES = [(300, 256), (260, 252), (364, 256), (20, 64), (36, 44)]      # K and N short of 32-, 16- and 32-element tiles
TU_STATE = ("T", "b", "gT", "gb", "s0T", "s0b", "s1T", "s1b")
LR = 0.01


def plane_sizes(kind, N, K):
    nbytes, stride = C.c_int64(-1), C.c_int64(-1)
    ca._lib.check(ca.lib().nvsm_debug_plane_sizes(kind, N, K, C.byref(nbytes), C.byref(stride)))
    assert (stride.value, nbytes.value) == sk.plane_geometry(kind, N, K)
    return nbytes.value, stride.value


def tu_inputs(method, dw, de, seed):
    """T of the size of a trained projection, gradients of 1e-3, second moments of their squares' size; nothing negative under a root."""
    rs = np.random.RandomState(seed)
    nT = dw * de
    f = lambda a: a.astype(np.float32)
    st = dict(T=f(rs.uniform(-0.1, 0.1, nT)), b=f(rs.uniform(-0.3, 0.3, de)), gT=f(rs.standard_normal(nT) * 1e-3), gb=f(rs.standard_normal(de) * 1e-3))
    if method == sk.ADAGRAD:
        st.update(s0T=f(rs.uniform(1e-6, 1e-3, nT)), s0b=f(rs.uniform(1e-6, 1e-3, de)))
    if method == sk.ADAM:
        st.update(s0T=f(rs.standard_normal(nT) * 1e-3), s0b=f(rs.standard_normal(de) * 1e-3),
                  s1T=f(rs.uniform(1e-8, 1e-5, nT)), s1b=f(rs.uniform(1e-8, 1e-5, de)))
    for k in ("s1T", "s1b") if method == sk.ADAM else ("s0T", "s0b") if method == sk.ADAGRAD else ():
        assert np.all(st[k] >= 0)
    return st


def run_transform_update(method, dw, de, st, lam, t, partial=None, kinds=(0, 0)):
    """-> (state after the update, without the guards; planes the update wrote; planes cut afresh from the updated T)."""
    nT = dw * de
    buf = {}
    for k in TU_STATE:
        if k in st:
            buf[k] = np.zeros(st[k].size + 1, np.float32)
            buf[k][:-1] = st[k]
    planes, fresh = [None, None], [None, None]
    for i, kind in enumerate(kinds):
        if kind:
            nbytes, _ = plane_sizes(kind, de if i == 0 else dw, dw if i == 0 else de)
            planes[i], fresh[i] = np.full(nbytes, 0x5A, np.uint8), np.full(nbytes, 0x5A, np.uint8)
    a = TransformUpdateArgs(method=method, dw=dw, de=de, lr=LR, lambda_=lam, t_transform=t, partial=_ptr(partial),
                            slabs=0 if partial is None else partial.shape[0], **{k: _ptr(v) for k, v in buf.items()})
    for i in range(2):
        a.plane_kind[i] = kinds[i]
        a.planes[i], a.fresh[i] = _ptr(planes[i]), _ptr(fresh[i])
    if partial is not None:
        assert partial.shape[1] == nT
    ca._lib.check(ca.lib().nvsm_debug_transform_update(C.byref(a)))
    for k, v in buf.items():
        assert is_ff(v[-1:]), "transform_update: the guard behind %s was written" % k
    return {k: v[:-1] for k, v in buf.items()}, planes, fresh


def check_planes(kinds, dw, de, T_new, planes, fresh, label):
    for i, kind in enumerate(kinds):
        if not kind:
            continue
        N, K = (de, dw) if i == 0 else (dw, de)
        Bmat = T_new.reshape(dw, de) if i == 0 else np.ascontiguousarray(T_new.reshape(dw, de).T)      # element (k, n) of the operand
        stride, total = sk.plane_geometry(kind, N, K)
        got, cut = planes[i], fresh[i]
        what = "%s pt[%d] kind %d" % (label, i, kind)
        assert same_bits(got[:3 * stride], cut[:3 * stride]), "%s: %d bytes differ from the freshly cut planes" % (
            what, int((got[:3 * stride] != cut[:3 * stride]).sum()))
        assert not got[3 * stride:].any(), what + ": the update wrote behind the third plane"
        pieces = sk.decode_planes(kind, N, K, got)
        for name, g, w in zip("hml", pieces, sk.split3(Bmat)):
            assert np.array_equal(g, w), "%s: piece %s differs in %d elements" % (what, name, int((g != w).sum()))
        assert same_bits(got[:3 * stride], sk.encode_planes(kind, N, K, Bmat)), what + ": the padding is not zero"


TU_CASES = [(method, t, lam, shape) for shape in TU_SHAPES for lam in (0.0, 0.01)
            for method, t in ((sk.SGD, 1), (sk.ADAGRAD, 1), (sk.ADAM, 1), (sk.ADAM, 12))]
TU_KINDS = [(1, 2), (2, 1), (1, 1), (2, 2), (0, 1), (2, 0)]


@pytest.mark.parametrize("i", range(len(TU_CASES)), ids=["%s-t%d-lambda%g-%dx%d" % (("sgd", "adagrad", "adam")[c[0]], c[1], c[2], c[3][0], c[3][1]) for c in TU_CASES])
def test_transform_update(i):
    method, t, lam, (dw, de) = TU_CASES[i]
    kinds = TU_KINDS[(i + i // 4) % len(TU_KINDS)]
    st = tu_inputs(method, dw, de, 500 + i)
    new, planes, fresh = run_transform_update(method, dw, de, st, lam, t, kinds=kinds)
    label = "transform_update %s t=%d lambda=%g %dx%d" % (("sgd", "adagrad", "adam")[method], t, lam, dw, de)
    g = lambda k: st.get(k)
    args = (method, g("T"), g("b"), g("gT"), g("gb"), g("s0T"), g("s0b"), g("s1T"), g("s1b"), LR, lam, t)
    r64, r32 = sk.transform_update(*args), sk.transform_update(*args, dtype=np.float32)
    assert set(r64) == set(new)
    for k in new:
        hold_elementwise("transform_" + k, new[k], r64[k], r32[k], label)
    if method == sk.SGD:
        assert same_bits(new["gT"], st["gT"]) and same_bits(new["gb"], st["gb"]), label + ": SGD leaves the gradients"
    # the bias quirks on their own: λ never reaches b or its state ...
    if lam:
        zero, _, _ = run_transform_update(method, dw, de, st, 0.0, t)
        for k in ("b", "gb", "s0b", "s1b"):
            if k in new:
                assert same_bits(new[k], zero[k]), "%s: lambda reached %s" % (label, k)
        assert not same_bits(new["T"], zero["T"])
    # ... and the Adam moments of the bias are scaled by 1, where β would leave them elsewhere by a hundred allowances
    if method == sk.ADAM:
        for k, beta, grad in (("s0b", sk.BETA1, st["gb"].astype(np.float64)), ("s1b", sk.BETA2, st["gb"].astype(np.float64) ** 2)):
            decayed = st[k].astype(np.float64) * float(beta) + grad * (1.0 - float(beta))
            assert np.abs(new[k] - decayed).max() > 100 * sk.elementwise_tol(r64[k], r32[k]), (label, k)
    check_planes(kinds, dw, de, new["T"], planes, fresh, label)
    for i_pt, kind in enumerate(kinds):
        if kind:
            SEEN.add(("transform_update", method, kind, i_pt))


@pytest.mark.parametrize("method", [sk.SGD, sk.ADAGRAD, sk.ADAM], ids=["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("slabs,shape", [(1, (20, 64)), (16, (36, 44)), (17, (20, 64)), (50, (36, 44)), (50, (300, 256))],
                         ids=lambda v: str(v))
def test_transform_update_adds_the_slabs_as_splitk_reduce_does(slabs, shape, method):
    """With the dT product's slabs given, every output has the bits of an update handed gT = launch_splitk_reduce(slabs); the gT that
    goes in is NaN and must not be read. SGD leaves that sum in gT. The planes of this run (with the slabs) are checked too."""
    dw, de = shape
    nT = dw * de
    st = tu_inputs(method, dw, de, 900 + slabs + method)
    partial = binades(np.random.RandomState(slabs), (slabs, nT)) * np.float32(1e-3)
    summed = run_slab_sum(0, partial, nT)
    assert nT % 4 == 0 and same_bits(summed, sk.splitk_reduce_f32(partial))
    label = "transform_update with %d slabs %dx%d method %d" % (slabs, dw, de, method)
    kinds = TU_KINDS[(slabs + method) % 4]
    a, planes, fresh = run_transform_update(method, dw, de, dict(st, gT=np.full(nT, np.nan, np.float32)), 0.01, 3, partial=partial, kinds=kinds)
    b, _, _ = run_transform_update(method, dw, de, dict(st, gT=summed), 0.01, 3)
    for k in a:
        if not (method == sk.SGD and k == "gT"):
            assert same_bits(a[k], b[k]), "%s: %s differs in %d elements" % (label, k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()))
    if method == sk.SGD:
        assert same_bits(a["gT"], summed), label + ": gT does not hold the slabs' sum"
    check_planes(kinds, dw, de, a["T"], planes, fresh, label)
    SEEN.add(("transform_update", "slabs", min(slabs, 17)))


def test_hooks_refuse_bad_sizes_and_ids():
    """Refused on the host with NVSM_ERR_INVALID_ARGUMENT: nothing of this reaches the device."""
    m, v = np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    for bad in (4, -1):
        idx = np.array([[0, bad]], np.int32)
        for call in (lambda: run_adam_u(m, v, idx, 1.0, 1e-6), lambda: run_adagrad_scale(v, idx, 1e-6)):
            with pytest.raises(ca.NvsmError) as e:
                call()
            assert e.value.status == 1
        with pytest.raises(ca.NvsmError) as e:
            run_row_op(ROW_MATERIALIZE_L2, 2, 3, m[:2], coef=v[:2], E=m, ids=np.array([0, bad], np.int32), R=1)
        assert e.value.status == 1
    out = np.zeros(5, np.float32)
    for which, nparts, stride, n in ((2, 1, 4, 4), (0, 0, 4, 4), (0, 1, 3, 4), (1, 1, 4, 0)):
        assert ca.lib().nvsm_debug_slab_sum(which, _ptr(np.zeros(8, np.float32)), nparts, stride, n, _ptr(out)) == 1
    with pytest.raises(ca.NvsmError) as e:
        run_row_op(7, 2, 3, m[:2])
    assert e.value.status == 1
    with pytest.raises(ca.NvsmError) as e:
        run_transform_update(sk.ADAM, 2, 4, tu_inputs(sk.SGD, 2, 4, 1), 0.0, 1)      # Adam without its state
    assert e.value.status == 1
    with pytest.raises(ca.NvsmError) as e:
        run_transform_update(3, 2, 4, tu_inputs(sk.SGD, 2, 4, 1), 0.0, 1)
    assert e.value.status == 1


def test_every_path_was_launched():
    """Every (V, U) of adam_u, every method x plane kind x transposed of the projection update, both reduce kernels and the other
    paths the cases above were written for were launched in this session."""
    want = {("adam_u", v, u) for v in (1, 4) for u in range(1, 11)}
    want |= {("transform_update", m, kind, tr) for m in (sk.SGD, sk.ADAGRAD, sk.ADAM) for kind in (1, 2) for tr in (0, 1)}
    want |= {("transform_update", "slabs", s) for s in (1, 16, 17)}
    want |= {("splitk_reduce", "float4"), ("splitk_reduce", "scalar"), ("sum_parts", "clamped"), ("sum_parts", "whole")}
    want |= {(k, "second trip") for k in ("adam_u", "adagrad_scale", "bn_dx", "row ops", "slab sums")}
    want |= {("adagrad_scale", "tail"), ("adagrad_scale", "whole"), ("bn_dx", 1), ("bn_dx", 4), ("colsum_finalize",)}
    want |= {("row ops", d) for d in ("dim<64", "dim=64", "dim>64")} | {("materialise", R) for R in (1, 5, 17)}
    want |= {("gather_mean", v, u, "tail") for v in (1, 4) for u in (4, 5)} | {("gather_mean", v, u, "whole") for v in (1, 4) for u in (3, 4, 5)}
    if not SEEN:
        pytest.skip("selected on its own: the table is filled by the cases of this file")
    assert want <= SEEN, sorted(map(str, want - SEEN))
    print("step-kernels worst |g - ref| / bound per quantity: " + " ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
