"""No GPU: tests/step_kernels_reference.py against the CPU oracle on small inputs, its float32 emulations against hand-worked
cases, and the ctypes mirrors of the new hook structs against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from oracle import nvsm_oracle as orc
from tests import step_kernels_reference as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-300)


# ---- the float64 restatements against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 4, 7, 11])
def test_window_passes_against_the_oracle(window):
    rs = np.random.RandomState(window)
    rows, dim, B = 23, 7, 13
    table = rs.standard_normal((rows, dim))
    v = rs.uniform(0.0, 2.0, rows)
    idx = rs.randint(0, rows, (B, window))
    wts = rs.uniform(0.2, 2.0, (B, window))
    for w in (None, wts):
        mean, mag = sk.gather_mean(table, idx, w)
        assert close(mean, orc.average_repr(table.ravel(), dim, idx.ravel(), None if w is None else w.ravel(), window))
        assert np.all(mag >= np.abs(mean) - 1e-12)
    mean_m = orc.average_repr(table.ravel(), dim, idx.ravel(), None, window).reshape(B, dim)
    mean_v = orc.average_repr(v, 1, idx.ravel(), None, window)
    assert close(sk.adam_u(table, v, idx, 0.37, 1e-6), 0.37 * mean_m / (np.sqrt(mean_v) + 1e-6)[:, None])
    assert close(sk.adagrad_scale(v, idx, 1e-6), 1.0 / np.sqrt(mean_v + 1e-6))
    # the float32 evaluation is the same formula: it differs by float32 rounding and no more
    u32 = sk.adam_u(table, v, idx, 0.37, 1e-6, np.float32)
    assert u32.dtype == np.float32 and close(u32, sk.adam_u(table, v, idx, 0.37, 1e-6), rel=1e-5)


def test_bn_dx_against_the_oracle():
    rs = np.random.RandomState(2)
    rows, dim = 37, 5
    pre = rs.standard_normal((rows, dim)) + rs.uniform(-2, 2, dim)
    dy = rs.standard_normal((rows, dim)) * 0.1
    _, mean, inv_std = orc.bn_forward(pre.ravel(), rows, dim, np.zeros(dim), 1e-4)
    want, gb = orc.bn_backward(dy.ravel(), pre.ravel(), rows, dim, mean, inv_std)
    sums = sk.bn_sums(dy, pre, mean, inv_std)
    assert close(sums[0], gb)
    dx, db, dg = sk.bn_dx(dy, pre, mean, inv_std, sums, rows)
    # the restatement casts dβ, dγ and 1 / n to float, as the kernel's contract says; the oracle keeps doubles: 3 roundings of 2^-24
    xhat = (pre - mean) * inv_std
    slack = 4 * 2.0 ** -24 * inv_std * (np.abs(sums[0]) + np.abs(xhat * sums[1])) / rows + 1e-15
    assert np.all(np.abs(dx - want.reshape(rows, dim)) <= slack)
    assert np.array_equal(db, sums[0].astype(np.float32).astype(np.float64)) and np.array_equal(dg, sums[1].astype(np.float32).astype(np.float64))
    # the data-parallel form divides by the global row count
    dx8, _, _ = sk.bn_dx(dy, pre, mean, inv_std, sums, 8 * rows)
    assert not close(dx8, dx, rel=1e-3)


@pytest.mark.parametrize("dim", [1, 20, 65])
def test_normaliser_against_the_oracle(dim):
    rs = np.random.RandomState(dim)
    rows = 9
    x = rs.standard_normal((rows, dim)) + 0.1
    g = rs.standard_normal((rows, dim))
    y, n = sk.l2_forward(x)
    yo, no = orc.normalizer_forward(x.ravel(), rows, dim)
    assert close(y, yo) and close(n, no)
    # (at dim 1 the result is zero but for rounding: the difference is held to the size of the terms that cancel, |g| / n)
    diff = np.abs(sk.l2_backward(g, x, n, 1.0) - orc.normalizer_backward(g.ravel(), x.ravel(), no, rows, dim).reshape(rows, dim))
    assert diff.max() <= 1e-13 * (np.abs(g) / n[:, None]).max()
    assert close(sk.l2_backward(g, x, n, 0.25), 0.25 * sk.l2_backward(g, x, n, 1.0))
    assert close(sk.row_meansq(g, 1.0 / dim), (g * g).mean(axis=1))
    # the materialise ops: entries j read proj[j // R]; through the normaliser with the gathered raw rows
    R = 3
    coef, ids = rs.standard_normal(rows), rs.randint(0, 5, rows)
    proj, E = rs.standard_normal(((rows + R - 1) // R, dim)), rs.standard_normal((5, dim)) + 0.1
    plain = sk.materialize(coef, proj, R)
    assert all(np.array_equal(plain[j], proj[j // R] * coef[j]) for j in range(rows))
    e = E[ids]
    _, ne = orc.normalizer_forward(e.ravel(), rows, dim)
    diff = np.abs(sk.materialize_l2(coef, proj, E, ids, R) - orc.normalizer_backward(plain.ravel(), e.ravel(), ne, rows, dim).reshape(rows, dim))
    assert diff.max() <= 1e-13 * (np.abs(plain) / ne[:, None]).max()


@pytest.mark.parametrize("lam", [0.0, 0.01])
@pytest.mark.parametrize("method", [sk.SGD, sk.ADAGRAD, sk.ADAM])
def test_transform_update_against_the_oracle(method, lam):
    """Three updates from T = b = 0.3 and zero state (what the oracle's storage can be set to), the step count running 1, 2, 3."""
    rs = np.random.RandomState(10 * method + int(lam > 0))
    dw, de, lr = 5, 4, 0.05
    o = orc.Transform(dw, de, method, beta1=float(sk.BETA1), beta2=float(sk.BETA2), eps=float(sk.OPT_EPS))
    o.fill(0.3)
    st = dict(T=np.full(dw * de, 0.3), b=np.full(de, 0.3), s0T=np.zeros(dw * de), s0b=np.zeros(de), s1T=np.zeros(dw * de), s1b=np.zeros(de))
    for t in (1, 2, 3):
        gT, gb = rs.standard_normal(dw * de), rs.standard_normal(de)
        ogT, ogb = o.update(gT, gb, float(np.float32(lr)), float(np.float32(lam)))
        new = sk.transform_update(method, st["T"], st["b"], gT, gb, st["s0T"], st["s0b"], st["s1T"], st["s1b"], lr, lam, t)
        st.update(new)
        assert close(new["gT"], ogT) and close(new["gb"], ogb), t
        assert close(st["T"], o.get(0)) and close(st["b"], o.get(1)), t
        if method != sk.SGD:
            assert close(st["s0T"], o.get(2)) and close(st["s0b"], o.get(3)), t
        if method == sk.ADAM:
            assert close(st["s1T"], o.get(4)) and close(st["s1b"], o.get(5)), t


@pytest.mark.parametrize("method", [sk.SGD, sk.ADAGRAD, sk.ADAM])
def test_transform_update_bias_quirks(method):
    """λ never reaches the bias, and the Adam moments of the bias are scaled by 1: b and its state after an update with λ = 0.5 are
    those of an update with λ = 0, and the first moment of the bias GROWS by (1 − β1) · g where T's is also scaled by β1."""
    rs = np.random.RandomState(method)
    n = 6
    T, b, gT, gb = (rs.standard_normal(n) for _ in range(4))
    s0, s1 = rs.uniform(0.5, 1.0, n), rs.uniform(0.5, 1.0, n)
    a = sk.transform_update(method, T, b, gT, gb, s0, s0.copy(), s1, s1.copy(), 0.1, 0.5, 3)
    z = sk.transform_update(method, T, b, gT, gb, s0, s0.copy(), s1, s1.copy(), 0.1, 0.0, 3)
    for k in ("b", "gb", "s0b", "s1b"):
        if k in a:
            assert np.array_equal(a[k], z[k]), k
    assert not np.array_equal(a["T"], z["T"])
    if method == sk.ADAM:
        one_m_b1 = 1.0 - np.float64(sk.BETA1)
        assert np.allclose(a["s0b"], s0 + gb * one_m_b1, rtol=1e-15)
        assert np.allclose(z["s0T"], s0 * (1.0 - one_m_b1) + gT * one_m_b1, rtol=1e-15)


# ---- the float32 emulations --------------------------------------------------------------------------------------------------------
def test_ordered_sums_add_in_the_documented_order():
    big = np.float32(2.0 ** 24)
    parts = np.zeros((17, 1), np.float32)
    parts[0], parts[1], parts[16] = big, -big, 1.0
    # group 0 = (2^24 + 1) -> 2^24 in float32, group 1 = −2^24: 0. In slab order: (2^24 − 2^24) + 1 = 1.
    assert sk.splitk_reduce_f32(parts)[0] == 0.0
    assert sk.splitk_reduce_scalar_f32(parts)[0] == 1.0 and sk.sum_parts_f32(parts)[0] == 1.0
    rs = np.random.RandomState(3)
    for slabs in (1, 2, 7, 16):                      # up to sixteen slabs a group holds one slab: slab order
        p = (rs.standard_normal((slabs, 50)) * 2.0 ** rs.randint(-20, 20, (slabs, 50))).astype(np.float32)
        assert np.array_equal(sk.splitk_reduce_f32(p), sk.splitk_reduce_scalar_f32(p))
        assert np.array_equal(sk.sum_parts_f32(p), sk.splitk_reduce_scalar_f32(p))
    ints = rs.randint(-1000, 1000, (128, 40)).astype(np.float32)          # exact in any order
    for f in (sk.splitk_reduce_f32, sk.splitk_reduce_scalar_f32, sk.sum_parts_f32):
        assert f(ints).dtype == np.float32 and np.array_equal(f(ints), ints.sum(axis=0))
    p = (rs.standard_normal((50, 4000)) * 2.0 ** rs.randint(-12, 12, (50, 4000))).astype(np.float32)
    assert (sk.splitk_reduce_f32(p) != sk.splitk_reduce_scalar_f32(p)).any()      # the two orders are told apart by data like the tests'


def test_bf16_rounding_is_to_nearest_even():
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)
    assert sk.bf16_round(f(0x3F800000))[0] == 0x3F80
    assert sk.bf16_round(f(0x3F807FFF))[0] == 0x3F80          # below the tie
    assert sk.bf16_round(f(0x3F808000))[0] == 0x3F80          # tie, even stays
    assert sk.bf16_round(f(0x3F818000))[0] == 0x3F82          # tie, odd goes up
    assert sk.bf16_round(f(0x3F808001))[0] == 0x3F81
    assert sk.bf16_round(f(0xBF818000))[0] == 0xBF82
    assert sk.bf16_value(np.array([0x3F80, 0xC000], np.uint16)).tolist() == [1.0, -2.0]


def test_three_pieces_reproduce_the_float_exactly():
    """h + m + l == x for every mantissa (all 2^23 at one exponent, both signs) and, with 4096 mantissas each (the edge patterns and
    random ones), at every exponent at which the claim can hold: the lowest bit of x, 2^(e − 23), must be a bf16 value, i.e. at least
    the smallest bf16 subnormal 2^-133 - e >= −110 -, and bf16(x) must not round up to infinity, which excludes the 2^15 largest
    magnitudes of exponent 127. (The trained projection lives some thirty binades inside either end.)"""
    def exact(x):
        h, m, l = sk.split3(x)
        s = sk.bf16_value(h).astype(np.float64) + sk.bf16_value(m).astype(np.float64) + sk.bf16_value(l).astype(np.float64)
        return s == x.astype(np.float64)
    mant = np.arange(1 << 23, dtype=np.uint32)
    for sign in (0, 0x80000000):
        assert exact((mant | np.uint32(127 << 23) | np.uint32(sign)).view(np.float32)).all()
    rs = np.random.RandomState(5)
    edge = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0x17FFF, 0x18000, 0x18001, 0x7F7FFF, 0x7F8000 - 1, 0x400000, 0x3FFFFF, 0x7F0000], np.uint32)
    some = np.concatenate([edge, rs.randint(0, 1 << 23, 4096 - edge.size).astype(np.uint32)])
    for e in range(-110, 128):
        x = (some | np.uint32((e + 127) << 23)).view(np.float32)
        if e == 127:
            x = x[some < 0x7F8000]
        assert np.isfinite(x).all() and exact(x).all() and exact(-x).all(), e
    # ... and outside that range it does not hold: the restriction is real
    assert not exact(np.array([0x00800001], np.uint32).view(np.float32)).all()


@pytest.mark.parametrize("kind", [1, 2])
def test_plane_offsets(kind):
    """Every element of the matrix has two bytes of its own inside the plane; encode and decode are inverse; and two offsets worked
    out by hand from the layout comments."""
    if kind == 1:      # np = 32 columns: [k // 32 = 1][n = 5][k % 32 = 1]
        assert sk.plane_offset(1, 20, 40, 33, 5) == (1 * 32 + 5) * 64 + 1 * 2
        assert sk.plane_geometry(1, 20, 40) == (2 * 32 * 64, 3 * 2 * 32 * 64 + 2048)
    else:              # NT = 2: k step 1, tile 1, lane 5 + 32 · 1, element 3
        assert sk.plane_offset(2, 64, 40, 27, 37) == (((1 * 2 + 1) * 64 + 37) * 16) + 3 * 2
        assert sk.plane_geometry(2, 64, 40) == (4 * 2 * 1024, 3 * 4 * 2 * 1024)      # three k steps padded to four
    rs = np.random.RandomState(kind)
    for N, K in ((256, 300), (300, 256), (252, 260), (260, 252), (256, 364), (64, 20), (20, 64), (44, 36), (36, 44)):
        stride, total = sk.plane_geometry(kind, N, K)
        k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
        off = sk.plane_offset(kind, N, K, k, n).ravel()
        assert off.min() >= 0 and off.max() + 2 <= stride and np.all(off % 2 == 0) and np.unique(off).size == off.size
        assert total >= 3 * stride
        B = (rs.standard_normal((K, N)) * 2.0 ** rs.randint(-8, 8, (K, N))).astype(np.float32)
        buf = sk.encode_planes(kind, N, K, B)
        h, m, l = sk.decode_planes(kind, N, K, buf)
        want = sk.split3(B)
        assert np.array_equal(h, want[0]) and np.array_equal(m, want[1]) and np.array_equal(l, want[2])
        assert np.count_nonzero(buf) <= 6 * N * K
        # the product's own sizes (host arithmetic, no device)
        nbytes, pstride = C.c_int64(-1), C.c_int64(-1)
        ca._lib.check(ca.lib().nvsm_debug_plane_sizes(kind, N, K, C.byref(nbytes), C.byref(pstride)))
        assert (pstride.value, nbytes.value) == (stride, total), (kind, N, K)


def test_tolerance_helpers():
    assert [sk.wave_sum_additions(d) for d in (1, 63, 64, 65, 130, 300)] == [9, 9, 9, 10, 11, 13]
    a = np.array([1.0, -2.0])
    assert sk.elementwise_tol(a, a) == 2e-6
    assert np.isclose(sk.elementwise_tol(a, a + np.array([1e-3, 0.0])), 4e-3 + 2e-6)
    assert sk.inv_dim_f32(3) == np.float32(1.0 / 3.0) and sk.inv_dim_f32(256) == np.float32(2.0 ** -8)


def test_hook_structs_match_their_ctypes_mirrors(tmp_path):
    """The new argument structs of include/cunvsm_amd_test_hooks.h against cunvsm_amd/_lib.py: size, every offset, no field missing
    (as tests/test_abi.py does for the older ones)."""
    pairs = [("nvsm_debug_bn_dx_args", ca._lib.BnDxArgs), ("nvsm_debug_row_op_args", ca._lib.RowOpArgs),
             ("nvsm_debug_transform_update_args", ca._lib.TransformUpdateArgs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cunvsm_amd_test_hooks.h"', 'int main(void) {']
    for cname, mirror in pairs:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in mirror._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field.rstrip("_")))
    lines += ['    return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    with open(os.path.join(ROOT, "include", "cunvsm_amd_test_hooks.h")) as f:
        header = f.read()
    for cname, mirror in pairs:
        assert int(got[cname]) == C.sizeof(mirror), cname
        for field, _ in mirror._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(mirror, field).offset, (cname, field)
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct " + cname):header.index("} " + cname)], flags=re.S)
        body = body[body.index("{") + 1:]
        declared = sum(len(stmt.split(",")) for stmt in body.split(";") if stmt.strip())
        assert declared == len(mirror._fields_), (cname, declared, len(mirror._fields_))
