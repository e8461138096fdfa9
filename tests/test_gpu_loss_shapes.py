"""-m gpu: ONE launch_loss (csrc/loss_bn.hip) on chosen inputs through nvsm_debug_loss, element by element against
tests/loss_reference.py, across the dispatch table of the loss kernels.

Every other check of these kernels compares a norm over a whole tensor with the oracle: at 1024 examples one row that is half a
percent wrong passes, and so does a clamped re-read of the wrong row in a ragged last set of rows, a wrong sign on one candidate or
one stale lazy row. Here every element of proj, pp, probs, the signed multipliers, dy, μ and 1/sqrt(σ² + ε) is held to the float64
restatement, within K_F32 times what a plain float32 evaluation of the same formulas loses (taken over the tensor) plus 1e-6 of the
tensor's largest magnitude (the floor of test_gpu_magnitudes.py). The column sums and the loss word - the ordered grid-wide sum - are
held to float64 sums of the launch's OWN dy and probs within t · 2^-24 · Σ|term|, t = 4 · (examples per wave) + 2 float32 additions.

The inputs keep the float64 logits within |s| <= 8 (asserted), far from the clamps of the sigmoid: no band logic. With batch-norm
and hard_tanh a unit whose float64 activation lies within 1e-5 of a clip bound may be clipped on one side and not on the other; its
dy element is held to the float32 restatement instead, and such units are at most 0.1 % of a case's elements (asserted).

Each case also asserts the plan launch_loss took (kernels.h LossPlan) against the one it was written for, that every element the
kernel owns is finite and every guard element untouched, that the arrival counters are back at zero, and that three launches on one
workspace return the bits of one. test_every_instantiation_was_launched closes the file: rows 6 / 11 / 17 each eager, lazy, pipe and
lazy + pipe, and the generic <1,1> <1,2> <1,4> <4,1> <4,2> <4,4> each with and without the entity normaliser.

What four deliberately broken builds of the kernels (never committed) do to this file is recorded in profiles/NOTES_loss_shapes.md."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd._lib import LossArgs
from tests import loss_reference as lr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_parity import SPECS

pytestmark = pytest.mark.gpu

K_F32 = 4
U32 = 2.0 ** -24
LOGIT_MAX = 8.0
ROWS = 97                       # a table of a few rows: ids repeat inside an example and are shared between examples
PIPE_BYTES = 256 << 20          # loss_two_row_sets: a table beyond the Infinity Cache
SEEN = set()                    # plan names of the launches of this session
WORST = {}                      # tensor -> worst |g - ref64| / bound over the file


def plan_name(p):
    if p["family"] == 1:
        return "rows<%d%s%s>" % (p["rb"], ",lazy" if p["lazy"] else "", ",pipe" if p["pipe"] else "")
    return "generic<%d,%d%s>" % (p["v"], p["niter"], ",l2e" if p["l2e"] else "")


def expected_plan(B, de, R, l2=False, lazy=False, pipe=False):
    """The dispatch table written down by hand (NOT a call of the product's loss_plan): name, examples per wave, workgroups."""
    if de % 4 == 0 and de <= 256 and R <= 64 and not l2:
        rb = 6 if R <= 6 else (11 if R <= 11 else 17)
        pipe = pipe and R <= rb
        epw = {2049: 2, 4097: 3, 6145: 4, 8193: 2, 40961: 27 if pipe else 20}.get(B, 1)
        assert B in (2049, 4097, 6145, 8193, 40961) or B < 2048
        name = "rows<%d%s%s>" % (rb, ",lazy" if lazy else "", ",pipe" if pipe else "")
    else:
        v = 4 if de % 4 == 0 else 1
        niter = (1 if de <= 256 else 2 if de <= 512 else 4) if v == 4 else (1 if de <= 64 else 2 if de <= 128 else 4)
        epw = 8
        name = "generic<%d,%d%s>" % (v, niter, ",l2e" if l2 else "")
    return name, epw, (B + 4 * epw - 1) // (4 * epw)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def run_loss(inp, repeats=1):
    """The inputs through the hook: (outputs with their guards, plan, arrival counters left)."""
    B, de, R = inp.B, inp.de, inp.R
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    pre, E, bias, inst_w = f32(inp.pre), f32(inp.E), f32(inp.bias), f32(inp.inst_w)
    ids = np.ascontiguousarray(inp.ids, dtype=np.int32)
    out = dict(proj=np.zeros((B + 1, de), np.float32), dy=np.zeros((B + 1, de), np.float32), coef=np.zeros((B + 1, R), np.float32),
               probs=np.zeros((B + 1, R), np.float32), pp=np.zeros(B + 1, np.float32), bn_mean=np.zeros((2, de), np.float32),
               bn_inv_std=np.zeros((2, de), np.float32), loss=np.zeros(1, np.float64), colstats=np.zeros((3, de), np.float64))
    plan = (C.c_int * 10)(*([-1] * 10))
    left = C.c_int(-1)
    a = LossArgs(B=B, de=de, R=R, k=inp.k, pre=_ptr(pre), bn=int(inp.bn), bn_sums=_ptr(inp.bn_sums), bn_n=inp.bn_n, bias=_ptr(bias),
                 E=_ptr(E), rows=inp.rows, ids=_ptr(ids), inst_w=_ptr(inst_w), nonlinearity=inp.nonlinearity,
                 clip_sigmoid=int(inp.clip_sigmoid), bias_negative_samples=int(inp.bias_negative_samples), l2_entity=int(inp.l2_entity),
                 b_global=inp.b_global, stamp=_ptr(inp.stamp), decay=_ptr(inp.decay), now=inp.now,
                 rows_for_dispatch=inp.rows_for_dispatch, repeats=repeats,
                 plan=plan, arrive_left=C.pointer(left), **{k: _ptr(v) for k, v in out.items()})
    ca._lib.check(ca.lib().nvsm_debug_loss(C.byref(a)))
    names = ("family", "rb", "lazy", "pipe", "v", "niter", "l2e", "epw", "grid", "shmem")
    return out, dict(zip(names, plan)), left.value


def same_bits(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s differs in %d elements" % (
                what, k, int((a[k].view(np.uint32 if a[k].itemsize == 4 else np.uint64) != b[k].view(np.uint32 if b[k].itemsize == 4 else np.uint64)).sum()))


def is_ff(a):
    return np.all(a.view(np.uint8) == 0xFF)


def make_inputs(B, de, R, bn, nl, seed, inst_w=True, bias_neg=False, clip=True, l2=False, dp=False, const_col=None, k=None):
    """pre ~ N(0, 1) (+ a per-column offset with batch-norm), document rows ~ N(0, 1.2² / de): the logits have a standard deviation of
    at most 1.2 (|proj| <= 1), |s| <= 8 is seven of them. dp: the data-parallel form, statistics over 8 B rows and 1 / (8 B) in the
    multipliers."""
    rs = np.random.RandomState(seed)
    n_stat = 8 * B if dp else B
    allpre = rs.standard_normal((n_stat, de))
    if bn:
        allpre += rs.uniform(-2, 2, de)
        if const_col is not None:
            allpre[:, const_col] = 3.7
    allpre = allpre.astype(np.float32)
    pre = allpre[:B]
    E = (rs.standard_normal((ROWS, de)) * (1.2 / np.sqrt(de))).astype(np.float32)
    E[E == 0] = np.float32(0.01)
    ids = rs.randint(0, ROWS, (B, R)).astype(np.int32)
    if R >= 2:
        rep = rs.rand(B) < 0.34
        ids[rep, R - 1] = ids[rep, 0]                       # the positive drawn again as a negative
        if R >= 3:
            ids[rep, R // 2] = ids[rep, 1]
    bias = rs.uniform(-0.3, 0.3, de).astype(np.float32)
    iw = rs.uniform(0.25, 2.0, B).astype(np.float32) if inst_w else None
    return lr.LossInputs(pre=pre, E=E, ids=ids, k=k, bn=bn, bn_sums=lr.column_sums(allpre) if bn else None, bn_n=n_stat,
                         bias=bias if bn else None, inst_w=iw, nonlinearity=nl, clip_sigmoid=clip, bias_negative_samples=bias_neg,
                         l2_entity=l2, b_global=n_stat)


def check_elementwise(inp, out, plan, label):
    B, de, R = inp.B, inp.de, inp.R
    r64, r32 = lr.loss_reference(inp, np.float64), lr.loss_reference(inp, np.float32)
    assert np.abs(r64["logits"]).max() <= LOGIT_MAX, np.abs(r64["logits"]).max()
    assert np.all(np.abs(inp.E).sum(axis=1) > 0)      # no zero rows
    # ---- owned elements finite, guards untouched, what the launch does not own untouched ----
    owned = {}
    for t in ("proj", "dy", "coef", "probs", "pp"):
        owned[t] = out[t][:B]
        assert is_ff(out[t][B:]), "%s: the guard behind %s was written" % (label, t)
    for t in ("bn_mean", "bn_inv_std"):
        assert is_ff(out[t][1]), "%s: the guard behind %s was written" % (label, t)
        if inp.bn:
            owned[t] = out[t][0]
        else:
            assert is_ff(out[t][0]), "%s: %s was written without batch-norm" % (label, t)
    assert is_ff(out["colstats"][2]) and (inp.bn or is_ff(out["colstats"][1]))
    for t, v in owned.items():
        assert np.all(np.isfinite(v)), "%s: %s has non-finite elements" % (label, t)
    assert np.all(np.isfinite(out["loss"])) and np.all(np.isfinite(out["colstats"][:2 if inp.bn else 1]))
    # ---- element by element ----
    near = np.zeros((B, de), bool)
    if inp.bn and inp.nonlinearity == 1:
        near = np.abs(np.abs(r64["act_in"]) - 1.0) < 1e-5
        assert near.mean() <= 1e-3, near.mean()
    ratios = {}
    for t, g in owned.items():
        ref, ref32 = r64[t], r32[t].astype(np.float64)
        tol = K_F32 * np.abs(ref32 - ref).max() + 1e-6 * np.abs(ref).max()
        err = np.abs(g.astype(np.float64) - ref)
        if t == "dy" and near.any():
            err = np.where(near, np.abs(g.astype(np.float64) - ref32), err)
        ratios[t] = float(err.max() / tol)
        WORST[t] = max(WORST.get(t, 0.0), ratios[t])
    # ---- the ordered sums against float64 sums of the launch's own dy and probs ----
    t_add = (4 * plan["epw"] + 2) * U32
    dy = owned["dy"].astype(np.float64)
    sums = {"colsum_dy": (out["colstats"][0], dy.sum(axis=0), np.abs(dy).sum(axis=0))}
    if inp.bn:
        xhat = ((inp.pre.astype(np.float32) - owned["bn_mean"]) * owned["bn_inv_std"]).astype(np.float64)      # the kernel's own two roundings
        sums["colsum_dyx"] = (out["colstats"][1], (dy * xhat).sum(axis=0), np.abs(dy * xhat).sum(axis=0))
    w = np.ones(B, np.float32) if inp.inst_w is None else inp.inst_w.astype(np.float32)
    wj = np.repeat(w[:, None], R, axis=1)
    if (not inp.bias_negative_samples) and inp.k > 1:
        w = w * np.float32((float(np.float32(inp.k)) + 1.0) / (2.0 * float(np.float32(inp.k))))
        wj = np.repeat(w[:, None], R, axis=1)
        wj[:, 0] = w * np.float32(inp.k)
    mass = np.log(owned["probs"].astype(np.float64)) * wj.astype(np.float64)
    sums["loss"] = (out["loss"], np.array([mass.sum()]), np.array([np.abs(mass).sum()]))
    for t, (g, want, mag) in sums.items():
        bound = t_add * mag
        err = np.abs(g - want)
        ratios[t] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        WORST[t] = max(WORST.get(t, 0.0), ratios[t])
    print("loss-shape %s B=%d de=%d R=%d: %s" % (plan_name(plan), B, de, R, " ".join("%s %.3f" % kv for kv in ratios.items())))
    bad = {t: r for t, r in ratios.items() if not r <= 1.0}
    assert not bad, (label, bad)


def check_case(B, de, R, bn, nl, seed, **opts):
    inp = make_inputs(B, de, R, bn, nl, seed, **opts)
    out, plan, left = run_loss(inp)
    label = "B=%d de=%d R=%d bn=%d nl=%d %s" % (B, de, R, bn, nl, opts)
    name, epw, grid = expected_plan(B, de, R, l2=opts.get("l2", False))
    assert (plan_name(plan), plan["epw"], plan["grid"]) == (name, epw, grid), label
    assert left == 0, label
    SEEN.add(plan_name(plan))
    check_elementwise(inp, out, plan, label)
    out3, plan3, left3 = run_loss(inp, repeats=3)
    assert plan3 == plan and left3 == 0
    same_bits(out, out3, label + ": three launches on one workspace against one")


# ---- the rows kernel ------------------------------------------------------------------------------------------------------------
# (R, B, de): every R, B and de of the table once per pass, large batches with few rows per example. Pass A runs with batch-norm and
# hard_tanh, pass B without batch-norm and with tanh: every value appears with batch-norm on and off and with both nonlinearities.
# Ragged batches (B no multiple of 4 · examples per wave) per (RB, row sets): (6, 1) 6145 / 5; (11, 1) 2049 / 65; (17, 1) 1025 / 2049;
# (17, 2) 65 / 1025; (17, 3) 5 / 4097; (17, 4) 3, 1 / 6145, 8193.
ROWS_A = [(1, 8193, 8), (2, 6145, 4), (6, 4097, 36), (7, 2049, 252), (11, 2047, 256), (12, 1025, 8), (17, 1024, 256), (18, 65, 252),
          (34, 64, 36), (35, 5, 4), (52, 3, 256), (64, 1, 252)]
ROWS_B = [(1, 3, 252), (2, 1, 256), (6, 5, 8), (7, 1024, 36), (11, 65, 4), (12, 64, 256), (17, 2049, 252), (18, 1025, 256),
          (34, 2047, 8), (35, 4097, 36), (52, 6145, 4), (64, 8193, 8)]


def _options(i):
    """Options that rotate over the cases of a pass: instance weights given / null, bias_negative_samples on / off."""
    return dict(inst_w=i % 2 == 0, bias_neg=i % 3 == 0)


@pytest.mark.parametrize("i", range(len(ROWS_A)), ids=["R%d-B%d-de%d" % c for c in ROWS_A])
def test_rows_kernel_batch_norm_hard_tanh(i):
    R, B, de = ROWS_A[i]
    check_case(B, de, R, True, 1, 1000 + i, const_col=(de - 1 if i % 2 else 0) if i % 4 < 2 else None, **_options(i))


@pytest.mark.parametrize("i", range(len(ROWS_B)), ids=["R%d-B%d-de%d" % c for c in ROWS_B])
def test_rows_kernel_plain_tanh(i):
    R, B, de = ROWS_B[i]
    check_case(B, de, R, False, 0, 2000 + i, **_options(i + 1))


# the other two pairings, the options, and the largest grid
ROWS_C = [
    dict(B=40961, de=4, R=6, bn=True, nl=0),                               # 20 examples per wave
    dict(B=40961, de=4, R=17, bn=False, nl=1, inst_w=False),
    dict(B=1025, de=252, R=18, bn=True, nl=0, dp=True, const_col=251),     # data parallel: statistics and 1 / B over 8 B rows
    dict(B=65, de=256, R=17, bn=False, nl=1, dp=True),
    dict(B=2049, de=36, R=11, bn=True, nl=1, clip=False),                  # clip_sigmoid off
    dict(B=64, de=8, R=35, bn=False, nl=0, clip=False, bias_neg=True),
    dict(B=1024, de=256, R=2, bn=True, nl=0, bias_neg=True),               # k = 1: nothing is rebalanced either way
    dict(B=1025, de=252, R=2, bn=False, nl=1, bias_neg=False, inst_w=False),
    dict(B=3, de=4, R=64, bn=True, nl=0, bias_neg=True),
    dict(B=6145, de=256, R=6, bn=False, nl=1),
]


@pytest.mark.parametrize("case", ROWS_C, ids=["-".join("%s%s" % kv for kv in c.items()) for c in ROWS_C])
def test_rows_kernel_options(case):
    c = dict(case)
    check_case(c.pop("B"), c.pop("de"), c.pop("R"), c.pop("bn"), c.pop("nl"), 3000 + len(case) + case["B"] % 89, **c)


# ---- the generic kernel ---------------------------------------------------------------------------------------------------------
GEN_DE = [1, 7, 63, 65, 66, 127, 129, 130, 254, 255, 260, 512, 516, 1020, 1024]
GEN_R, GEN_B = [1, 2, 17], [1, 33, 1025]


def _generic_cases(shift):
    return [(de, GEN_R[(i + shift) % 3], GEN_B[(i + i // 3 + 2 * shift) % 3]) for i, de in enumerate(GEN_DE)]


GEN_A, GEN_B_CASES = _generic_cases(0), _generic_cases(1)


@pytest.mark.parametrize("i", range(len(GEN_A)), ids=["de%d-R%d-B%d" % c for c in GEN_A])
def test_generic_kernel_batch_norm_hard_tanh(i):
    de, R, B = GEN_A[i]
    check_case(B, de, R, True, 1, 4000 + i, const_col=(de // 2 if i % 3 == 0 else None), **_options(i))


@pytest.mark.parametrize("i", range(len(GEN_B_CASES)), ids=["de%d-R%d-B%d" % c for c in GEN_B_CASES])
def test_generic_kernel_plain_tanh(i):
    de, R, B = GEN_B_CASES[i]
    check_case(B, de, R, False, 0, 5000 + i, **_options(i + 1))


GEN_C = [
    dict(B=33, de=8, R=65, bn=True, nl=0),                                 # the first R beyond the rows kernel
    dict(B=1025, de=8, R=65, bn=False, nl=1, bias_neg=True),
    dict(B=33, de=256, R=70, bn=False, nl=0, inst_w=False),
    dict(B=1025, de=256, R=70, bn=True, nl=1, dp=True),
    dict(B=1025, de=20, R=17, bn=True, nl=1, l2=True),                     # the entity normaliser: <4,1> <1,4> <4,2> ...
    dict(B=33, de=20, R=2, bn=False, nl=0, l2=True, inst_w=False),
    dict(B=33, de=130, R=17, bn=True, nl=0, l2=True, clip=False),
    dict(B=1025, de=130, R=2, bn=False, nl=1, l2=True),
    dict(B=1, de=260, R=17, bn=True, nl=1, l2=True, const_col=259),
    dict(B=1025, de=260, R=1, bn=False, nl=0, l2=True),
    dict(B=33, de=7, R=17, bn=True, nl=0, l2=True),                        # ... and <1,1> <1,2> <4,4>
    dict(B=33, de=66, R=2, bn=False, nl=1, l2=True),
    dict(B=33, de=516, R=17, bn=True, nl=1, l2=True),
    dict(B=1025, de=1020, R=2, bn=False, nl=1, clip=False, dp=True),
    dict(B=33, de=127, R=17, bn=False, nl=1, bias_neg=True, inst_w=False),
]


@pytest.mark.parametrize("case", GEN_C, ids=["-".join("%s%s" % kv for kv in c.items()) for c in GEN_C])
def test_generic_kernel_options(case):
    c = dict(case)
    check_case(c.pop("B"), c.pop("de"), c.pop("R"), c.pop("bn"), c.pop("nl"), 6000 + len(case) + case["de"], **c)


def test_the_case_table_covers_what_it_was_written_for():
    """Host only: every value of the table appears with batch-norm on and off and with both nonlinearities."""
    rows = [(R, B, de, True, 1) for R, B, de in ROWS_A] + [(R, B, de, False, 0) for R, B, de in ROWS_B] + \
           [(c["R"], c["B"], c["de"], c["bn"], c["nl"]) for c in ROWS_C]
    gen = [(R, B, de, True, 1) for de, R, B in GEN_A] + [(R, B, de, False, 0) for de, R, B in GEN_B_CASES] + \
          [(c["R"], c["B"], c["de"], c["bn"], c["nl"]) for c in GEN_C]

    def covered(cases, pos, values):
        for v in values:
            hit = [(c[3], c[4]) for c in cases if c[pos] == v]
            assert {b for b, _ in hit} == {True, False} and {n for _, n in hit} == {0, 1}, (pos, v, hit)
    covered(rows, 0, [1, 2, 6, 7, 11, 12, 17, 18, 34, 35, 52, 64])
    covered(rows, 1, [1, 3, 5, 64, 65, 1024, 1025, 2047, 2049, 4097, 6145, 8193])
    covered(rows, 2, [4, 8, 36, 252, 256])
    assert any(c[1] == 40961 and c[2] == 4 for c in rows)
    covered(gen, 0, GEN_R)
    covered(gen, 1, GEN_B)
    covered(gen, 2, GEN_DE)
    assert {(8, 65), (256, 70)} <= {(c[2], c[0]) for c in gen}
    assert {20, 130, 260} <= {c["de"] for c in GEN_C if c.get("l2")}
    for R, B, de, bn, nl in rows:
        assert expected_plan(B, de, R)[0].startswith("rows")
    for R, B, de, bn, nl in gen:
        assert expected_plan(B, de, R)[0].startswith("generic") or any(c.get("l2") and c["de"] == de for c in GEN_C)
    # each (RB, row sets) with a ragged batch
    ragged = set()
    for R, B, de, bn, nl in rows:
        name, epw, grid = expected_plan(B, de, R)
        rb = int(name[5:name.index(">")].split(",")[0])
        if B % (4 * epw):
            ragged.add((rb, (R + rb - 1) // rb))
    assert ragged >= {(6, 1), (11, 1), (17, 1), (17, 2), (17, 3), (17, 4)}, ragged


# ---- bit-exact identities -------------------------------------------------------------------------------------------------------
def lazy_view(rs, rows, now):
    """Stamps with lags from {0, 1, 63, 64, 65, 127, 128 (the most the factor ring allows)}, every lag used; factors near 1."""
    lags = np.array([0, 1, 63, 64, 65, 127, lr.LAZY_HISTORY])
    lag = lags[np.arange(rows) % lags.size]
    rs.shuffle(lag)
    decay = (1.0 - rs.uniform(1e-4, 3e-2, lr.LAZY_HISTORY)).astype(np.float32)
    return (now - lag).astype(np.int32), decay


def with_lazy(inp, stamp, decay, now):
    inp.stamp, inp.decay, inp.now = stamp, decay, now
    return inp


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("B", [1, 2, 3, 9, 2049, 4097, 40961])
@pytest.mark.parametrize("RB", [6, 11, 17])
def test_two_row_sets_return_the_bits_of_one(RB, B, lazy):
    """loss_rows_kernel<RB, LAZY, PIPE = true> - which the model launches only on a table beyond 256 MB - against PIPE = false on
    the same inputs: "the same statements: results are bit-identical" (loss_bn.hip). Waves with 0, 1, 2, 3 and 27 or more examples.
    At 40 961 examples the two forms walk 27 and 20 examples per wave: every per-example output has the same bits, the ordered
    sums add the same terms in another grouping and are held to each other within the bound of the sums above."""
    de = 4 if B == 40961 else (8 if RB != 17 else 252)
    R = RB if B % 2 else max(1, RB - 2)
    bn = (B + RB) % 2 == 0
    inp = make_inputs(B, de, R, bn, 1 if bn else 0, 7000 + B + RB, inst_w=B % 3 != 0)
    now = 300
    if lazy:
        with_lazy(inp, *lazy_view(np.random.RandomState(B + RB), ROWS, now), now)
    one, plan1, left1 = run_loss(inp)
    inp.rows_for_dispatch = PIPE_BYTES // (4 * de) + 1
    two, plan2, left2 = run_loss(inp)
    name1, epw1, grid1 = expected_plan(B, de, R, lazy=lazy)
    name2, epw2, grid2 = expected_plan(B, de, R, lazy=lazy, pipe=True)
    assert (plan_name(plan1), plan1["epw"], plan1["grid"]) == (name1, epw1, grid1)
    assert (plan_name(plan2), plan2["epw"], plan2["grid"]) == (name2, epw2, grid2) and plan2["pipe"] == 1 and plan1["pipe"] == 0
    assert left1 == 0 and left2 == 0
    SEEN.update((plan_name(plan1), plan_name(plan2)))
    if epw1 == epw2:
        same_bits(one, two, "two row sets against one")
    else:
        same_bits(one, two, "two row sets against one", skip=("loss", "colstats"))
        dy = one["dy"][:B].astype(np.float64)
        bound = (4 * epw1 + 2 + 4 * epw2 + 2) * U32 * np.abs(dy).sum(axis=0)
        assert np.all(np.abs(one["colstats"][0] - two["colstats"][0]) <= bound)
        assert is_ff(two["colstats"][2]) and np.all(np.isfinite(two["loss"]))
    three, plan3, left3 = run_loss(inp, repeats=3)
    assert left3 == 0
    same_bits(two, three, "three launches on one workspace against one")


@pytest.mark.parametrize("de", [8, 252, 256])
@pytest.mark.parametrize("R", [2, 17, 18, 64])
def test_lazy_rows_return_the_bits_of_an_eager_table(R, de):
    """A launch on the raw table with stamps against an eager launch on the table the host brought up to date in float32, factor by
    factor: the same bits in every output. `now` is no multiple of 128 (the ring is entered in its middle and wrapped), every lag of
    {0, 1, 63, 64, 65, 127, 128} is used, and the rows of an example's second to fourth set of 17 carry stamps of their own."""
    B, now = 37, 128 * 3 + 77
    bn = (R + de) % 2 == 0
    inp = make_inputs(B, de, R, bn, 1 if R % 2 else 0, 8000 + R + de)
    stamp, decay = lazy_view(np.random.RandomState(R * de), ROWS, now)
    raw = inp.E.copy()
    current = lr.rows_up_to_date(raw, stamp, decay, now)
    assert (current != raw).any(axis=1).sum() == (stamp < now).sum()
    inp.E = current
    eager, plan_e, left_e = run_loss(inp)
    inp.E = raw
    with_lazy(inp, stamp, decay, now)
    lazy, plan_l, left_l = run_loss(inp)
    assert plan_name(plan_e) == expected_plan(B, de, R)[0] and plan_name(plan_l) == expected_plan(B, de, R, lazy=True)[0]
    assert plan_l["lazy"] == 1 and plan_e["lazy"] == 0 and left_e == 0 and left_l == 0
    SEEN.update((plan_name(plan_e), plan_name(plan_l)))
    same_bits(eager, lazy, "lazy against eager")
    # and the lazy launch element by element against the restatement (which brings the rows up to date itself)
    check_elementwise(inp, lazy, plan_l, "lazy R=%d de=%d" % (R, de))


def test_hook_refuses_what_the_model_never_launches():
    inp = make_inputs(5, 7, 3, False, 0, 1)                    # the generic kernel reads the rows as they are
    stamp, decay = lazy_view(np.random.RandomState(1), ROWS, 200)
    with pytest.raises(ca.NvsmError) as e:
        run_loss(with_lazy(inp, stamp, decay, 200))
    assert e.value.status == 2
    for args in (dict(R=65), dict(l2=True)):
        inp = make_inputs(5, 8, args.get("R", 3), False, 0, 1, l2=args.get("l2", False))
        with pytest.raises(ca.NvsmError) as e:
            run_loss(with_lazy(inp, stamp, decay, 200))
        assert e.value.status == 2
    inp = make_inputs(5, 8, 3, False, 0, 1)
    for wrong in (200 - 129, 201, -1):                          # one update too far behind, ahead of the table, negative
        s2 = stamp.copy()
        s2[11] = wrong
        with pytest.raises(ca.NvsmError) as e:
            run_loss(with_lazy(inp, s2, decay, 200))
        assert e.value.status == 1
    s2 = stamp.copy()
    s2[11] = 200 - 128
    run_loss(with_lazy(inp, s2, decay, 200))


@pytest.mark.parametrize("name,B", [("lse", 256), ("tiny_odd", 100)])
def test_hook_returns_the_bits_of_the_model(name, B):
    """(de 256, R 17, B 256) on the rows kernel and (de 7, R 4, B 100) on the generic one, no batch-norm: a handle's compute_cost and
    compute_gradients, then the handle's own pre, parameters, ids and weights through the hook - the hook launches what the model
    launches, with the constants the model hands it."""
    spec = SPECS[name]
    assert not spec.get("batch_norm")
    de, R = spec["entity_dim"], spec["num_random"] + 1
    rs = np.random.RandomState(41)
    params = random_params(spec, rs)
    g = gpu_model(spec, B)
    load_params(g, params, True)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    g.compute_cost(ca.Batch(words, labels, ww, iw), ids)
    g.compute_gradients()
    pre = g.get_tensor("pre").reshape(B, de)
    inp = lr.LossInputs(pre=pre, E=g.get_param(PARAMS[1]).reshape(-1, de), ids=ids.reshape(B, R), inst_w=iw,
                        nonlinearity=1 if spec["nonlinearity"] == "hard_tanh" else 0, clip_sigmoid=spec.get("clip_sigmoid", True),
                        bias_negative_samples=spec.get("bias_negative_samples", False))
    out, plan, left = run_loss(inp)
    assert plan_name(plan) == expected_plan(B, de, R)[0] and left == 0
    for mine, theirs in (("proj", "proj"), ("probs", "probs"), ("coef", "multipliers"), ("dy", "grad_proj")):
        a, b = out[mine][:B].ravel(), g.get_tensor(theirs)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (mine, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def test_every_instantiation_was_launched():
    """Every kernel launch_loss can pick was launched by the cases above, by the plan the hook reported."""
    want = {"rows<%d%s%s>" % (rb, lz, pp) for rb in (6, 11, 17) for lz in ("", ",lazy") for pp in ("", ",pipe")}
    want |= {"generic<%d,%d%s>" % (v, n, l2) for v in (1, 4) for n in (1, 2, 4) for l2 in ("", ",l2e")}
    assert len(want) == 24
    if SEEN:                                                       # (empty when this test is selected on its own)
        assert want <= SEEN, sorted(want - SEEN)
        print("loss-shape worst |g - ref| / bound per tensor: " + " ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
