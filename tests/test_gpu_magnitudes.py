"""-m gpu: batch-norm statistics and the loss clamps at the magnitudes of a trained model, against the fp64 oracle.

Every other GPU test starts from initial-scale parameters (tests/helpers.py random_params): a batch-norm column's mean is about
its spread and every logit is a few units. Trained models leave both ranges, and two parts of the hot path behave differently
outside them.

1. Batch-norm columns with an offset. Every word row is u + noise for one fixed direction u, the phrases are unweighted means,
   so every row of pre carries T·u. u is scaled so that the median over columns of r = |column mean| / column std, taken from
   the fp64 oracle's pre, is 0, 10, 100 or 1 000. Three further columns are constant (0.3, 3.7 and 0): their variance is 0, so
   1/sqrt(σ² + ε) must come out as 1/sqrt(ε) and proj as the nonlinearity of β. Every product that writes the column sums
   (gemm_f32_mfma, gemm_rsplit, gemm_split, gemm_rows, gemm_tstat) takes one step against the oracle; the dispatch is asserted
   first. The statistics are formed from [Σx | Σx²]: summed in fp32 as they stand, E[x²] − E[x]² loses about eps · r² of the
   variance, which this is built to catch.
2. A saturated loss. The document rows are scaled so that the logits cover about [−25, 25] and each of the five regions of the
   reference's sigmoid — value clamp, derivative cut, interior, derivative cut, value clamp — holds at least 1 % of the entries.
   Both loss kernels (rows, generic) compare probs and the multipliers elementwise. Near a threshold fp32 p and fp64 p can fall
   on different sides of it, so a band of logit around each threshold is compared with the fp32 oracle instead, which rounds p
   the way the GPU does; at most a handful of band entries may disagree with it.

Where fp32 rounding of pre (or of a logit) bounds what any fp32 path can reach, the yardstick is K_F32 times the fp32 oracle's
own distance from fp64.
"""
import numpy as np
import pytest

import cunvsm_amd as ca
from oracle import nvsm_oracle as orc
from tests.helpers import PARAMS, gpu_model, load_params, oracle_model, random_batch, random_params, rel_err
from tests.test_gpu_dispatch import FAMILIES, FWD, LOSS, fields

FWD_TOL, GRAD_TOL, UPD_TOL = 2e-5, 2e-4, 2e-4          # = tests/test_gpu_parity.py
K_F32 = 4.0                                            # at most this many times the fp32 oracle's distance from fp64
BN_EPS = 1e-4
CONST_VALUES = (0.3, 3.7, 0.0)


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _gpu_present(), reason="needs an MI355X")]


def within(err, err_f32, bound):
    return err <= bound or err <= K_F32 * err_f32


# ---------------------------------------------------------------------------------------------
# 1. batch-norm at column offsets
# ---------------------------------------------------------------------------------------------
def _spec(fam, **kw):
    return dict(FAMILIES[fam], **kw)


def _bn_spec(fam, **kw):
    # tanh rather than hard_tanh: after batch-norm a third of hard_tanh's units sit on its bound, and a unit within fp32 roundoff
    # of it sends its derivative the other way on any fp32 path (test_gpu_dispatch.py fp32_yardstick) — a smooth nonlinearity
    # keeps the gradients' comparison about the statistics
    return dict(FAMILIES[fam], nonlinearity="tanh", **kw)


# (case id, spec, batch, NVSM_GEMM_SPLIT=0, the forward product describe() must name)
BN_CASES = [
    ("f32-nvsm-B256", _bn_spec("nvsm"), 256, False, "f32"),
    ("f32-de512-B512", _bn_spec("wide"), 512, False, "f32"),
    ("f32-odd-B2048", _bn_spec("odd", batch_norm=True), 2048, False, "f32"),
    ("rsplit-nvsm-B1024", _bn_spec("nvsm"), 1024, False, "rsplit"),
    ("rsplit-nvsm-B8192", _bn_spec("nvsm"), 8192, False, "rsplit"),
    ("split-nvsm-B8193", _bn_spec("nvsm"), 8193, False, "split"),
    ("split-nvsm-B16384", _bn_spec("nvsm"), 16384, False, "split"),
    ("rows-de128-B4096", _bn_spec("de128"), 4096, False, "rows"),
    ("rows-nvsm-B4096", _bn_spec("nvsm"), 4096, True, "rows"),
    ("tstat-de128-B16384", _bn_spec("de128"), 16384, False, "tstat"),
    ("tstat-de512-B2048", _bn_spec("wide"), 2048, False, "tstat"),
    ("tstat-nvsm-B16383", _bn_spec("nvsm"), 16383, True, "tstat"),
]
OFFSETS = [0, 10, 100, 1000]
METHODS = ["sgd", "adagrad", "sparse_adam", "full_adam"]


def offset_problem(spec, B, target, seed):
    """Parameters and a batch whose pre has median column offset r = target (see the module docstring), plus the indices of
    the constant columns. Returns (params, batch, const_cols, other_cols)."""
    rs = np.random.RandomState(seed)
    nV, dw, de = spec["num_words"], spec["word_dim"], spec["entity_dim"]
    params = random_params(spec, rs)
    T = params[PARAMS[2]].astype(np.float64).reshape(dw, de).T.copy()      # (stored [d_w][d_e]: pre = phrase · T)
    W = params[PARAMS[0]].astype(np.float64).reshape(nV, dw)
    k0 = dw - 1                                            # the coordinate the constant columns read
    const = np.array([1, de // 2, de - 2])
    other = np.setdiff1d(np.arange(de), const)
    T[:, k0] = 0.0
    for c, v in zip(const, CONST_VALUES):
        T[c, :] = 0.0
        T[c, k0] = v
    W[:, k0] = 1.0                                         # (a mean of ones is exactly one in fp32 too)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    ww = np.ones_like(ww)
    alpha, u = 0.0, np.zeros(dw)
    if target > 0:
        # u: T u = ± 1 on the other columns (least squares where d_w is too narrow), then scaled to the target median r
        sgn = rs.choice([-1.0, 1.0], other.size)
        u[:k0] = np.linalg.lstsq(T[np.ix_(other, np.arange(k0))], sgn, rcond=None)[0]
        u /= np.linalg.norm(u)
        pn = W[words.reshape(B, -1)].mean(axis=1) @ T[other].T
        off, mu, sd = T[other] @ u, pn.mean(axis=0), pn.std(axis=0)
        lo, hi = 0.0, 1.0
        while np.median(np.abs(hi * off + mu) / sd) < target:
            hi *= 2.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if np.median(np.abs(mid * off + mu) / sd) < target else (lo, mid)
        alpha = 0.5 * (lo + hi)
    W += alpha * u[None, :]
    W[:, k0] = 1.0
    params[PARAMS[0]] = W.ravel().astype(np.float32)
    params[PARAMS[2]] = T.T.ravel().astype(np.float32)
    return params, (words, ww, labels, iw, ids), const, other


def column_offsets(pre, cols):
    p = pre[:, cols]
    return np.abs(p.mean(axis=0)) / p.std(axis=0)


def check_step(spec, B, params, batch, const=None, other=None, target=None):
    """One compute_cost / compute_gradients / update, HIP against the fp64 oracle with the fp32 oracle as yardstick; with
    `target`, the achieved column offsets first; with `const`, the constant columns exactly."""
    words, ww, labels, iw, ids = batch
    o, o32, g = oracle_model(spec), oracle_model(spec, orc.F32), gpu_model(spec, B)
    load_params(o, params, False)
    load_params(o32, params, False)
    load_params(g, params, True)
    de = spec["entity_dim"]
    errs = {}
    for m in (o, o32):
        m.forward(words, ww, ids, iw)
    g.compute_cost(ca.Batch(words, labels, ww, iw), ids)
    if target:
        # (where d_w covers every column, T u = ±1 is solved exactly and no column escapes the offset)
        r = column_offsets(o.get("pre").reshape(B, de), other)
        assert 0.8 * target <= np.median(r) <= 1.25 * target, (target, np.median(r))
        assert spec["word_dim"] - 1 < other.size or r.min() >= 0.3 * target, (target, r.min())
    co, co32, cg = o.get_cost(), o32.get_cost(), g.get_cost()
    assert within(abs(cg - co), abs(co32 - co), FWD_TOL * abs(co)), (cg, co, co32)
    for t in ("pre", "proj", "probs", "bn_mean", "bn_inv_std"):
        if t.startswith("bn_") and not spec.get("batch_norm"):
            continue
        errs[t] = (rel_err(g.get_tensor(t), o.get(t)), rel_err(o32.get(t), o.get(t)))
        assert within(errs[t][0], errs[t][1], FWD_TOL), (t, errs[t])
    if const is not None:
        inv, mean = g.get_tensor("bn_inv_std"), g.get_tensor("bn_mean")
        pre = g.get_tensor("pre").reshape(B, de)
        proj = g.get_tensor("proj").reshape(B, de)
        beta = params[PARAMS[3]]
        act = (lambda x: np.clip(x, -1.0, 1.0)) if spec["nonlinearity"] == "hard_tanh" else np.tanh
        for c, v in zip(const, CONST_VALUES):
            assert np.all(pre[:, c] == pre[0, c]), (c, v)
            assert mean[c] == pre[0, c], (c, v, mean[c], pre[0, c])
            assert abs(inv[c] * np.sqrt(BN_EPS) - 1.0) <= 1e-6, (c, v, inv[c], 1 / np.sqrt(BN_EPS))
            np.testing.assert_allclose(proj[:, c], act(np.float64(beta[c])), rtol=0, atol=1e-6, err_msg="column %d (%g)" % (c, v))
    for m in (o, o32):
        m.backward()
    g.compute_gradients()
    R = spec["num_random"] + 1
    sign = np.where(np.arange(B * R) % R == 0, 1.0, -1.0)
    for t in ("multipliers", "grad_proj", "grad_bias", "grad_transform", "grad_phrase"):
        a, b, c = g.get_tensor(t), o.get(t), o32.get(t)
        if t == "multipliers":
            b, c = b * sign, c * sign
        errs[t] = (rel_err(a, b), rel_err(c, b))
        assert within(errs[t][0], errs[t][1], GRAD_TOL), (t, errs[t])
    lr = {"sgd": 0.1, "adagrad": 0.01}.get(spec.get("update_method", "sgd"), 1e-3)
    for m in (o, o32):
        m.update(lr)
    g.update(lr)
    for p in PARAMS:
        new_o = o.get(p)
        delta = np.linalg.norm(new_o - params[p].astype(np.float64))
        err = np.linalg.norm(g.get_param(p).astype(np.float64) - new_o)
        err32 = np.linalg.norm(np.asarray(o32.get(p), np.float64) - new_o)
        floor = 1e-7 * np.linalg.norm(new_o)
        errs[p] = (err / max(delta, 1e-30), err32 / max(delta, 1e-30))
        assert within(err, err32 + floor, UPD_TOL * max(delta, 1e-12) + floor), (p, errs[p])


BN_MATRIX = [(c, r) for c in BN_CASES for r in OFFSETS]


@pytest.mark.parametrize("case,target", BN_MATRIX, ids=["%s-r%d" % (c[0], r) for c, r in BN_MATRIX])
def test_batch_norm_at_column_offsets(case, target, monkeypatch):
    name, spec, B, no_split, product = case
    if no_split:
        monkeypatch.setenv("NVSM_GEMM_SPLIT", "0")
    method = METHODS[(BN_CASES.index(case) + OFFSETS.index(target)) % len(METHODS)]
    spec = dict(spec, update_method=method)
    params, batch, const, other = offset_problem(spec, B, target, seed=B + target + len(name))
    desc = gpu_model(spec, B).describe(B)
    assert fields(desc)["forward"].startswith(FWD[product]), (product, desc)
    check_step(spec, B, params, batch, const, other, target)


def test_fused_steps_from_offset_parameters():
    """Five fused steps (step / step_deferred) with sparse Adam at B = 6 400 from parameters with column offset r = 100: the
    statistics of every step come from the projection product of that step, on a handle loaded by set_param."""
    spec = dict(FAMILIES["nvsm"], update_method="sparse_adam", nonlinearity="tanh")
    B, steps, lr = 6400, 5, 1e-3
    params, first, _, _ = offset_problem(spec, B, 100, seed=64)
    rs = np.random.RandomState(65)
    batches = [first]
    for _ in range(steps - 1):
        w, ww, l, iw, ids = random_batch(spec, rs, B, zipf=True)
        batches.append((w, np.ones_like(ww), l, iw, ids))
    o, o32, g = oracle_model(spec), oracle_model(spec, orc.F32), gpu_model(spec, B)
    load_params(o, params, False)
    load_params(o32, params, False)
    load_params(g, params, True)
    assert fields(g.describe(B))["forward"].startswith(FWD["rsplit"])
    tickets = [g.step_deferred(ca.Batch(w, l, ww, iw), lr, entity_ids=ids) for (w, ww, l, iw, ids) in batches[:2]]
    costs = [g.deferred_cost(t) for t in tickets]
    for w, ww, l, iw, ids in batches[2:]:
        costs.append(g.step(ca.Batch(w, l, ww, iw), lr, entity_ids=ids, want_cost=True))
    for s, (w, ww, l, iw, ids) in enumerate(batches):
        for m in (o, o32):
            m.forward(w, ww, ids, iw)
        if s == 0:
            co, co32 = o.get_cost(), o32.get_cost()
            assert within(abs(costs[0] - co), abs(co32 - co), FWD_TOL * abs(co)), (costs[0], co, co32)
        for m in (o, o32):
            m.backward()
            m.update(lr)
    for n in PARAMS:                                   # (= test_one_handle_across_regimes: 5e-3 of the change for Adam)
        new_o, old = o.get(n), params[n].astype(np.float64)
        change = np.linalg.norm(new_o - old)
        err = np.linalg.norm(g.get_param(n).astype(np.float64) - new_o)
        err32 = np.linalg.norm(np.asarray(o32.get(n), np.float64) - new_o)
        floor = 1e-7 * np.linalg.norm(old)
        assert within(err, err32 + floor, 5e-3 * change + floor), (n, err / change, err32 / change)


# ---------------------------------------------------------------------------------------------
# 2. the saturated loss
# ---------------------------------------------------------------------------------------------
T_CUT, T_CLAMP = 13.8155, 16.1181                      # σ(s) = 1 − 1e-6, 1 − 1e-7 (and 1e-6, 1e-7 at −s)
# Band of logit around a threshold where fp32 and fp64 p may fall on different sides of it: near 1, fp32 p is spaced 6e-8
# apart — 0.06 of logit at 1 − 1e-6 and 0.6 at 1 − 1e-7; near 0 fp32 p is relatively exact and only the logit's own
# rounding counts. (Comparing p with 1 − 1e-6 in float instead of double changes nothing on this path: 1 / (1 + e^−s) in fp32
# only reaches EVEN multiples of 2^-24 below 1, and the float nearest 1 − 1e-6 is 1 − 17 · 2^-24.)
BANDS = [(-T_CLAMP, 0.1), (-T_CUT, 0.1), (T_CUT, 0.1), (T_CLAMP, 0.7)]

LOSS_CASES = [
    ("rows-nvsm", _spec("nvsm"), 4096, "rows"),
    ("rows-nvsm-biasneg", _spec("nvsm", bias_negative_samples=True), 4096, "rows"),
    ("rows-lse", _spec("lse"), 4096, "rows"),
    ("generic-odd", _spec("odd"), 2048, "generic"),
    ("generic-de512", _spec("wide"), 2048, "generic"),
    ("generic-de512-biasneg", _spec("wide", bias_negative_samples=True), 2048, "generic"),
]


def signed_logits(o, params, spec, ids, B):
    de, R = spec["entity_dim"], spec["num_random"] + 1
    E = params[PARAMS[1]].astype(np.float64).reshape(-1, de)
    proj = o.get("proj").reshape(B, de)
    s = np.einsum("bt,brt->br", proj, E[ids.reshape(B, R)])
    s[:, 1:] *= -1.0
    return s.ravel()


def saturated_problem(spec, B, seed, spread):
    """Initial-scale parameters with the document rows scaled so that the fp64 logits have standard deviation `spread`."""
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    batch = random_batch(spec, rs, B, zipf=True)
    words, ww, labels, iw, ids = batch
    o = oracle_model(spec)
    load_params(o, params, False)
    o.forward(words, ww, ids, iw)
    s = signed_logits(o, params, spec, ids, B)
    params[PARAMS[1]] = (params[PARAMS[1]].astype(np.float64) * (spread / s.std())).astype(np.float32)
    return params, batch


def check_saturated(spec, B, params, batch, clip=True):
    words, ww, labels, iw, ids = batch
    o, o32, g = oracle_model(spec), oracle_model(spec, orc.F32), gpu_model(spec, B)
    load_params(o, params, False)
    load_params(o32, params, False)
    load_params(g, params, True)
    desc = g.describe(B)
    for m in (o, o32):
        m.forward(words, ww, ids, iw)
    g.compute_cost(ca.Batch(words, labels, ww, iw), ids)
    s = signed_logits(o, params, spec, ids, B)
    band = np.zeros(s.size, bool)
    if clip:
        for t, w in BANDS:
            band |= np.abs(s - t) < w
    # probs: the clamp constants exactly where the oracle clamps; elsewhere within the fp32 oracle's largest distance
    pg, po, p32 = g.get_tensor("probs").astype(np.float64), o.get("probs"), o32.get("probs")
    if clip:
        lo_c, hi_c = (s < -T_CLAMP) & ~band, (s > T_CLAMP) & ~band
        assert np.all(pg[lo_c] == np.float32(1e-7)), np.unique(pg[lo_c])[:8]
        assert np.all(pg[hi_c] == np.float32(1.0 - 1e-7)), np.unique(pg[hi_c])[:8]
    dmax32 = np.abs(p32 - po).max()
    bad = np.abs(pg - po) > K_F32 * dmax32 + 1e-7
    assert not bad.any(), (bad.sum(), s[bad][:8], pg[bad][:8], po[bad][:8], dmax32)
    co, co32, cg = o.get_cost(), o32.get_cost(), g.get_cost()
    assert within(abs(cg - co), abs(co32 - co), FWD_TOL * abs(co)), (cg, co, co32)
    for m in (o, o32):
        m.backward()
    g.compute_gradients()
    R = spec["num_random"] + 1
    sign = np.where(np.arange(B * R) % R == 0, 1.0, -1.0)
    mg, mo, m32 = g.get_tensor("multipliers").astype(np.float64), o.get("multipliers") * sign, o32.get("multipliers") * sign
    out = ~band
    # outside the band: the derivative cut and the value clamp give exact zeros, the interior follows fp64
    if clip:
        flip = (mg[out] == 0) != (mo[out] == 0)
        assert not flip.any(), (flip.sum(), s[out][flip][:8])
    dm32 = np.abs(m32[out] - mo[out]).max()
    scale = np.abs(mo).max()
    bad = np.abs(mg[out] - mo[out]) > K_F32 * dm32 + 1e-6 * scale
    assert not bad.any(), (bad.sum(), s[out][bad][:8], mg[out][bad][:8], mo[out][bad][:8])
    # inside the band: the fp32 oracle's rounding of p decides; a handful may fall the other way (a one-ulp different logit)
    disagree = np.flatnonzero(band & ((mg == 0) != (m32 == 0)))
    print("band entries %d, disagreeing with the fp32 oracle %d: logits %s" % (band.sum(), disagree.size, s[disagree][:8]))
    assert disagree.size <= 3, (disagree.size, s[disagree][:8], mg[disagree][:8], m32[disagree][:8])
    both = band & (mg != 0) & (m32 != 0)
    assert np.all(np.abs(mg[both] - m32[both]) <= K_F32 * dm32 + 1e-6 * scale)
    for t in ("grad_proj", "grad_bias", "grad_transform", "grad_phrase", "grad_entity"):
        a, b, c = g.get_tensor(t), o.get(t), o32.get(t)
        assert within(rel_err(a, b), rel_err(c, b), GRAD_TOL), (t, rel_err(a, b), rel_err(c, b))
    return desc, s


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_saturated_loss_regions(case):
    name, spec, B, kernel = case
    params, batch = saturated_problem(spec, B, seed=B + len(name), spread=12.0)
    desc, s = check_saturated(spec, B, params, batch)
    assert fields(desc)["loss"].startswith(LOSS[kernel]), (kernel, desc)
    n = s.size
    regions = [s < -T_CLAMP, (s >= -T_CLAMP) & (s <= -T_CUT), np.abs(s) < T_CUT, (s >= T_CUT) & (s < T_CLAMP), s >= T_CLAMP]
    share = [r.sum() / n for r in regions]
    assert min(share) >= 0.01, share


def test_unclipped_sigmoid_at_large_logits():
    """clip_sigmoid = 0: no clamp and no derivative cut; |logit| <= 60 stays clear of fp32 underflow of exp."""
    spec = _spec("nvsm", clip_sigmoid=False)
    B = 2048
    params, batch = saturated_problem(spec, B, seed=5, spread=12.0)
    desc, s = check_saturated(spec, B, params, batch, clip=False)
    assert np.abs(s).max() <= 60.0, np.abs(s).max()
    assert np.mean(np.abs(s) > T_CLAMP) >= 0.05
