"""The contract of the fused loss kernels (csrc/loss_bn.hip:97-108, the constants of kernels.h fill_loss_consts) in numpy: what
nvsm_debug_loss must return for its inputs, in the floating-point type asked for. float64 is the reference the kernels are held to,
float32 the yardstick: what a plain float32 evaluation of the same formulas loses against float64.

It is trusted only through tests/test_loss_reference.py, which holds it to the pinned oracle (oracle/nvsm_oracle.hpp) element by
element. The formulas are the oracle's, statement by statement; the one thing the oracle does not have is the lazy view, whose rows
are brought up to date first, in float32, factor by factor, in update order - the roundings of the dense passes (kernels.h "lazy
dense decay")."""
import numpy as np

BN_EPS = 1e-4               # objective.cu:114
LAZY_HISTORY = 128          # kernels.h kLazyHistory
CHUNK_ELEMENTS = 1 << 22    # gathered rows held at once: [examples of a chunk][R][de]


class LossInputs:
    """The inputs of nvsm_debug_loss. Arrays keep the type they are given in (the oracle test hands over float64)."""

    def __init__(self, pre, E, ids, k=None, bn=False, bn_sums=None, bn_n=None, bias=None, inst_w=None, nonlinearity=0,
                 clip_sigmoid=True, bias_negative_samples=False, l2_entity=False, b_global=None, stamp=None, decay=None, now=0,
                 rows_for_dispatch=0):
        self.pre = np.ascontiguousarray(pre)
        self.B, self.de = self.pre.shape
        self.E = np.ascontiguousarray(E)
        self.rows = self.E.shape[0]
        self.ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(self.B, -1)
        self.R = self.ids.shape[1]
        self.k = self.R - 1 if k is None else k
        self.bn = bool(bn)
        self.bn_sums = None if bn_sums is None else np.ascontiguousarray(bn_sums, dtype=np.float64).reshape(2, self.de)
        self.bn_n = float(self.B if bn_n is None else bn_n)
        self.bias = None if bias is None else np.ascontiguousarray(bias)
        self.inst_w = None if inst_w is None else np.ascontiguousarray(inst_w)
        self.nonlinearity = int(nonlinearity)      # 0 tanh, 1 hard_tanh
        self.clip_sigmoid = bool(clip_sigmoid)
        self.bias_negative_samples = bool(bias_negative_samples)
        self.l2_entity = bool(l2_entity)
        self.b_global = float(self.B if b_global is None else b_global)
        self.stamp = None if stamp is None else np.ascontiguousarray(stamp, dtype=np.int32)
        self.decay = None if decay is None else np.ascontiguousarray(decay, dtype=np.float32)
        self.now = int(now)
        self.rows_for_dispatch = int(rows_for_dispatch)
        assert self.ids.min() >= 0 and self.ids.max() < self.rows


def column_sums(x):
    """[2][de] float64: the sums of the columns of x and of their squares, as the projection product's epilogue leaves them."""
    x = np.asarray(x, np.float64)
    return np.stack([x.sum(axis=0), (x * x).sum(axis=0)])


def rows_up_to_date(E, stamp, decay, now):
    """Row r of a lazily decayed table has had stamp[r] of the table's `now` updates applied: the factors of the others, one by one
    in update order, each product rounded to float32 (the factor of update u + 1 sits at decay[u % 128])."""
    E = np.array(E, dtype=np.float32)
    stamp = np.asarray(stamp)
    assert E.dtype == np.float32 and decay.dtype == np.float32 and decay.size == LAZY_HISTORY
    assert stamp.min() >= 0 and stamp.max() <= now and now - stamp.min() <= LAZY_HISTORY
    for u in range(int(stamp.min()), now):
        behind = stamp <= u
        E[behind] = E[behind] * decay[u % LAZY_HISTORY]
    return E


def loss_reference(inp, dtype):
    """dict of proj [B][de], pp [B], probs, coef (the signed multipliers) [B][R], dy [B][de], colsum_dy, colsum_dyx [de] (float64
    sums of this evaluation's own dy and dy * xhat), bn_mean, bn_inv_std [de], loss (float64 sum of this evaluation's weighted log
    probabilities), logits [B][R] (signed) and act_in [B][de] (what the nonlinearity is applied to)."""
    F = np.dtype(dtype).type
    B, de, R, k = inp.B, inp.de, inp.R, inp.k
    x = inp.pre.astype(F)
    E = inp.E if inp.stamp is None else rows_up_to_date(inp.E, inp.stamp, inp.decay, inp.now)
    E = E.astype(F)

    # batch statistics from the column sums, in double whatever the type (cudnn_utils.cu:107-124: biased variance)
    mean, inv_std = np.zeros(de, F), np.ones(de, F)
    xhat = np.zeros((B, de), F)
    y = x
    if inp.bn:
        m = inp.bn_sums[0] / inp.bn_n
        var = np.maximum(inp.bn_sums[1] / inp.bn_n - m * m, 0.0)
        mean = m.astype(F)
        inv_std = (1.0 / np.sqrt(var + float(F(BN_EPS)))).astype(F)
        xhat = (x - mean) * inv_std
        y = xhat + inp.bias.astype(F)
    act_in = y
    lo, hi = np.nextafter(F(-1), F(-2)), np.nextafter(F(1), F(2))      # cuda_utils.h:91-96: the bounds widened by one step
    proj = np.tanh(y) if inp.nonlinearity == 0 else np.minimum(np.maximum(y, lo), hi)
    if F is np.float32:
        pp = (proj * proj).sum(axis=1, dtype=F) * F(np.exp(-np.log(float(de))))      # updates_adam.cu:238-240
    else:
        pp = (proj * proj).sum(axis=1) / de

    # instance weights (objective.cu:268-290)
    w = np.ones(B, F) if inp.inst_w is None else inp.inst_w.astype(F)
    rebalance = (not inp.bias_negative_samples) and k > 1
    if rebalance:
        w = w * F((float(F(k)) + 1.0) / (2.0 * float(F(k))))
    wj = np.repeat(w[:, None], R, axis=1)
    if rebalance:
        wj[:, 0] = w * F(k)
    sig_eps = F(1e-7) if inp.clip_sigmoid else F(0)
    sig_hi = F(1.0 - float(sig_eps))
    d_eps = F(1e-6) if inp.clip_sigmoid else F(0)
    d_hi = 1.0 - float(d_eps)
    inv_batch = F(np.exp(-np.log(inp.b_global)))
    sign = np.where(np.arange(R) == 0, F(1), F(-1))

    logits, probs, coef, gp = np.empty((B, R), F), np.empty((B, R), F), np.empty((B, R), F), np.empty((B, de), F)
    step = max(1, CHUNK_ELEMENTS // (R * de))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        e = E[inp.ids[sl]]                                               # [n][R][de]
        if inp.l2_entity:                                                # objective.cu:168-174
            e = e / np.sqrt((e * e).sum(axis=2, dtype=F))[:, :, None]
        s = np.einsum("bt,brt->br", proj[sl], e) * sign                  # :184-239
        with np.errstate(over="ignore"):
            p = np.where(s >= 0, 1 / (1 + np.exp(-s)), np.exp(s) / (1 + np.exp(s))).astype(F)      # cuda_utils.h:205-207
        p = np.minimum(np.maximum(p, sig_eps), sig_hi)
        d = np.where((p.astype(np.float64) >= d_hi) | (p <= d_eps), F(0), F(1) - p)                # :229-231
        c = sign * (wj[sl] * (d * inv_batch))                            # objective.cu:357-371, :398-401
        logits[sl], probs[sl], coef[sl] = s, p, c
        gp[sl] = np.einsum("br,brt->bt", c, e)                           # :420-425
    mass = np.log(probs) * wj                                            # :250-305
    dd = (F(1) - proj * proj) if inp.nonlinearity == 0 else ((proj > lo) & (proj < hi)).astype(F)      # params.cu:474-491
    dy = dd * gp
    dy64 = dy.astype(np.float64)
    return dict(proj=proj, pp=pp.astype(F), probs=probs, coef=coef, dy=dy, bn_mean=mean, bn_inv_std=inv_std,
                colsum_dy=dy64.sum(axis=0), colsum_dyx=(dy64 * xhat.astype(np.float64)).sum(axis=0),
                loss=float(mass.astype(np.float64).sum()), logits=logits, act_in=act_in, xhat=xhat, mass=mass)


def bn_backward(ref, inp):
    """The batch-norm backward the model runs behind the loss kernel (cudnn_utils.cu:158-177), in float64 on a reference's own dy and
    column sums: dx = 1/σ · (dy − (Σdy + x̂ · Σdy·x̂) / N)."""
    dy, xhat = ref["dy"].astype(np.float64), ref["xhat"].astype(np.float64)
    return ref["bn_inv_std"].astype(np.float64) * (dy - (ref["colsum_dy"] + xhat * ref["colsum_dyx"]) / inp.bn_n)
