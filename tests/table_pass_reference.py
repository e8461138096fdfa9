"""Plain numpy restatement of ONE table pass of the update (csrc/update.hip: CSR build, chunk tree, row formulas), and the cases
tests/test_gpu_table_pass.py runs through nvsm_debug_table_pass. No GPU, no library: tests/test_table_pass_reference.py checks
this file against itself in float64 on any machine.

Why the reference has no tolerance. X is drawn from the integers -4 .. 4, the per-entry coefficients from {±0.5, ±1, ±2}, sq_src
from {0.25, 0.5, 1} and src_scale from {0.5, 1, 2}: every term of a row's gradient sum g is a multiple of 1/4 (1/2 without
src_scale) of magnitude <= 16 and every term of its scalar q a multiple of 1/16 of magnitude <= 4, so for rows of up to 65 537
entries every partial sum - in any order, under any chunking, fused multiply-add or not - is an integer below 2^24 in units of its
granularity and therefore exact in float32 (Case.exactness() computes the margin from the case's own arrays). g and q of every row
equal the sums computed here in float64, which are exact for the same reason; an entry that is dropped, counted twice or given to
another row moves g by at least 1/4 whatever the row's length. The row formulas are then restated operation by operation in
np.float32 - one rounding per operation, in the kernel's order (apply_row_formula_sc is compiled with fp contract off).

Lazy decay (tests/test_gpu_lazy_rows.py). A case with `lags` is a pass over a lazily decayed table (csrc/kernels.h "lazy dense
decay"): row r has had stamp[r] = now - lags[r] updates applied, the table `now`, and ring[u % 128] holds the factor of update
u + 1. The rows WITH entries first get the factors they sat out - refresh32: one float32 rounding per factor, ascending u; m by
the constant S_M; the per-row scalar by scalar32 -, then the row formula above; rows without entries keep every bit and their
stamp, the rows with entries are stamped now + 1. The factors are 1 - uniform(1e-4, 3e-2), all distinct, so that a wrong ring slot
moves the result by at least 1e-4 relative, four thousand ulps (test_table_pass_reference.py asserts that every stale row of
every case would show it)."""
import numpy as np

F32 = np.float32
K_FAN = 32
CHUNK, CHUNK_SMALL, CHUNK_SMALL_MAX_ENTRIES = 64, 32, 131072
SGD, ADAGRAD_ENT, ADAM_MV, ADAM_SPARSE_ENT, ADAM_DENSE, ADAM_FULL, SCALAR_ACC = range(7)      # RowKind (csrc/kernels.h)
KIND_NAMES = ["sgd", "adagrad_ent", "adam_mv", "adam_sparse_ent", "adam_dense", "adam_full", "scalar_acc"]
PATH_DENSE, PATH_LIST_WALK, PATH_ENTRY_WALK = 0, 1, 2      # TablePassPath
USES_M = (ADAM_MV, ADAM_SPARSE_ENT, ADAM_DENSE, ADAM_FULL)
USES_P = (SGD, ADAGRAD_ENT, ADAM_SPARSE_ENT, ADAM_DENSE, ADAM_FULL)
USES_SC = (ADAGRAD_ENT, SCALAR_ACC, ADAM_MV, ADAM_SPARSE_ENT, ADAM_DENSE)
SQRT_DIV_KINDS = (ADAGRAD_ENT, ADAM_SPARSE_ENT, ADAM_DENSE, ADAM_FULL)      # P goes through sqrtf and a division: bounded, not bit-exact
ENTRY_WALK_KINDS = (SGD, ADAGRAD_ENT, ADAM_MV, ADAM_SPARSE_ENT)
ENTRY_WALK_DEFAULT_MIN = 64 * 4096
_alive = None
SENTINEL = F32(-12345.5)      # what sc_out holds where the pass must not write

EPS = F32(1e-6)
# fill_adam_consts (csrc/model.cpp): beta1 = 0.9f, beta2 = 0.999f widened to double
ONE_M_B1 = F32(1.0 - float(F32(0.9)))
ONE_M_B2 = F32(1.0 - float(F32(0.999)))
S_M = F32(1.0 - float(ONE_M_B1))
S_V = F32(1.0 - float(ONE_M_B2))
LAZY_HISTORY = 128                               # kLazyHistory (csrc/kernels.h)
LAZY_LAGS = (0, 1, 64, 127, 128)                 # the lags the table-pass cases lay their ladder out for
LAZY_KINDS = (SGD, ADAGRAD_ENT, ADAM_MV, ADAM_SPARSE_ENT)
SITE_ROW_PASS, SITE_BODY_SHORT, SITE_LONG_FINISH, SITE_ENTRY_WALK = "row_pass_kernel", "table_pass_body-short", "long-row-finish", "entry_walk_kernel"
SITES = (SITE_ROW_PASS, SITE_BODY_SHORT, SITE_LONG_FINISH, SITE_ENTRY_WALK)      # the four call sites of refresh_row_state


def lazy_ring(seed, ones=False):
    """The factor ring of a case: 128 distinct factors of the magnitudes a training run produces (1 - lambda lr), or all ones (lambda = 0)."""
    if ones:
        return np.ones(LAZY_HISTORY, F32)
    rs = np.random.RandomState(7000 + seed)
    while True:      # (two of 128 draws round to the same float32 once in sixty rings: draw again)
        ring = (1.0 - rs.uniform(1e-4, 3e-2, LAZY_HISTORY)).astype(F32)
        if np.unique(ring).size == LAZY_HISTORY:
            return ring


def refresh32(x, stamp, now, ring, shift=0):
    """Every row of x [rows][...] through the factors of the updates stamp[row] .. now - 1 it sat out: x = float32(x * ring[(u + shift)
    % 128]) for ascending u, one rounding per factor. shift != 0 is the WRONG slot (the sensitivity condition of the CPU test)."""
    x = np.array(x, F32, copy=True)
    stamp = np.asarray(stamp, np.int64)
    ring = np.asarray(ring, F32)
    assert x.shape[0] == stamp.shape[0] and ring.shape == (LAZY_HISTORY,) and np.all(stamp <= now) and np.all(stamp >= 0)
    tail = (1,) * (x.ndim - 1)
    for k in range(int((now - stamp).max()) if stamp.size else 0):
        u = stamp + k
        on = u < now
        x[on] = x[on] * ring[(u[on] + shift) % LAZY_HISTORY].reshape((-1,) + tail)
    assert x.dtype == F32
    return x


def scalar32(v, lag, s):
    """v[row] = float32(v[row] * s), lag[row] times; skipped altogether for s == 1, as the kernels skip it."""
    v = np.array(v, F32, copy=True)
    lag = np.asarray(lag, np.int64)
    s = F32(s)
    if s == F32(1.0):
        return v
    for k in range(int(lag.max()) if lag.size else 0):
        on = lag > k
        v[on] = v[on] * s
    return v


def chunk_entries(adam, dim, n):
    """Model::chunk_entries: entries per level-1 chunk of a long row."""
    return CHUNK_SMALL if (not adam and n <= CHUNK_SMALL_MAX_ENTRIES and dim <= 128) else CHUNK


def ladder(c):
    """Row lengths at every boundary of the chunk tree for chunks of c entries."""
    k = K_FAN
    return [0, 1, 2, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, k * c - 1, k * c, k * c + 1, (k + 1) * c, (k + 1) * c + 1,
            2 * k * c, 2 * k * c + 1, k * k * c, k * k * c + 1]


def short_ladder(c):
    """The same boundaries up to two level-2 chunks: about 10 000 entries at c = 64."""
    k = K_FAN
    return [0, 1, 2, c - 1, c, c + 1, 2 * c + 1, k * c, k * c + 1, (k + 1) * c + 1, 2 * k * c + 1]


def expected_chunks(lengths, c):
    """(level-1, level-2) chunks of a batch with these row lengths."""
    L = np.asarray(lengths, np.int64)
    nch = -(-L // c)
    long_rows = L > c
    two_level = long_rows & (nch > K_FAN)
    return int(nch[long_rows].sum()), int((-(-nch[two_level] // K_FAN)).sum())


def keys_from_lengths(lengths, seed, contiguous=False):
    """Row r exactly lengths[r] times; a seeded permutation spreads every row's entries over the batch (the sort must be stable)."""
    keys = np.repeat(np.arange(len(lengths), dtype=np.int32), np.asarray(lengths, np.int64))
    if not contiguous:
        keys = keys[np.random.RandomState(seed).permutation(keys.size)]
    return np.ascontiguousarray(keys)


class Case:
    """One call of nvsm_debug_table_pass: what goes in, and which path / chunk length / chunk counts it was built for."""

    def __init__(self, name, lengths, kind, table=0, dim=128, div=10, coef=True, src_scale=False, adam=False, max_entries=None,
                 dense=0, lam=0.0, one_launch=1, chunk_order=0, fill_in_bounds=0, entry_walk_min=ENTRY_WALK_DEFAULT_MIN,
                 contiguous=False, prev_lengths=None, path=PATH_DENSE, chunk=CHUNK, wide=0, nt=0, seed=1, lags=None, now=0):
        self.name, self.lengths, self.kind, self.table, self.dim, self.div = name, list(lengths), kind, table, dim, div
        self.coef, self.src_scale, self.adam, self.dense, self.lam = coef, src_scale and table == 0, adam, dense, lam
        self.one_launch, self.chunk_order, self.fill_in_bounds, self.entry_walk_min = one_launch, chunk_order, fill_in_bounds, entry_walk_min
        self.contiguous, self.prev_lengths, self.path, self.chunk, self.wide, self.nt, self.seed = contiguous, prev_lengths, path, chunk, wide, nt, seed
        self.rows = len(self.lengths)
        # lazy decay: lags per row (cut to `now`: a young table has no row further behind than it is old), None = the rows are current
        self.lazy, self.now = lags is not None, int(now)
        self.lags = np.minimum(np.asarray(lags, np.int64), self.now) if self.lazy else None
        assert not self.lazy or (len(self.lags) == self.rows and kind in LAZY_KINDS and prev_lengths is None and self.lags.min() >= 0
                                 and self.lags.max() <= LAZY_HISTORY)
        self.n = int(sum(self.lengths))
        self.prev_n = int(sum(prev_lengths)) if prev_lengths is not None else 0
        assert prev_lengths is None or len(prev_lengths) == self.rows
        self.max_entries = max_entries if max_entries is not None else max(self.n, self.prev_n, 1)
        self.lr = F32(0.0625 + 0.001)
        self.bc = F32(0.31622776)
        self.decay = F32(1.0 - float(F32(lam)) * float(self.lr)) if lam > 0 else F32(1.0)
        if kind == ADAM_FULL:
            self.decay = F32(1.0)      # (Model::update_words / update_entities: the L2 term is folded into the gradient)
        self.c_reg = F32(float(1.0 - float(F32(0.9))) * float(F32(lam)))

    def __repr__(self):
        return self.name

    def uses_q(self):
        return self.kind not in (SGD, ADAM_FULL)

    def draw(self):
        """The host arrays, drawn from the case's seed. One case's arrays are alive at a time (the larger ones are tens of MB)."""
        global _alive
        if hasattr(self, "keys"):
            return self
        if _alive is not None:
            _alive.release()
        _alive = self
        rs = np.random.RandomState(1000 + self.seed)
        rows, dim, nent = self.rows, self.dim, max(self.n, self.prev_n)
        self.keys = keys_from_lengths(self.lengths, self.seed, self.contiguous)
        self.prev_keys = keys_from_lengths(self.prev_lengths, self.seed + 1) if self.prev_lengths is not None else None
        self.num_src = max(1, -(-nent // self.div))
        self.X = rs.randint(-4, 5, (self.num_src, dim)).astype(F32)
        self.coefs = (rs.choice([0.5, 1.0, 2.0], nent) * rs.choice([-1.0, 1.0], nent)).astype(F32) if self.coef else None
        self.sq_src = rs.choice([0.25, 0.5, 1.0], self.num_src).astype(F32) if self.uses_q() else None
        self.scale = rs.choice([0.5, 1.0, 2.0], self.num_src).astype(F32) if self.src_scale else None
        self.P = rs.standard_normal((rows, dim)).astype(F32)
        self.m = rs.standard_normal((rows, dim)).astype(F32) if self.kind in USES_M else None
        self.v = rs.uniform(0.5, 2.0, (rows, dim)).astype(F32) if self.kind == ADAM_FULL else None
        self.sc_base = rs.uniform(0.5, 2.0, rows) if self.kind in USES_SC else None
        if self.lazy:
            self.stamp = (self.now - self.lags).astype(np.int32)
            self.ring = lazy_ring(self.seed, ones=self.decay == F32(1.0))
        return self

    def build(self):
        """... and the exact sums of every row."""
        self.draw()
        if hasattr(self, "g"):
            return self
        self.g, self.q, self.cnt = self.exact_sums()
        # the per-row scalar (Adagrad's accumulator, Adam's v) stays positive under the signed coefficients of the words table:
        # it starts at least |q| above zero
        self.sc_in = (self.sc_base + np.abs(self.q)).astype(F32) if self.kind in USES_SC else None
        return self

    def release(self):
        for name in ("keys", "prev_keys", "X", "coefs", "sq_src", "scale", "P", "m", "v", "sc_base", "g", "q", "cnt", "sc_in", "stamp", "ring", "_start"):
            self.__dict__.pop(name, None)

    def entry_terms(self):
        """Per entry: source row, coefficient of the gradient row (cf), term of the scalar (sq) - entry_terms() of update.hip."""
        e = np.arange(self.n, dtype=np.int64)
        src = e // self.div
        c = self.coefs[: self.n] if self.coefs is not None else np.ones(self.n, F32)
        cf = c * self.scale[src] if self.scale is not None else c
        if self.sq_src is None:
            sq = np.zeros(self.n, F32)
        else:
            sq = c * self.sq_src[src] if self.table == 0 else (c * c) * self.sq_src[src]
        return src, cf.astype(F32), sq.astype(F32)

    def exact_sums(self):
        """g [rows][dim], q [rows] as float64 (exact: see the module docstring) and the entry count of every row."""
        rows, dim = self.rows, self.dim
        g, q = np.zeros((rows, dim)), np.zeros(rows)
        cnt = np.bincount(self.keys, minlength=rows).astype(np.int64)
        if self.n == 0:
            return g, q, cnt
        src, cf, sq = self.entry_terms()
        order = np.argsort(self.keys, kind="stable")
        ks = self.keys[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        present = ks[starts]
        q[present] = np.add.reduceat(sq[order].astype(np.float64), starts)
        if self.kind != SCALAR_ACC:
            cfo, so = cf[order].astype(np.float64)[:, None], src[order]
            for c0 in range(0, dim, 32):
                g[present, c0:c0 + 32] = np.add.reduceat(cfo * self.X[so, c0:c0 + 32], starts, axis=0)
        return g, q, cnt

    def exactness(self):
        """Largest possible |partial sum| of g and of q in units of their granularity, from this case's own lengths and values."""
        self.draw()
        if self.n == 0:
            return 0.0, 0.0
        _, cf, sq = self.entry_terms()

        def units(x):      # the granularity of an array of dyadic values: the largest power of two that divides them all
            x = np.abs(x[x != 0]).astype(np.float64)
            if x.size == 0:
                return 1.0
            gran = 1.0
            while np.any(np.modf(x / gran)[0] != 0):
                gran /= 2
                assert gran >= 2.0 ** -10
            return gran
        longest = max(self.lengths)
        gg = units(cf)      # (X holds integers)
        return (longest * float(np.abs(cf).max()) * float(np.abs(self.X).max()) / gg,
                longest * float(np.abs(sq).max()) / units(sq) if self.sq_src is not None else 0.0)

    # ---- the row formulas ----
    def visited(self):
        """(rows that get the formula, rows whose P it rewrites): apply_row_formula_sc's touch_p in the three walks."""
        has = self.cnt > 0
        p_always = (self.decay != F32(1.0)) or self.kind in (ADAM_FULL, ADAM_DENSE)
        if self.dense and not self.lazy:      # (RowPassArgs::lazy: rows without entries are not visited, their decay stays pending)
            return np.ones(self.rows, bool), (np.ones(self.rows, bool) if p_always else has)
        return has, has

    def refreshes(self):
        """Which of P, m a lazy pass of this kind brings up to date (RowKindTraits: kUsesP, kUsesM): the moments pass of sparse Adam's
        words update leaves P alone, the wide SGD pass behind it leaves m alone."""
        return self.kind in USES_P, self.kind in USES_M

    def start(self):
        """What the row formula starts from - dict of P, m, sc: the inputs as they are, or (lazy) with the pending factors applied to
        the rows with entries: P by the ring, m by S_M, the scalar by S_V (the Adam kinds; Adagrad's accumulator does not decay)."""
        self.build()
        if not self.lazy:
            return dict(P=self.P, m=self.m, sc=self.sc_in)
        if not hasattr(self, "_start"):
            has = self.cnt > 0
            ref_p, ref_m = self.refreshes()
            P, m, sc = self.P, self.m, self.sc_in
            if ref_p:
                P = np.where(has[:, None], refresh32(self.P, self.stamp, self.now, self.ring), self.P)
            if ref_m:
                m = np.where(has[:, None], refresh32(self.m, self.stamp, self.now, np.full(LAZY_HISTORY, S_M, F32)), self.m)
            if sc is not None:
                sc = np.where(has, scalar32(self.sc_in, self.lags, S_V if self.kind in USES_M else F32(1.0)), self.sc_in)
            self._start = dict(P=P, m=m, sc=sc)
        return self._start

    def stamps_after(self):
        """The rows with entries carry this update, the others keep their stamp."""
        self.build()
        return np.where(self.cnt > 0, self.now + 1, self.stamp).astype(np.int32)

    def sites(self, path=None, chunk=None):
        """The call sites of refresh_row_state (csrc/update.hip) this case takes its rows with entries through - by the path and chunk
        length it was built for, or by those a launch reported."""
        path = self.path if path is None else path
        chunk = self.chunk if chunk is None else chunk
        short = any(0 < L <= chunk for L in self.lengths)
        long_ = any(L > chunk for L in self.lengths)
        out = set()
        if not self.one_launch:
            out.add(SITE_ROW_PASS)                       # the three-launch form: every row, short or long
        else:
            if long_:
                out.add(SITE_LONG_FINISH)                # (also behind an entry walk: the chunk-only launch finishes those rows)
            if short:
                out.add(SITE_ENTRY_WALK if path == PATH_ENTRY_WALK else SITE_BODY_SHORT)
        return out

    def reference32(self):
        """The state after the pass in np.float32 arithmetic: dict of P, m, v, sc (None where the kind has none)."""
        self.build()
        k = self.kind
        vis, touch = self.visited()
        g, q, fc = self.g.astype(F32), self.q.astype(F32), self.cnt.astype(F32)
        assert np.array_equal(g.astype(np.float64), self.g) and np.array_equal(q.astype(np.float64), self.q)
        st = self.start()
        sc_in = st["sc"]
        P, m = st["P"].copy(), (st["m"].copy() if st["m"] is not None else None)
        v = self.v.copy() if self.v is not None else None
        lr, decay, bc = self.lr, self.decay, self.bc
        sc = None
        if k in USES_SC:      # (a lazy pass writes the stored scalar in place: rows it does not visit keep what they hold)
            sc = self.sc_in.copy() if (k == SCALAR_ACC or self.lazy) else np.full(self.rows, SENTINEL, F32)
        V, T = vis[:, None], touch[:, None]
        with np.errstate(all="ignore"):
            if k == SGD:
                P = np.where(T, P * decay + lr * g, P)
            elif k == ADAGRAD_ENT:
                acc = sc_in + q
                sc = np.where(vis, acc, sc)
                s = F32(1.0) / np.sqrt(acc + EPS)
                P = np.where(T, P * decay + lr * (g * s[:, None]), P)
            elif k == SCALAR_ACC:
                sc = np.where(vis, sc_in + q, sc)
            elif k == ADAM_FULL:
                mn = m * S_M + ONE_M_B1 * g
                mn = mn + (-self.c_reg) * P
                ag = g + (-F32(self.lam)) * P
                ag = ag * ag
                vn = v * S_V + ag * ONE_M_B2
                pn = P + ((mn / (np.sqrt(vn) + EPS)) * bc) * lr
                m, v, P = np.where(V, mn, m), np.where(V, vn, v), np.where(V, pn, P)
            else:
                mn = m * S_M + ONE_M_B1 * g
                m = np.where(V, mn, m)
                vn = sc_in * S_V + ONE_M_B2 * q
                sc = np.where(vis, vn, sc)
                denom = (np.sqrt(vn) + EPS)[:, None]
                if k == ADAM_SPARSE_ENT:
                    P = np.where(T, P * decay + (lr * fc)[:, None] * ((bc * mn) / denom), P)
                elif k == ADAM_DENSE:
                    P = np.where(T, P * decay + ((mn / denom) * bc) * lr, P)
        for a in (P, m, v, sc):
            assert a is None or a.dtype == F32
        return dict(P=P, m=m, v=v, sc=sc)

    def reference64(self, ref32):
        """P of the kinds whose formula holds sqrtf or a division, in float64 from the exact g, q and the float32 state (the new m and
        the new scalar / v, which are asserted bit for bit), and the allowance per element:
            2^-20 |step| + 2^-23 max(|p decay|, |P_new|)
        The step passes through at most five rounded operations from that state, sqrtf and / allowed 3 ulp each, the others half an
        ulp: under 16 ulp = 2^-20 relative; the decay product and the final add round once each: half an ulp (2^-24) of either."""
        k = self.kind
        assert k in SQRT_DIV_KINDS
        _, touch = self.visited()
        P, g = self.start()["P"].astype(np.float64), self.g
        lr, decay, bc, eps = float(self.lr), float(self.decay), float(self.bc), float(EPS)
        with np.errstate(all="ignore"):
            if k == ADAGRAD_ENT:
                step = lr * (g / np.sqrt(ref32["sc"].astype(np.float64) + eps)[:, None])
            elif k == ADAM_FULL:
                step = lr * bc * ref32["m"].astype(np.float64) / (np.sqrt(ref32["v"].astype(np.float64)) + eps)
            else:
                denom = (np.sqrt(ref32["sc"].astype(np.float64)) + eps)[:, None]
                step = lr * bc * ref32["m"].astype(np.float64) / denom
                if k == ADAM_SPARSE_ENT:
                    step = step * self.cnt[:, None]
        step = np.where(touch[:, None], step, 0.0)
        base = np.where(touch[:, None], P * decay, P)
        new = base + step
        tol = 2.0 ** -20 * np.abs(step) + 2.0 ** -23 * np.maximum(np.abs(base), np.abs(new))
        return new, np.where(touch[:, None], tol, 0.0)


# =====================================================================================================================
# The cases
# =====================================================================================================================
def _pad(lengths, rows, fill=0):
    return list(lengths) + [fill] * (rows - len(lengths))


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    L64, L32 = ladder(64), ladder(32)

    # ---- the length ladder (dense walk: 18 rows, 150 214 / 75 107 entries). Ascending: the longest row is row rows - 1 and its tail is
    #      entry n - 1; reversed: it is row 0 and the bisection of csr_bounds_kernel ends at lo = 0 ----
    for one in (1, 0):
        f = "one" if one else "three"
        add("ladder64-adam_mv-words-wts-div10-dim300-%s" % f, L64, ADAM_MV, table=0, dim=300, div=10, adam=True, one_launch=one, dense=1, seed=2)
        add("ladder64-adam_sparse-ents-div17-dim256-rev-%s" % f, L64[::-1], ADAM_SPARSE_ENT, table=1, dim=256, div=17, adam=True, one_launch=one, dense=1, lam=0.01, seed=3)
        add("ladder64-adam_dense-words-nowts-div10-dim128-%s" % f, L64, ADAM_DENSE, table=0, dim=128, div=10, coef=False, adam=True, one_launch=one, dense=1, seed=4)
        add("ladder64-adam_full-ents-div1-dim64-rev-%s" % f, L64[::-1], ADAM_FULL, table=1, dim=64, div=1, adam=True, one_launch=one, dense=1, lam=0.01, seed=5)
        add("ladder64-sgd-words-scale-div10-dim260-%s" % f, L64, SGD, table=0, dim=260, div=10, src_scale=True, one_launch=one, lam=0.01, dense=1, seed=6)
        add("ladder64-sgd_wide-words-wts-div17-dim128-rev-%s" % f, L64[::-1], SGD, table=0, dim=128, div=17, adam=True, wide=1, one_launch=one, seed=7)
        add("ladder64-sgd-ents-div1-dim140-contiguous-%s" % f, L64, SGD, table=1, dim=140, div=1, one_launch=one, contiguous=True, nt=3, seed=8)
        add("ladder32-sgd-words-wts-div10-dim128-%s" % f, L32, SGD, table=0, dim=128, div=10, one_launch=one, chunk=32, max_entries=131072, lam=0.01, dense=1, seed=9)
        add("ladder32-adagrad-ents-div17-dim100-rev-%s" % f, L32[::-1], ADAGRAD_ENT, table=1, dim=100, div=17, one_launch=one, chunk=32, dense=1, lam=0.01, seed=10)
        add("ladder32-scalar_acc-words-wts-div10-dim128-%s" % f, L32, SCALAR_ACC, table=0, dim=128, div=10, one_launch=one, chunk=32, seed=11)
        add("ladder32-adagrad-words-nowts-div1-dim4-%s" % f, L32, ADAGRAD_ENT, table=0, dim=4, div=1, coef=False, one_launch=one, chunk=32, dense=1, seed=12)
        add("ladder32-sgd-words-scale-div17-dim96-rev-%s" % f, L32[::-1], SGD, table=0, dim=96, div=17, src_scale=True, one_launch=one, chunk=32, fill_in_bounds=1, seed=13)

    # ---- placement ----
    for c, kw in ((64, dict(adam=True, kind=ADAM_MV)), (32, dict(kind=ADAGRAD_ENT, chunk=32))):
        for one in (1, 0):
            f = "one" if one else "three"
            kind = kw["kind"]
            rest = {k: v for k, v in kw.items() if k != "kind"}
            add("only-row-c%d+1-%s" % (c, f), [0, 0, c + 1, 0], kind, table=1, dim=12, div=3, one_launch=one, dense=1, seed=20, **rest)
            add("only-row-c%d+1-sparse-%s" % (c, f), _pad([0, 0, c + 1], 40), kind, table=1, dim=12, div=3, one_launch=one, seed=21,
                path=PATH_LIST_WALK, **rest)
    for one in (1, 0):
        for fib in (0, 1):
            # a row of exactly a chunk in front, then two rows of c + 1: their tails are entries 64 and 97, one wave's positions 64 .. 127
            add("two-c32+1-rows-adjacent-%s-fib%d" % ("one" if one else "three", fib), [32, 33, 33, 5], SGD, table=0, dim=8, div=2, one_launch=one,
                chunk=32, fill_in_bounds=fib, seed=22)

    # ---- no entry at all: a dense pass still decays every row, another one touches nothing ----
    for one in (1, 0):
        f = "one" if one else "three"
        add("empty-batch-dense-%s" % f, [0, 0, 0, 0, 0], ADAM_SPARSE_ENT, table=1, dim=20, adam=True, one_launch=one, dense=1, lam=0.01, max_entries=100, seed=25)
        add("empty-batch-sparse-%s" % f, [0, 0, 0], SGD, table=0, dim=7, one_launch=one, max_entries=100, chunk=32, seed=26)

    # ---- CSR build forms: either side of kCsrMergeMaxEntries (chunks reserved by the bounds kernel / by csr_chunks_kernel), with and
    #      without a chunk order; one-entry rows pad the c = 64 ladder ----
    for n in (262143, 262144):
        for order in (0, 1):
            lengths = L64 + [1] * (n - sum(L64))
            add("merge-n%d-order%d" % (n, order), lengths, ADAM_MV if order else SGD, table=1, dim=8, div=10, adam=True, chunk_order=order,
                max_entries=262144, dense=1, lam=0.01, seed=30 + order)
    add("merge-n262144-three", L64 + [1] * (262144 - sum(L64)), ADAM_DENSE, table=0, dim=4, div=10, adam=True, one_launch=0, max_entries=262144, dense=1, seed=33)
    for one in (1, 0):
        f = "one" if one else "three"
        add("order-ladder64-%s" % f, L64[::-1], ADAM_SPARSE_ENT, table=1, dim=64, div=10, adam=True, chunk_order=1, one_launch=one, dense=1, seed=34)
        add("order-ladder32-%s" % f, L32, SGD, table=0, dim=32, div=10, chunk_order=1, chunk=32, one_launch=one, seed=35)
        # no long row at all next to a chunk order: num_chunks[0] == 0 early-outs
        add("order-no-long-row-%s" % f, [0, 1, 64, 63, 2, 64, 17], ADAM_MV, table=0, dim=64, div=10, adam=True, chunk_order=1, one_launch=one, dense=1, seed=36)
        add("fill-in-bounds-ladder64-%s" % f, L64, ADAM_MV, table=0, dim=16, div=10, adam=True, fill_in_bounds=1, one_launch=one, dense=1, seed=37)

    # ---- the cap: as many rows of exactly c + 1 entries as max_entries holds, the rest in one more row ----
    def cap(name, c, max_entries, **kw):
        r = max_entries // (c + 1)
        lengths = [c + 1] * r + ([max_entries - r * (c + 1)] if max_entries % (c + 1) else [])
        add("cap-%s-c%d-max%d" % (name, c, max_entries), lengths, max_entries=max_entries, chunk=c, **kw)
    for me in (33, 66, 100, 4321, 131072):
        cap("sgd", 32, me, kind=SGD, table=0, dim=4, div=10, seed=40)
    cap("adagrad-three", 32, 131072, kind=ADAGRAD_ENT, table=1, dim=8, div=10, one_launch=0, dense=1, seed=41)
    for me in (65, 130, 200, 4321, 131072):
        cap("adam_mv", 64, me, kind=ADAM_MV, table=1, dim=4, div=10, adam=True, dense=1, seed=42)
    cap("sgd-above-small", 64, 131073, kind=SGD, table=0, dim=4, div=10, seed=43)      # the smallest batch of an SGD handle with 64-entry chunks
    cap("sgd-wide-rows", 64, 6500, kind=SGD, table=0, dim=132, div=10, seed=44)        # dim > 128: 64-entry chunks at any size
    cap("adam_dense-three", 64, 131072, kind=ADAM_DENSE, table=0, dim=4, div=10, adam=True, one_launch=0, dense=1, seed=45)

    # ---- geometry (short ladder): thread groups of 1, 3, 7, 32, 64, 65, 75, 128, 129, 256 (column loop strides at 1028) ----
    kinds64 = [ADAM_MV, ADAM_SPARSE_ENT, ADAM_DENSE, ADAM_FULL, SGD]
    kinds32 = [SGD, ADAGRAD_ENT, SCALAR_ACC]
    for i, dim in enumerate([1, 3, 4, 7, 128, 256, 260, 300, 512, 516, 1028]):
        for one in (1, 0):
            f = "one" if one else "three"
            k = kinds64[(i + one) % 5]
            add("geometry-dim%d-c64-%s-%s" % (dim, KIND_NAMES[k], f), short_ladder(64), k, table=i % 2, dim=dim, div=(1, 10, 17)[i % 3], adam=True,
                one_launch=one, dense=1, lam=0.01 if i % 2 else 0.0, seed=50 + i)
            if dim <= 128:
                k = kinds32[(i + one) % 3]
                add("geometry-dim%d-c32-%s-%s" % (dim, KIND_NAMES[k], f), short_ladder(32)[::-1], k, table=(i + 1) % 2, dim=dim, div=(10, 17, 1)[i % 3],
                    one_launch=one, chunk=32, dense=0 if k == SCALAR_ACC else 1, lam=0.01, seed=70 + i)

    # ---- regimes, each in both launch forms and with dense 0 and 1 ----
    walk_rows = [30, 31, 32, 33, 1, 47, 48, 49, 1, 1, 60, 61, 62, 63, 64, 1, 2, 3, 35, 5, 64, 7, 64, 64, 9]
    for one in (1, 0):
        f = "one" if one else "three"
        for dense in (0, 1):
            lam = 0.01 if dense else 0.0
            s = short_ladder(64)
            n = sum(s)
            tag = "%s-dense%d" % (f, dense)
            # list walk: rows * 2 >= n, rows < n, n below the entry walk's minimum
            add("regime-list-adam_sparse-%s" % tag, _pad(s, n // 2 + 3), ADAM_SPARSE_ENT, table=1, dim=64, div=10, adam=True, one_launch=one, dense=dense,
                lam=lam, path=PATH_LIST_WALK, seed=90)
            add("regime-list-adam_dense-stays-dense-%s" % tag, _pad(s, n // 2 + 3), ADAM_DENSE, table=0, dim=12, div=10, adam=True, one_launch=one,
                dense=1, lam=lam, path=PATH_DENSE, seed=91)      # (a kind that is not row-local for untouched rows is never split)
            s32 = short_ladder(32)
            add("regime-list-sgd-c32-%s" % tag, _pad(s32[::-1], (sum(s32) + 1) // 2), SGD, table=0, dim=28, div=17, one_launch=one, dense=dense, lam=lam,
                chunk=32, path=PATH_LIST_WALK, seed=92)
            # shallow list walk: rows >= n
            add("regime-shallow-adagrad-c32-%s" % tag, _pad(s32, sum(s32)), ADAGRAD_ENT, table=1, dim=20, div=10, one_launch=one, dense=dense, lam=lam,
                chunk=32, path=PATH_LIST_WALK, seed=93)
            add("regime-shallow-adam_mv-%s" % tag, _pad(s[::-1], n + 100), ADAM_MV, table=0, dim=300, div=10, adam=True, one_launch=one, dense=dense,
                path=PATH_LIST_WALK, seed=94)
            add("regime-shallow-scalar_acc-%s" % tag, _pad(s32, sum(s32) + 1), SCALAR_ACC, table=0, dim=64, div=10, one_launch=one, dense=0,
                chunk=32, path=PATH_LIST_WALK, seed=95)
            # entry walk (one-launch form only: the three-launch form walks the list): rows of 30 - 64 entries between ones, so that
            # they straddle the wave's 4, 8 or 16 positions (n < 65 536: 4; < 131 072: 8; above: 16), and a two-level row for the
            # chunk-only launch next to it
            ew = PATH_ENTRY_WALK if one else PATH_LIST_WALK
            for j, (k, dim, target, c) in enumerate([(SGD, 128, 0, 32), (ADAGRAD_ENT, 7, 0, 32), (ADAM_MV, 256, 0, 64), (ADAM_SPARSE_ENT, 260, 0, 64),
                                                     (SGD, 512, 0, 64), (ADAM_MV, 32, 70000, 64), (ADAM_SPARSE_ENT, 8, 140000, 64),
                                                     (ADAGRAD_ENT, 16, 70000, 32), (SGD, 132, 70000, 64), (SGD, 12, 140000, 64)]):
                if target and not one:
                    continue      # (the large batches once: the three-launch form has no entry walk, and the small ones show that)
                body = walk_rows + [K_FAN * c + 1, 2 * c + 1] + walk_rows[::-1]
                if target:
                    body = body + [1] * (target - sum(body))
                nn = sum(body)
                add("regime-entry-walk-%s-dim%d-n%d-%s" % (KIND_NAMES[k], dim, nn, tag), _pad(body, max(len(body), nn // 2 + 1)), k, table=j % 2, dim=dim,
                    div=(10, 1, 17)[j % 3], adam=k in USES_M, one_launch=one, dense=dense, lam=lam, entry_walk_min=0, chunk=c, path=ew,
                    seed=100 + j)
            # 129 column vectors: refused by the entry walk
            body = walk_rows + [2049]
            add("regime-entry-walk-refused-dim516-%s" % tag, _pad(body, sum(body)), SGD, table=1, dim=516, div=10, one_launch=one, dense=dense, lam=lam,
                entry_walk_min=0, path=PATH_LIST_WALK, seed=110)
            # a kind the entry walk does not take
            add("regime-entry-walk-other-kind-%s" % tag, _pad(body, sum(body)), SCALAR_ACC, table=0, dim=64, div=10, adam=True, one_launch=one, dense=0,
                entry_walk_min=0, path=PATH_LIST_WALK, seed=111)
        # dense walk, dense 0: rows without entries stay as they are
        add("regime-dense-sparse-pass-%s" % f, short_ladder(64) + [0, 0, 5, 0], SGD, table=1, dim=36, div=10, adam=True, wide=1, one_launch=one, seed=112)

    # ---- leftover counters: the c = 64 ladder first, then other lengths on other rows through the same workspace ----
    other = [65, 2 * K_FAN * 64 + 1, 0, 64, K_FAN * 64 + 1, 3 * 64, 1, K_FAN * 64, 0, 130, (K_FAN + 2) * 64 + 5, 2, 63, 64 * 40, 0, 7, 129, 66]
    for one in (1, 0):
        f = "one" if one else "three"
        add("leftover-ladder64-then-other-%s" % f, other, ADAM_SPARSE_ENT, table=1, dim=128, div=10, adam=True, one_launch=one, dense=1, lam=0.01,
            prev_lengths=L64[::-1], seed=120)
        add("leftover-order-%s" % f, other[::-1], ADAM_MV, table=0, dim=32, div=10, adam=True, one_launch=one, chunk_order=1, prev_lengths=L64, seed=121)
        add("leftover-c32-%s" % f, [33, 0, 2 * K_FAN * 32 + 1, 32, K_FAN * 32 + 1, 0, 65, 1] + [0] * 10, SGD, table=0, dim=64, div=10, one_launch=one,
            chunk=32, prev_lengths=L32, seed=122)
    out.extend(_lazy_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# ---- lazy decay: a pass over a table whose rows carry pending factors (tests/test_gpu_lazy_rows.py) ----
# kind variants of a lazy pass: (name, kind, extra arguments, tables it is run on)
LAZY_VARIANTS = [("sgd", SGD, dict(), (0, 1)), ("sgd_wide", SGD, dict(wide=1, adam=True), (0, 0)), ("sgd_scale", SGD, dict(src_scale=True), (0, 0)),
                 ("adagrad_ent", ADAGRAD_ENT, dict(), (1, 0)), ("adam_mv", ADAM_MV, dict(adam=True), (0, 1)),
                 ("adam_sparse_ent", ADAM_SPARSE_ENT, dict(adam=True), (1, 0))]
LAZY_NOWS = (5, 128, 421, 1000003)      # a young table (lags cut to 5, stamp 0 present); a full ring; a lag range across the wrap; a large count
LAZY_DIMS = (3, 7, 12, 128, 256, 300)
LAZY_FORMS = ("one", "three", "walk")   # list walk in one launch / in three; entry walk


def lazy_layout(lengths_per_lag, lags=LAZY_LAGS, shallow=False):
    """The lengths once per lag, then rows without entries, their lags cycling through the same set, until rows * 2 >= n: the pass
    is split, as a lazy table's always is - or (shallow) until rows >= n, where launch_table_pass sets RowPassArgs::shallow, as it
    does for every table much larger than the batch. Returns (lengths, lags per row)."""
    lengths, row_lags = [], []
    for lag in lags:
        lengths += list(lengths_per_lag)
        row_lags += [lag] * len(lengths_per_lag)
    n = sum(lengths)
    i = 0
    while (1 if shallow else 2) * len(lengths) < n:
        lengths.append(0)
        row_lags.append(lags[i % len(lags)])
        i += 1
    return lengths, row_lags


def lazy_chunk(variant_kw, dim, n):
    return chunk_entries(variant_kw.get("adam", False), dim, n)


def lazy_lengths(form, c, dim):
    """List walk: the short ladder (up to kFan c + 1 for dim >= 256): a short row, c, c + 1, kFan c + 1, 2 kFan c + 1 - every boundary of
    the chunk tree. Entry walk: the short-row lengths, between ones so that the rows straddle a wave's positions."""
    if form == "walk":
        return [L for L in (30, 31, 32, 33, 1, 47, 48, 49, 1, 1, 60, 61, 62, 63, 64, 1, 2, 3, 35, 5, 64, 7, 64, 64, 9) if L <= c]
    s = short_ladder(c)
    return [L for L in s if L <= K_FAN * c + 1] if dim >= 256 else s


# per (walk, kind variant): every `now` at lambda > 0 - a ring of distinct factors, the tables alternating, the second of them a
# shallow pass -, then lambda = 0 (a ring of ones: P must come back untouched by the refresh) once on either table
LAZY_PLAN = [(now, 0.01, i % 2, i == 1) for i, now in enumerate(LAZY_NOWS)] + [(128, 0.0, 0, False), (421, 0.0, 1, True)]


def lazy_variant(c):
    return ("sgd_wide" if c.wide else "sgd_scale" if c.src_scale else "sgd") if c.kind == SGD else KIND_NAMES[c.kind]


def _lazy_cases():
    out = []
    for fi, form in enumerate(LAZY_FORMS):
        dims = [d for d in LAZY_DIMS if form != "walk" or d <= 256]      # (the entry walk takes rows of at most 128 column vectors)
        for ki, (vname, kind, kw, tables) in enumerate(LAZY_VARIANTS):
            for ji, (now, lam, ti, shallow) in enumerate(LAZY_PLAN):
                dim = dims[(ki + ji + fi) % len(dims)]
                table = tables[ti]
                c = lazy_chunk(kw, dim, 1)                  # (n stays below the small-chunk limit: the chunk length follows kind and dim)
                lengths, lags = lazy_layout(lazy_lengths(form, c, dim), shallow=shallow)
                assert sum(lengths) <= CHUNK_SMALL_MAX_ENTRIES
                walk = form == "walk"
                out.append(Case("lazy-%s-%s-%s-dim%d-c%d-now%d-lam%s%s" % (form, vname, "words" if table == 0 else "ents", dim, c, now, "1" if lam else "0",
                                                                         "-shallow" if shallow else ""),
                                lengths, kind, table=table, dim=dim, div=(10, 1, 17)[(ki + ji) % 3], one_launch=0 if form == "three" else 1,
                                dense=1, lam=lam, chunk=c, entry_walk_min=0 if walk else ENTRY_WALK_DEFAULT_MIN,
                                path=PATH_ENTRY_WALK if walk else PATH_LIST_WALK, lags=lags, now=now, seed=200 + 36 * fi + 6 * ki + ji, **kw))
    return out


def lazy_coverage(cases, sites=None):
    """{(site, axis, value)} the cases reach (sites: those of a launch's report, instead of the case's own). A kind whose pass
    refreshes P counts for a `now` only with lambda > 0: with a ring of ones no slot can be told from another."""
    got = set()
    for c in cases:
        variant = lazy_variant(c)
        lam = bool(c.lam > 0)
        axes = [("kind", variant), ("lambda", lam), ("table", c.table), ("dim", c.dim), ("chunk", c.chunk), ("now", c.now),
                ("table-lambda", (c.table, lam)), ("kind-table-lambda", (variant, c.table, lam)), ("shallow", c.rows >= c.n)]
        if lam or c.kind not in USES_P:
            axes.append(("kind-now", (variant, c.now)))
        for site in (c.sites() if sites is None else sites):
            for axis, value in axes:
                got.add((site, axis, value))
    return got


def lazy_coverage_wanted():
    """Every value of every axis at every refresh site (the entry walk has no dim 300): kind, lambda, table, dim, chunk length, `now`,
    shallow or not; every table with lambda > 0 and with lambda = 0, per kind too (on the tables the model runs it on); every kind at
    every `now` with distinct factors."""
    want = set()
    for site in SITES:
        for name, _, _, tables in LAZY_VARIANTS:
            want.add((site, "kind", name))
            for now in LAZY_NOWS:
                want.add((site, "kind-now", (name, now)))
            for t in set(tables):
                for lam in (True, False):
                    want.add((site, "kind-table-lambda", (name, t, lam)))
        for axis, values in (("lambda", (True, False)), ("table", (0, 1)), ("chunk", (32, 64)), ("now", LAZY_NOWS), ("shallow", (True, False)),
                             ("table-lambda", [(t, lam) for t in (0, 1) for lam in (True, False)]),
                             ("dim", [d for d in LAZY_DIMS if site != SITE_ENTRY_WALK or d <= 256])):
            for v in values:
                want.add((site, axis, v))
    return want


CASES = _cases()
