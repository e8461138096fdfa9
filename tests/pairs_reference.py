"""numpy fp64 restatement of the entity-entity similarity objective and of the documents-table update from one or two
gradient lists — the checker of tests/test_gpu_pairs.py (a helper, not a test; tests/test_pairs_reference.py holds it against
central differences). Clamps are evaluated in float32, as the reference (release build: FloatT = float) and the kernel do.

Every function cites the reference lines it follows (cuNVSM, cpp/ and include/cuNVSM/)."""
import numpy as np

BETA1, BETA2, EPSILON = np.float32(0.9), np.float32(0.999), np.float32(1e-6)      # include/cuNVSM/updates.h:21,183-185


def sigmoid(s):
    """func::sigmoid, include/cuNVSM/cuda_utils.h:193-214: the two-branch form that never exponentiates a positive number."""
    s = np.asarray(s)
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def truncated_sigmoid(s, clip=True):
    """func::truncated_sigmoid(epsilon = 1e-7), cpp/objective.cu:546-550 / cuda_utils.h:193-214. The probability itself in
    fp64; WHETHER a clamp is active is decided on the float32 evaluation, and an active clamp yields the float32 bound."""
    p = sigmoid(np.asarray(s, np.float64))
    if not clip:
        return p
    eps = np.float32(1e-7)
    hi = np.float32(1.0 - np.float64(eps))
    p32 = sigmoid(np.asarray(s, np.float32)).astype(np.float32)
    p = np.where(p32 <= eps, np.float64(eps), p)
    p = np.where(p32 >= hi, np.float64(hi), p)
    return p


def log_sigmoid_deriv(p, clip=True):
    """func::sigmoid_to_log_sigmoid_deriv(epsilon = 1e-6), cpp/objective.cu:620-623 / cuda_utils.h:218-235:
    0 where p >= 1 - eps (compared in double) or p <= eps, else 1 - p; the comparisons on the float32 probability."""
    p = np.asarray(p, np.float64)
    if not clip:
        return 1.0 - p
    eps = np.float32(1e-6)
    p32 = p.astype(np.float32)
    off = (p32.astype(np.float64) >= 1.0 - np.float64(eps)) | (p32 <= eps)
    return np.where(off, 0.0, 1.0 - p)


def pair_forward(E, pairs, weights=None, clip=True, scale=1.0):
    """RepresentationSimilarity::Objective::compute_cost + compute_gradients on ENTITY_REPRS (cpp/objective.cu:487-664).
    E [nD, de]; pairs [M, 2]; weights [M] or None; scale: the mixture share w_ee / (w_te + w_ee) (MergeGradientsFn,
    cpp/intermediate_results.cu:19-38). Returns probs [M], cost, multipliers [M] (scale included), grad [2M, de] and the
    interleaved ids [2M] (features[2p], features[2p + 1], cpp/data.cu:316-334)."""
    E = np.asarray(E, np.float64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    M = pairs.shape[0]
    w = np.ones(M) if weights is None else np.asarray(weights, np.float64)
    ra, rb = E[pairs[:, 0]], E[pairs[:, 1]]                      # get_representations: copies, :519-521
    s = (ra * rb).sum(axis=1)                                    # fold_columns<multiplies> + reduce_axis, :526-543
    probs = truncated_sigmoid(s, clip)                           # :546-550
    cost = -(w * np.log(probs)).sum() / M                        # :553-567, intermediate_results.cu:81-124
    mult = w * (log_sigmoid_deriv(probs, clip) * np.exp(-np.log(M))) * scale        # :607-626
    grad = np.empty((2 * M, E.shape[1]))
    grad[0::2] = mult[:, None] * rb                              # flip_adjacent_columns + apply_columnwise, :643-661
    grad[1::2] = mult[:, None] * ra
    return dict(probs=probs, cost=cost, multipliers=mult, grad=grad, ids=pairs.reshape(-1))


def pair_cost(E, pairs, weights=None, clip=True):
    return pair_forward(E, pairs, weights, clip)["cost"]


def dense_gradient(shape, lists):
    """The summed gradient of the table: Σ over the lists' entries (update_repr_kernel's scatter, cpp/storage.cu:37-49)."""
    g = np.zeros(shape)
    for grad, ids in lists:
        np.add.at(g, np.asarray(ids, np.int64), np.asarray(grad, np.float64))
    return g


def scaled_lambda(lam, B=None, M=None):
    """ForwardResult::scaled_regularization_lambda: lambda / batch (intermediate_results.cu:126-129); the mean of the two for the
    merged result (AverageFn)."""
    parts = [lam / n for n in (B, M) if n]
    return sum(parts) / len(parts)


class TableOptimizer:
    """The documents table under one optimiser, updated from a LIST of (grad [n, de], ids [n]) gradient lists (window 1, no
    per-entry weights: cpp/intermediate_results.cu:300-307) — RepresentationsStorage::update (cpp/storage.cu:51-102) and the
    Representations updaters (cpp/updates.cu:36-48, updates_adagrad.cu:99-179, updates_adam.cu:153-385).
    method: sgd | adagrad | sparse_adam | dense_adam | full_adam."""

    def __init__(self, E, method):
        self.P = np.array(E, np.float64)
        self.method = method
        n, d = self.P.shape
        self.t = 1                                               # updates_adam.cu:130
        if method == "adagrad":
            self.a = np.zeros(n)                                 # updates_adagrad.cu:79-81
        elif method in ("sparse_adam", "dense_adam"):
            self.m, self.v = np.zeros((n, d)), np.zeros(n)       # updates_adam.cu:122-127
        elif method == "full_adam":
            self.m, self.v = np.zeros((n, d)), np.zeros((n, d))
        elif method != "sgd":
            raise ValueError(method)

    @staticmethod
    def _storage_update(S, lists, lr, lam):
        """cpp/storage.cu:51-102: one decay (1 - lam * lr) when lam > 0, then every list's scatter-add of lr * grad."""
        if lam > 0:
            S *= np.float64(np.float32(1.0 - np.float64(np.float32(lam)) * np.float64(np.float32(lr))))
        for grad, ids in lists:
            np.add.at(S, np.asarray(ids, np.int64), lr * np.asarray(grad, np.float64))

    def update(self, lists, lr, lam):
        lists = [(np.asarray(g, np.float64), np.asarray(i, np.int64)) for g, i in lists]
        P = self.P
        if self.method == "sgd":                                 # updates.cu:36-48
            self._storage_update(P, lists, lr, lam)
            return
        if self.method == "adagrad":                             # updates_adagrad.cu:99-179
            if len(lists) != 1:
                raise RuntimeError("Adagrad currently does not implement multiple gradients.")      # :108
            g, ids = lists[0]
            np.add.at(self.a, ids, (g * g).sum(axis=1) * np.exp(-np.log(g.shape[1])))               # :136-158
            g = g / np.sqrt(self.a[ids] + np.float64(EPSILON))[:, None]                             # adagrad_update_kernel :83-97
            self._storage_update(P, [(g, ids)], lr, lam)                                             # :177-178
            return
        b1, b2 = np.float64(BETA1), np.float64(BETA2)
        one_m_b1, one_m_b2 = np.float64(np.float32(1.0 - b1)), np.float64(np.float32(1.0 - b2))
        full = self.method == "full_adam"
        self._storage_update(self.m, lists, one_m_b1, 1.0)                                           # m_t, updates_adam.cu:196-200
        if full:
            self.m += -(np.float64(np.float32((1.0 - b1) * lam))) * P                               # :203-213
            agg = dense_gradient(P.shape, lists)                                                     # :253-282
            agg += -lam * P
            self.v = self.v * np.float64(np.float32(1.0 - one_m_b2)) + one_m_b2 * agg * agg
        else:
            sq = [((g * g).sum(axis=1, keepdims=True) * np.exp(-np.log(g.shape[1])), ids) for g, ids in lists]      # :216-252
            v = self.v[:, None]
            self._storage_update(v, sq, one_m_b2, 1.0)
        bc = np.float64(np.float32(np.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)))              # :285
        self.t += 1
        eps = np.float64(EPSILON)
        if self.method == "dense_adam":                                                              # :293-311
            decay = np.float64(np.float32(1.0 - np.float64(np.float32(lam)) * np.float64(np.float32(lr))))
            P[...] = P * decay + lr * bc * self.m / (np.sqrt(self.v)[:, None] + eps)
        elif full:                                                                                   # :312-328
            P[...] = P + lr * bc * self.m / (np.sqrt(self.v) + eps)
        else:                                                                                        # sparse, :332-384
            if len(lists) != 1:
                raise RuntimeError("Sparse Adam currently does not implement multiple gradients.")  # :348
            _, ids = lists[0]
            upd = bc * self.m[ids] / (np.sqrt(self.v[ids]) + eps)[:, None]                          # adam_sparse_update_kernel :132-151
            self._storage_update(P, [(upd, ids)], lr, lam)
