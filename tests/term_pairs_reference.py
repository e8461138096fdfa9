"""numpy fp64 restatement of the term-term similarity objective (RepresentationSimilarity::Objective with param_id_ == WORD_REPRS,
cpp/objective.cu:485-696) and of the WORDS-table update from one or two windowed gradient lists — the checker of
tests/test_gpu_term_pairs.py (a helper, not a test; tests/test_term_pairs_reference.py holds it to central differences, to
tests/pairs_reference.py's TableOptimizer and to a hand-computed example). Clamps are decided in float32, as in pairs_reference.

The objective itself is pairs_reference.pair_forward on W: the reference instantiates one class for both tables. What differs is the
table it lands in: the words table also takes the text objective's list, whose n gradient rows each go to `window` ids with per-entry
weights (cpp/storage.cu:37-49), and whose per-source means of squares are scattered into v with the SAME window and weights
(cpp/updates_adam.cu:242-252) — linearly in the weight, not squared."""
import numpy as np

from tests import pairs_reference as ref

BETA1, BETA2, EPSILON = ref.BETA1, ref.BETA2, ref.EPSILON


def term_pair_forward(W, pairs, weights=None, clip=True, scale=1.0):
    """pair_forward on the words table: probs [M], cost, multipliers [M] (scale included), grad [2M, dw], ids [2M]."""
    return ref.pair_forward(W, pairs, weights, clip, scale)


def term_pair_cost(W, pairs, weights=None, clip=True):
    return ref.pair_forward(W, pairs, weights, clip)["cost"]


def mixed_cost(cost_text, cost_pairs):
    """AverageFn over the two forward results: an unweighted mean."""
    return (cost_text + cost_pairs) / 2.0


def _norm_list(item):
    """(grad [n, d], ids [n * window], window, weights [n * window] or None) in fp64 / int64; ids and weights source-major
    (entry s * window + j belongs to gradient row s: update_repr_kernel's blockIdx.x * gridDim.y + blockIdx.y)."""
    grad, ids, window, weights = item
    grad, ids = np.asarray(grad, np.float64), np.asarray(ids, np.int64).reshape(-1)
    assert ids.size == grad.shape[0] * window, (ids.size, grad.shape, window)          # storage.cu:82-85
    if weights is not None:
        weights = np.asarray(weights, np.float64).reshape(-1)
        assert weights.size == ids.size                                                  # storage.cu:75-77
    return grad, ids, int(window), weights


def scatter(S, lists, lr):
    """Every list's update_repr_kernel (cpp/storage.cu:37-49): S[ids[s·w + j]] += lr · weight[s·w + j] · grad[s]."""
    for grad, ids, window, weights in lists:
        rows = np.repeat(grad, window, axis=0)
        if weights is not None:
            rows = rows * weights[:, None]
        np.add.at(S, ids, lr * rows)


def dense_gradient(shape, lists):
    g = np.zeros(shape)
    scatter(g, [_norm_list(l) for l in lists], 1.0)
    return g


class WindowedTableOptimizer:
    """A table under one optimiser, updated from a LIST of windowed gradient lists — RepresentationsStorage::update
    (cpp/storage.cu:51-102) and the Representations updaters (cpp/updates.cu:36-48, updates_adagrad.cu:83-179,
    updates_adam.cu:132-385). method: sgd | adagrad | sparse_adam | dense_adam | full_adam. With window 1 and no weights every
    method is pairs_reference.TableOptimizer."""

    def __init__(self, P, method):
        self.P = np.array(P, np.float64)
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
    def _decay(lam, lr):
        return np.float64(np.float32(1.0 - np.float64(np.float32(lam)) * np.float64(np.float32(lr))))

    def _storage_update(self, S, lists, lr, lam):
        """cpp/storage.cu:51-102: one decay (1 - lam * lr) when lam > 0, then every list's scatter."""
        if lam > 0:
            S *= self._decay(lam, lr)
        scatter(S, lists, lr)

    @staticmethod
    def _mean_squares(lists):
        """Per-source means of squares, with the list's ids, window and weights (updates_adam.cu:220-247, updates_adagrad.cu:132-150)."""
        return [((g * g).sum(axis=1, keepdims=True) * np.exp(-np.log(g.shape[1])), ids, window, weights) for g, ids, window, weights in lists]

    def update(self, lists, lr, lam):
        lists = [_norm_list(l) for l in lists]
        P = self.P
        if self.method == "sgd":                                 # updates.cu:36-48
            self._storage_update(P, lists, lr, lam)
            return
        if self.method == "adagrad":                             # updates_adagrad.cu:99-179
            if len(lists) != 1:
                raise RuntimeError("Adagrad currently does not implement multiple gradients.")      # :108
            g, ids, window, weights = lists[0]
            a = self.a[:, None]
            self._storage_update(a, self._mean_squares(lists), 1.0, 0.0)                            # :136-158
            agg = self.a[ids].reshape(-1, window).sum(axis=1) / window                              # adagrad_update_kernel :83-97
            g = g / np.sqrt(agg + np.float64(EPSILON))[:, None]
            self._storage_update(P, [(g, ids, window, weights)], lr, lam)                           # :177-178
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
            v = self.v[:, None]
            self._storage_update(v, self._mean_squares(lists), one_m_b2, 1.0)                        # :216-252
        bc = np.float64(np.float32(np.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)))              # :285
        self.t += 1
        eps = np.float64(EPSILON)
        if self.method == "dense_adam":                                                              # :293-311
            P[...] = P * self._decay(lam, lr) + lr * bc * self.m / (np.sqrt(self.v)[:, None] + eps)
        elif full:                                                                                   # :312-328
            P[...] = P + lr * bc * self.m / (np.sqrt(self.v) + eps)
        else:                                                                                        # sparse, :332-384
            if len(lists) != 1:
                raise RuntimeError("Sparse Adam currently does not implement multiple gradients.")  # :348
            _, ids, window, weights = lists[0]
            agg_m = self.m[ids].reshape(-1, window, P.shape[1]).sum(axis=1) / window                 # adam_sparse_update_kernel :132-151
            agg_v = self.v[ids].reshape(-1, window).sum(axis=1) / window
            upd = bc * agg_m / (np.sqrt(agg_v) + eps)[:, None]
            self._storage_update(P, [(upd, ids, window, weights)], lr, lam)
