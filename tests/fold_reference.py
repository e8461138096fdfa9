"""A numpy fp64 restatement of one fold-in step's update (nvsm_step_fold), and the procedure that DEFINES the
feature on the CPU oracle: a full step, then the frozen parameters put back.

The restatement works from what the loss kernel leaves behind — proj [B][de], the signed multipliers coef [B*R], pp [B] =
mean_t(proj²), the document ids [B*R] — and the state of the rows that train. It is held to the oracle by
tests/test_fold_reference.py, and the GPU tests (tests/test_gpu_fold.py) use both."""
import numpy as np

from tests.helpers import PARAMS

E = PARAMS[1]
FROZEN = (PARAMS[0], PARAMS[2], PARAMS[3])
METHOD_NAMES = ("sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-6      # the oracle's (oracle/nvsm_oracle.hpp Config): doubles; the engine's are the floats next to them


def oracle_state_names(method):
    """(engine name, oracle name, per-row scalar?) of the documents table's optimiser state."""
    if method == "sgd":
        return []
    if method == "adagrad":
        return [("entity_representations/a", "entities.s0", True)]
    return [("entity_representations/m", "entities.s0", False), ("entity_representations/v", "entities.s1", method != "full_adam")]


def row_sums(proj, coef, pp, ids, R, rows):
    """g [rows][de] = Σ coef[e]·proj[e // R], q [rows] = Σ coef[e]²·pp[e // R], cnt [rows] over the entries e with ids[e] = row."""
    proj = np.asarray(proj, np.float64)
    coef = np.asarray(coef, np.float64).ravel()
    pp = np.asarray(pp, np.float64).ravel()
    ids = np.asarray(ids, np.int64).ravel()
    src = np.arange(ids.size) // R
    g = np.zeros((rows, proj.shape[1]))
    np.add.at(g, ids, coef[:, None] * proj[src])
    q = np.zeros(rows)
    np.add.at(q, ids, coef * coef * pp[src])
    cnt = np.bincount(ids, minlength=rows).astype(np.float64)
    return g, q, cnt


def fold_update(method, P, state, g, q, cnt, n0, lr, sl, t):
    """One fold step's update of rows >= n0, in place, fp64. P [rows][de]; state: "m" [rows][de], "v" [rows] or [rows][de], "a" [rows]
    as the method has them; g, q, cnt: row_sums; sl: the scaled lambda (λ / B); t: the documents table's Adam step counter (from 1).
    The row formulas are cpp/storage.cu:51-102, updates_adagrad.cu:99-179, updates_adam.cu:153-385 for a table whose every entry is a
    gradient list of window 1 — what Model::update_entities applies — restricted to the rows that train."""
    r = slice(n0, P.shape[0])
    decay = 1.0 - sl * lr if sl > 0 else 1.0
    if method == "sgd":
        P[r] = P[r] * decay + lr * g[r]
        return
    if method == "adagrad":
        state["a"][r] += q[r]
        P[r] = P[r] * decay + lr * g[r] / np.sqrt(state["a"][r] + EPS)[:, None]
        return
    one_m_b1, one_m_b2 = 1.0 - BETA1, 1.0 - BETA2
    s_m, s_v = 1.0 - one_m_b1, 1.0 - one_m_b2
    bc = np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)
    m, v = state["m"], state["v"]
    m[r] = m[r] * s_m + one_m_b1 * g[r]
    if method == "full_adam":
        m[r] += -(one_m_b1 * sl) * P[r]
        ag = g[r] - sl * P[r]
        v[r] = v[r] * s_v + ag * ag * one_m_b2
        P[r] = P[r] + (m[r] / (np.sqrt(v[r]) + EPS)) * bc * lr
        return
    v[r] = v[r] * s_v + one_m_b2 * q[r]
    denom = (np.sqrt(v[r]) + EPS)[:, None]
    if method == "sparse_adam":
        P[r] = P[r] * decay + lr * cnt[r][:, None] * (bc * m[r] / denom)
    else:
        P[r] = P[r] * (1.0 - sl * lr) + (m[r] / denom) * bc * lr


def oracle_sums(o, ids, R, rows):
    """row_sums of the oracle's current forward / backward result (the oracle keeps |multiplier| and negates the entity rows)."""
    proj = o.get("proj")
    de = proj.size // (np.asarray(ids).size // R)
    proj = proj.reshape(-1, de)
    sign = np.where(np.arange(np.asarray(ids).size) % R == 0, 1.0, -1.0)
    coef = o.get("multipliers") * sign
    pp = (proj * proj).sum(axis=1) * np.exp(-np.log(float(de)))
    return row_sums(proj, coef, pp, ids, R, rows)


def oracle_fold_step(o, words, ww, ids, iw, n0, lr):
    """THE DEFINITION: the oracle's full forward / backward / update, then W, T, b and rows < n0 of E put back. Returns the cost.
    (The frozen rows' optimiser state moves in the oracle; every row's update is local to the row, so rows >= n0 do not see it.)"""
    keep = {p: o.get(p).copy() for p in PARAMS}
    o.forward(words, ww, ids, iw)
    o.backward()
    cost = o.get_cost()
    o.update(lr)
    for p in FROZEN:
        o.set(p, keep[p])
    e = o.get(E).copy()
    de = o.get(PARAMS[3]).size
    e[:n0 * de] = keep[E][:n0 * de]
    o.set(E, e)
    return cost
