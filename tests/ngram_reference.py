"""numpy restatement of the n-gram search in document space (include/cunvsm_amd.h nvsm_ngram_search; py/nvsm/base.py:106-162), in
fp64 and in float32. No test in here: tests/test_ngram_reference.py (CPU) and tests/test_gpu_ngrams.py (-m gpu) import it.

  phrase rows      for k = 1 .. max_cardinality the k-combinations of the vocabulary's positions, straight from
                   itertools.combinations, stacked (np.vstack(reprs), base.py:140)
  reference chain  mean of the k word rows, then @ T, then + c·b, then f (Model.infer of the mean vector, no batch normalisation)
  library chain    G = W[S] @ T once; 1-gram f(G[a] + c·b); 2-gram f(0.5·(G[a] + G[b]) + c·b): the projection is linear before the bias
  generator        the library chain's last step from a given float32 G, operation for operation as csrc/ngram.hip performs it, with
                   the nextafter-widened hard_tanh bounds of the kernels: what nvsm_debug_ngram_rows must return bit for bit"""
import itertools

import numpy as np

W_NAME, E_NAME, T_NAME, B_NAME = ("word_representations-representations", "entity_representations-representations",
                                  "word_entity_mapping-transform", "word_entity_mapping-bias")


def phrase_positions(m, max_cardinality):
    """[R][2] int64: positions (a, b) in the vocabulary of every phrase row, b = -1 for a 1-gram — itertools.combinations order"""
    rows = []
    for k in range(1, max_cardinality + 1):
        for combo in itertools.combinations(range(m), k):
            rows.append(tuple(combo) + (-1,) * (2 - k))
    return np.array(rows, dtype=np.int64).reshape(-1, 2)


def activation(pre, act):
    if act == "tanh":
        return np.tanh(pre)
    if act == "hard_tanh":
        return np.clip(pre, -1, 1)
    assert act == "identity", act
    return pre


def model_arrays(params, spec, dtype):
    dw, de = spec["word_dim"], spec["entity_dim"]
    W = params[W_NAME].reshape(-1, dw).astype(dtype)
    T = params[T_NAME].reshape(dw, de).astype(dtype)          # stored T[r + de·c]: [c][r]
    return W, T, params[B_NAME].astype(dtype)


def reference_rows(params, spec, vocabulary, max_cardinality, c, act, dtype):
    """[R][d_e]: the reference chain for every phrase row, everything in `dtype`"""
    W, T, b = model_arrays(params, spec, dtype)
    Ws = W[np.asarray(vocabulary, np.int64)]
    out = []
    for k in range(1, max_cardinality + 1):
        idx = np.array(list(itertools.combinations(range(Ws.shape[0]), k)), dtype=np.int64).reshape(-1)
        if idx.size == 0:
            continue
        phrase = Ws[idx].reshape(-1, k, Ws.shape[1]).mean(axis=1, dtype=dtype)
        out.append(activation(phrase @ T + dtype(c) * b, act))
    return np.vstack(out)


def library_rows(params, spec, vocabulary, max_cardinality, c, act, dtype):
    """[R][d_e]: the library's reassociated chain, everything in `dtype`"""
    W, T, b = model_arrays(params, spec, dtype)
    G = W[np.asarray(vocabulary, np.int64)] @ T
    pos = phrase_positions(G.shape[0], max_cardinality)
    one = pos[:, 1] < 0
    pre = np.where(one[:, None], G[pos[:, 0]], dtype(0.5) * (G[pos[:, 0]] + G[np.maximum(pos[:, 1], 0)]))
    return activation(pre + dtype(c) * b, act)


def projected_words(params, spec, word_ids, c, act, dtype):
    """f(T·W[w] + c·b) of single words: the query side for projected-word ids"""
    W, T, b = model_arrays(params, spec, dtype)
    return activation(W[np.asarray(word_ids, np.int64)] @ T + dtype(c) * b, act)


CLIP_LO, CLIP_HI = np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(1), np.float32(2))


def generator_rows(G, bias, c, act, p0, S):
    """float32 [S][d_e]: phrase rows p0 .. p0 + S from a float32 G [m][d_e] as ngram_rows_kernel computes them. Every operation is a
    single float32 rounding whether or not a compiler contracts it, for c in {0, 0.5, 1}: x + y rounds once, 0.5·(x + y) is exact,
    c·b is exact, and the last addition rounds once (an fma of exact products rounds the same sum). c = 0 adds nothing (the
    quirk of nvsm_rank_options). Not for tanh: that is no single rounding."""
    assert G.dtype == np.float32 and bias.dtype == np.float32 and act in ("identity", "hard_tanh") and c in (0.0, 0.5, 1.0)
    pos = phrase_positions(G.shape[0], 2)[p0:p0 + S]
    one = pos[:, 1] < 0
    v = np.where(one[:, None], G[pos[:, 0]], np.float32(0.5) * (G[pos[:, 0]] + G[np.maximum(pos[:, 1], 0)])).astype(np.float32)
    if c != 0.0:
        v = (v + (np.float32(c) * bias).astype(np.float32)).astype(np.float32)
    if act == "hard_tanh":
        v = np.minimum(np.maximum(v, CLIP_LO), CLIP_HI)
    return v


def top_k(scores, k):
    """(ids [Q][k], scores [Q][k], counts [Q]) of a score matrix: score descending, ties by ascending row"""
    Q, R = scores.shape
    ids = np.empty((Q, k), np.int64)
    for q in range(Q):
        ids[q] = np.lexsort((np.arange(R), -scores[q].astype(np.float64)))[:k]
    return ids, np.take_along_axis(scores, ids, 1), np.full(Q, min(k, R), np.int64)


# ---- the inputs of an end-to-end case: shared by the GPU test and by the CPU test that vets the cases ----------------------------
def case_inputs(case):
    """spec, params, vocabulary (int64 positions -> word ids), and the three kinds of queries of a case of tests/test_gpu_ngrams.py
    CASES: (V, m, dw, de, Q, k, act, c, sim, slab_mb, vocabulary kind, max_cardinality, query kind, seed offset)"""
    V, m, dw, de, Q, k, act, c, sim, slab_mb, vkind, card, qkind, offset = case
    D = 200
    rs = np.random.RandomState(7 * V + 3 * m + dw + de + Q + k % 97 + offset)
    spec = dict(num_words=V, num_entities=D, word_dim=dw, entity_dim=de, window=2, num_random=1,
                nonlinearity="hard_tanh" if act == "hard_tanh" else "tanh", batch_norm=True, update_method="sgd")
    params = {W_NAME: rs.uniform(-1, 1, V * dw).astype(np.float32),
              E_NAME: rs.standard_normal(D * de).astype(np.float32),
              T_NAME: (rs.uniform(-1, 1, dw * de) * 2.0 * np.sqrt(6.0 / (dw + de))).astype(np.float32),
              B_NAME: rs.uniform(-0.1, 0.1, de).astype(np.float32)}
    if vkind == "all":
        assert m == V
        vocabulary = np.arange(V, dtype=np.int64)
    else:                                                      # a subset with gaps
        vocabulary = np.sort(rs.choice(V, m, replace=False)).astype(np.int64)
        assert m < 2 or (np.diff(vocabulary) > 1).any()
    queries = dict(entity_ids=rs.choice(D, Q, replace=Q > D).astype(np.int64), word_ids=rs.choice(V, Q, replace=Q > V).astype(np.int64),
                   vectors=rs.standard_normal((Q, de)).astype(np.float32))
    return spec, params, vocabulary, queries


def case_scores(case, spec, params, vocabulary, queries, ref_scores):
    """s64, err32, tol = 4·err32 of the REFERENCE chain (fp64 against a float32 numpy evaluation of the same formula), and the
    float32 scores of the LIBRARY chain; ref_scores: tests/test_gpu_rank.py's scoring restatement"""
    V, m, dw, de, Q, k, act, c, sim, slab_mb, vkind, card, qkind, offset = case
    fact = spec["nonlinearity"] if act == "model" else act
    X64 = reference_rows(params, spec, vocabulary, card, c, fact, np.float64)
    X32 = reference_rows(params, spec, vocabulary, card, c, fact, np.float32)
    L32 = library_rows(params, spec, vocabulary, card, c, fact, np.float32)
    if qkind == "entity_ids":
        P64 = P32 = params[E_NAME].reshape(-1, de)[queries["entity_ids"]]
    elif qkind == "word_ids":
        P64 = projected_words(params, spec, queries["word_ids"], c, fact, np.float64)
        P32 = projected_words(params, spec, queries["word_ids"], c, fact, np.float32)
    else:
        P64 = P32 = queries["vectors"]
    s64 = ref_scores(P64, X64, sim, np.float64)
    s32 = ref_scores(P32, X32, sim, np.float32)
    err32 = float(np.abs(s32.astype(np.float64) - s64).max())
    return s64, err32, 4.0 * max(err32, 1e-45), ref_scores(P32, L32, sim, np.float32)
