"""CPU: the row order of the n-gram stack, its limit, and the cases of tests/test_gpu_ngrams.py vetted against the RANK CORRECTNESS
RULE of tests/test_gpu_rank.py before a GPU sees them.

For every case s64 and err32 come from the REFERENCE chain (mean, @ T, + c·b, f: fp64, and a float32 numpy evaluation of the same
formula), tol = 4·err32; the float32 evaluation of the library's REASSOCIATED chain (G = W[S] @ T once, 0.5·(G[a] + G[b]) + c·b) must
pass check_result — reassociating costs no more than the rule allows — and the narrow-band precondition must hold with the tolerance
DOUBLED, as tests/test_gpu_neighbors.py does, because numpy's float32 error differs between hosts. A case that fails here is replaced
(another seed offset, another shape), not loosened."""
import itertools

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import ngram_reference as ref
from tests.test_gpu_ngrams import CASES
from tests.test_gpu_rank import band_is_narrow, check_result, ref_scores


def stack(m):
    return [(a, -1) for a in range(m)] + list(itertools.combinations(range(m), 2))


@pytest.mark.parametrize("m", [1, 2, 3, 5, 100])
def test_encode_and_decode_round_trip_in_combinations_order(m):
    want = np.array(stack(m), np.int64)
    R = len(want)
    assert ca.ngram_rows(m, 2) == R and ca.ngram_rows(m, 1) == m
    np.testing.assert_array_equal(ref.phrase_positions(m, 2), want)
    np.testing.assert_array_equal(ref.phrase_positions(m, 1), want[:m])
    np.testing.assert_array_equal(ca.ngram_decode(np.arange(R), m), want)
    np.testing.assert_array_equal(ca.ngram_encode(want, m), np.arange(R))
    np.testing.assert_array_equal(ca.ngram_decode(np.arange(m), m, 1), want[:m, :1])
    np.testing.assert_array_equal(ca.ngram_encode(want[:m, :1], m), np.arange(m))
    np.testing.assert_array_equal(ca.ngram_decode([-1, 0], m), [[-1, -1], [0, -1]])
    assert ca.ngram_decode(np.zeros((2, 3), np.int64), m).shape == (2, 3, 2)


@pytest.mark.parametrize("m", [2, 3, 5, 100, 65535])
def test_every_run_begins_and_ends_where_the_formula_says(m):
    R = ca.ngram_rows(m, 2)
    assert R == m + m * (m - 1) // 2
    a = np.arange(m - 1, dtype=np.int64)
    first = m + a * (2 * m - a - 1) // 2
    last = first + (m - a - 2)
    assert first[0] == m and last[-1] == R - 1 and (first[1:] == last[:-1] + 1).all()
    np.testing.assert_array_equal(ca.ngram_decode(first, m), np.stack([a, a + 1], 1))
    np.testing.assert_array_equal(ca.ngram_decode(last, m), np.stack([a, np.full_like(a, m - 1)], 1))
    np.testing.assert_array_equal(ca.ngram_encode(np.stack([a, a + 1], 1), m), first)
    np.testing.assert_array_equal(ca.ngram_encode(np.stack([a, np.full_like(a, m - 1)], 1), m), last)
    np.testing.assert_array_equal(ca.ngram_decode([m - 1, m, R - 1], m), [[m - 1, -1], [0, 1], [m - 2, m - 1]])


def test_the_row_limit():
    L = ca.lib()
    for m, c in ((1, 1), (1, 2), (7, 1), (7, 2), (65535, 2), (65536, 1), ((1 << 31) - 1, 1)):
        want = m if c == 1 else m + m * (m - 1) // 2
        assert ca.ngram_rows(m, c) == want == L.nvsm_ngram_rows(m, c) and want < 1 << 31
    for m, c in ((65536, 2), (1 << 31, 1), (1 << 40, 2), (0, 1), (-3, 2), (5, 0), (5, 3)):
        assert ca.ngram_rows(m, c) == -1 == L.nvsm_ngram_rows(m, c), (m, c)
    with pytest.raises(ValueError):
        ca.ngram_decode([0], 65536)
    with pytest.raises(ValueError):
        ca.ngram_decode([15], 5)
    with pytest.raises(ValueError):
        ca.ngram_encode([[3, 2]], 5)
    with pytest.raises(ValueError):
        ca.ngram_encode([[3, 5]], 5)


def test_the_two_chains_agree_and_the_generator_is_the_library_chain():
    case = CASES[3]
    spec, params, vocabulary, queries = ref.case_inputs(case)
    for act in ("identity", "hard_tanh", "tanh"):
        for c in (0.0, 0.5, 1.0):
            X = ref.reference_rows(params, spec, vocabulary, 2, c, act, np.float64)
            L = ref.library_rows(params, spec, vocabulary, 2, c, act, np.float64)
            assert X.shape == L.shape == (ca.ngram_rows(len(vocabulary), 2), spec["entity_dim"])
            assert np.abs(X - L).max() < 1e-13
            if act != "tanh":                      # the generator's float32 steps, from the float32 G of the library chain
                W, T, b = ref.model_arrays(params, spec, np.float32)
                G = W[vocabulary] @ T
                got = ref.generator_rows(G, b, c, act, 0, X.shape[0])
                assert np.abs(got - L).max() < 1e-5
                np.testing.assert_array_equal(ref.generator_rows(G, b, c, act, 70, 33), got[70:103])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "V%d-m%d-de%d-Q%d-k%d-%s-%s-card%d-%s" % (c[0], c[1], c[3], c[4], c[5], c[6], c[8], c[11], c[12]))
def test_every_gpu_case_obeys_the_rule_on_the_cpu(case):
    V, m, dw, de, Q, k, act, c, sim, slab_mb, vkind, card, qkind, offset = case
    spec, params, vocabulary, queries = ref.case_inputs(case)
    assert len(vocabulary) == m and (np.diff(vocabulary) > 0).all()
    s64, err32, tol, lib32 = ref.case_scores(case, spec, params, vocabulary, queries, ref_scores)
    R = ca.ngram_rows(m, card)
    assert s64.shape == lib32.shape == (Q, R) and 1 <= k <= R
    for q in range(Q):
        band_is_narrow(s64[q], np.arange(R), k, 2 * tol)
    worst = check_result(ref.top_k(lib32, k), s64, k, tol)
    assert worst <= tol
