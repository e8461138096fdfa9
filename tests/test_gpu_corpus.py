"""-m gpu: training from an HBM-resident corpus — nvsm_corpus_upload and the *_windows calls (corpus.hip) against their
nvsm_batch twins.

The reference is always the twin call on ``expand_windows(corpus, refs, w)`` — the header's definition in numpy, checked on its
own by tests/test_corpus_abi.py — on a second handle built and initialised the same way, and equality is EXACT: float32 arrays
are compared as uint32. Nothing here has a tolerance: everything behind the expansion kernel is the twin's own code on an
ordinary device batch, so a difference of one bit is a bug."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd.model import pinned_copy
from tests.helpers import PARAMS, gpu_model

pytestmark = pytest.mark.gpu

METHODS = ["sgd", "adagrad", "sparse_adam", "dense_adam", "full_adam"]
LR = {"sgd": 0.1, "adagrad": 0.01, "sparse_adam": 0.001, "dense_adam": 0.001, "full_adam": 0.001}
ADAM_STATE = ["word_representations/m", "word_representations/v", "entity_representations/m", "entity_representations/v",
              "word_entity_mapping/s0_transform", "word_entity_mapping/s1_transform", "word_entity_mapping/s0_bias",
              "word_entity_mapping/s1_bias"]
# the optimiser state every update method keeps (as tests/test_gpu_dispatch.py lists it): each of these must exist and is compared
STATE = {"sgd": [], "adagrad": ["word_representations/a", "entity_representations/a", "word_entity_mapping/s0_transform"],
         "sparse_adam": ADAM_STATE, "dense_adam": ADAM_STATE, "full_adam": ADAM_STATE}


def small_spec(w=3, method="sgd", lam=0.01, **kw):
    spec = dict(num_words=60, num_entities=40, word_dim=24, entity_dim=20, window=w, num_random=4, update_method=method)
    spec["lambda"] = lam
    spec.update(kw)
    return spec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(a, b, what=""):
    assert np.array_equal(bits(a), bits(b)), what


def method_of(m):
    return [k for k, v in ca.UPDATE_METHODS.items() if v == (m.cfg.update_method, m.cfg.adam_mode)][0]


def state_of(m):
    """the four parameters and every state tensor of the handle's update method; a name the library does not know is an error"""
    return {n: m.get_param(n) for n in list(PARAMS) + STATE[method_of(m)]}


def assert_same_state(a, b):
    sa, sb = state_of(a), state_of(b)
    assert sa.keys() == sb.keys() and len(sa) == 4 + len(STATE[method_of(a)])
    for n in sa:
        assert_same_bits(sa[n], sb[n], n)
    assert a.rng_state == b.rng_state


def status_of(call):
    try:
        call()
    except ca.NvsmError as e:
        return e.status, str(e)
    return 0, ""


def hand_corpus(w, num_words=60, doc_weights=True, term_weights=True):
    """Documents of exactly w tokens, an empty document between two others, one long document, and a last document that ends
    at num_tokens."""
    rs = np.random.RandomState(100 + w)
    lengths = [w, w, 0, w, 5 * w + 7, w + 2]
    tokens = rs.randint(0, num_words, sum(lengths)).astype(np.int32)
    tokens[0], tokens[-1] = num_words - 1, num_words - 1           # the largest word id at both ends of the arena
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    dw = rs.uniform(0.25, 2.0, len(lengths)).astype(np.float32) if doc_weights else None
    tw = rs.uniform(0.25, 2.0, num_words).astype(np.float32) if term_weights else None
    return ca.Corpus(tokens, offsets, dw, tw)


def hand_refs(corpus, w, B, rs):
    """Position 0 and position len − w of each document that holds a window, a repeated reference, then random valid ones."""
    lengths = np.diff(corpus.doc_offsets)
    edge = []
    for d in np.nonzero(lengths >= w)[0]:
        edge += [(d, 0), (d, lengths[d] - w)]
    edge += [edge[-1], edge[0], edge[-1]]
    docs = np.nonzero(lengths >= w)[0]
    d = docs[rs.randint(0, docs.size, B)]
    rand = np.stack([d, (rs.uniform(0, 1, B) * (lengths[d] - w + 1)).astype(np.int64)], axis=1)
    refs = np.concatenate([np.array(edge, np.int64), rand])[:B] if B >= 5 else np.array(edge, np.int64)[-B:]
    return np.ascontiguousarray(refs, dtype=np.uint32)


def random_corpus(rs, num_words, num_documents, mean_len, zipf=False, doc_weights=True, term_weights=True):
    lengths = rs.poisson(mean_len, num_documents)
    lengths[rs.randint(0, num_documents, max(1, num_documents // 50))] = 0           # some empty documents
    n = int(lengths.sum())
    if zipf:
        p = 1.0 / np.arange(1, num_words + 1)
        tokens = rs.choice(num_words, size=n, p=p / p.sum()).astype(np.int32)
    else:
        tokens = rs.randint(0, num_words, n).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return ca.Corpus(tokens, offsets, rs.uniform(0.25, 2.0, num_documents).astype(np.float32) if doc_weights else None,
                     rs.uniform(0.25, 2.0, num_words).astype(np.float32) if term_weights else None)


def random_refs(corpus, w, n, rs):
    lengths = np.diff(corpus.doc_offsets)
    docs = np.nonzero(lengths >= w)[0]
    d = docs[rs.randint(0, docs.size, n)]
    pos = (rs.uniform(0, 1, n) * (lengths[d] - w + 1)).astype(np.int64)
    return np.ascontiguousarray(np.stack([d, pos], axis=1), dtype=np.uint32)


def twins(spec, B, seed=5, **extra):
    a, b = gpu_model(spec, B, **extra), gpu_model(spec, B, **extra)
    a.initialize(seed)
    b.initialize(seed)
    return a, b


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["both", "doc", "term", "none"])
@pytest.mark.parametrize("B", [1, 5, 1000, 4099])
@pytest.mark.parametrize("w", [1, 3, 10, 16])
def test_forward_equals_the_batch_twin(w, B, weights):
    corpus = hand_corpus(w, doc_weights=weights in ("both", "doc"), term_weights=weights in ("both", "term"))
    refs = hand_refs(corpus, w, B, np.random.RandomState(B + w))
    assert refs.shape == (B, 2)
    batch = ca.expand_windows(corpus, refs, w)
    win, ref = twins(small_spec(w), B)                 # host sampler: the negatives are drawn from the labels the host takes from refs
    win.upload_corpus(corpus)
    win.compute_cost_windows(refs)
    ref.compute_cost(batch)
    cw, cr = win.get_cost_f64(), ref.get_cost_f64()
    assert cw == cr and np.isfinite(cw)
    for name in ("phrase", "entity_ids", "probs"):
        assert_same_bits(win.get_tensor(name), ref.get_tensor(name), name)
    assert np.array_equal(win.get_tensor("entity_ids").reshape(B, -1)[:, 0], refs[:, 0].astype(np.float32))
    assert win.rng_state == ref.rng_state


# ---- 2. training --------------------------------------------------------------------------------------------------------------
def run_pair_of_trainings(spec, B, w, source, steps, sampler, corpus=None, extra_check=None):
    """`steps` deferred steps from slices of ONE plan buffer at alternating even and odd instance offsets; returns the handles."""
    rs = np.random.RandomState(11)
    corpus = corpus or hand_corpus(w, num_words=spec["num_words"])
    stride = B + 1                                            # slices start at instance 0, B + 1, 2 B + 2, ...: even, odd, even, ...
    plan = np.concatenate([hand_refs(corpus, w, stride, rs) for _ in range(steps)])
    win, ref = twins(spec, B, sampler=sampler)
    win.upload_corpus(corpus)
    keep = None
    if source == "pinned":
        keep = pinned_copy(plan)
        view = keep.array
    elif source == "pageable":
        view = plan
    else:
        import torch
        view = torch.from_numpy(plan.view(np.int32)).cuda()
    tw, tr = [], []
    for s in range(steps):
        piece = view[s * stride:s * stride + B]
        wb = ca.WindowBatch(piece)
        assert wb.on_device == (source == "device")
        if source == "pinned":                                  # an odd instance offset is only 8-byte aligned: the copy engine's
            assert (wb.as_struct().refs % 16 == 8) == bool(s % 2)
        tw.append(win.step_windows_deferred(wb, LR[spec["update_method"]]))
        tr.append(ref.step_deferred(ca.expand_windows(corpus, plan[s * stride:s * stride + B], w), LR[spec["update_method"]]))
    costs_w, costs_r = [win.deferred_cost(t) for t in tw], [ref.deferred_cost(t) for t in tr]
    assert_same_bits(np.array(costs_w, np.float32), np.array(costs_r, np.float32), "deferred costs")
    assert all(np.isfinite(costs_w))
    assert_same_state(win, ref)
    del keep
    return win, ref


@pytest.mark.parametrize("source", ["pinned", "pageable", "device"])
@pytest.mark.parametrize("sampler", [ca.SAMPLER_HOST_MINSTD, ca.SAMPLER_DEVICE], ids=["host_sampler", "device_sampler"])
@pytest.mark.parametrize("method", METHODS)
def test_six_training_steps_equal_the_batch_twin(method, sampler, source):
    run_pair_of_trainings(small_spec(3, method), 256, 3, source, 6, sampler)


@pytest.mark.parametrize("lazy", [True, False], ids=["NVSM_LAZY_MIN_MB=0", "NVSM_LAZY_DECAY=0"])
def test_batch_norm_hard_tanh_under_lazy_and_eager_decay(lazy, monkeypatch):
    # (a table decays lazily only when it has at least as many rows as a batch has entries: the tables of tests/test_gpu_lazy.py
    #  instead of the 60-word model, at its batch of 40)
    if lazy:
        monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    else:
        monkeypatch.setenv("NVSM_LAZY_DECAY", "0")
    spec = small_spec(3, "sparse_adam", lam=0.02, num_words=3000, num_entities=5000, batch_norm=True, nonlinearity="hard_tanh")
    corpus = random_corpus(np.random.RandomState(3), 3000, 4000, 12)
    win, ref = run_pair_of_trainings(spec, 40, 3, "pinned", 6, ca.SAMPLER_DEVICE, corpus=corpus)
    for m in (win, ref):
        assert ("words lazy" in m.describe()) == lazy and ("documents lazy" in m.describe()) == lazy


def test_poisoned_buffers(monkeypatch):
    monkeypatch.setenv("NVSM_POISON", "1")
    run_pair_of_trainings(small_spec(3, "dense_adam", batch_norm=True, nonlinearity="hard_tanh"), 256, 3, "pageable", 6, ca.SAMPLER_HOST_MINSTD)


# ---- 3. the product shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,steps", [(4096, 4), (51200, 3)])
def test_the_product_shapes(B, steps):
    nV, nD, w = 20000, 3000, 10
    spec = dict(num_words=nV, num_entities=nD, word_dim=300, entity_dim=256, window=w, num_random=16, batch_norm=True,
                nonlinearity="hard_tanh", update_method="sparse_adam")
    spec["lambda"] = 0.01
    rs = np.random.RandomState(B)
    corpus = random_corpus(rs, nV, nD, 100, zipf=True)                      # ~300 000 tokens
    assert 200_000 < corpus.num_tokens < 400_000
    win, ref = twins(spec, B, sampler=ca.SAMPLER_DEVICE)
    win.upload_corpus(corpus)
    for s in range(steps):
        refs = random_refs(corpus, w, B, rs)
        cw = win.step_windows(refs, 0.001, want_cost=True)
        cr = ref.step(ca.expand_windows(corpus, refs, w), 0.001, want_cost=True)
        assert np.float32(cw).view(np.uint32) == np.float32(cr).view(np.uint32) and np.isfinite(cw)
    assert_same_state(win, ref)


# ---- 4. staging reuse ---------------------------------------------------------------------------------------------------------
def test_24_queued_steps_alternating_batches_and_windows_reuse_the_staging_sets():
    B, w, steps = 256, 3, 24
    spec = small_spec(w, "sparse_adam")
    rs = np.random.RandomState(2)
    corpus = random_corpus(rs, 60, 40, 30)
    plan = pinned_copy(np.concatenate([random_refs(corpus, w, B, rs) for _ in range(steps)]))
    batches = []
    for s in range(steps):
        b = ca.expand_windows(corpus, plan.array[s * B:(s + 1) * B], w)
        pins = [pinned_copy(a) for a in (b.features, b.labels, b.feature_weights, b.weights)]
        batches.append((pins, ca.Batch(*[p.array for p in pins])))
    mixed, ref = twins(spec, B, sampler=ca.SAMPLER_DEVICE)
    mixed.upload_corpus(corpus)
    for s in range(steps):                                      # nothing in this loop waits for the device
        if s % 2:
            mixed.step_windows(plan.array[s * B:(s + 1) * B], 0.001)
        else:
            mixed.step(batches[s][1], 0.001)
        ref.step(batches[s][1], 0.001)
    assert mixed.get_cost() == ref.get_cost()
    assert_same_state(mixed, ref)


# ---- 5. replacing and freeing the corpus ----------------------------------------------------------------------------------------
def test_replacing_the_corpus_between_steps_and_freeing_it():
    B, w = 64, 3
    rs = np.random.RandomState(4)
    first, second = random_corpus(rs, 60, 40, 20), random_corpus(rs, 60, 25, 9, doc_weights=False)
    win, ref = twins(small_spec(w, "adagrad"), B)
    for corpus in (first, second, first):
        win.upload_corpus(corpus)                               # (queued steps still read the old one: the upload waits for them)
        for _ in range(2):
            refs = random_refs(corpus, w, B, rs)
            win.step_windows(refs, 0.01)
            ref.step(ca.expand_windows(corpus, refs, w), 0.01)
    assert_same_state(win, ref)
    assert "corpus=" in win.describe()
    win.upload_corpus(None)
    assert "corpus" not in win.describe()
    st, msg = status_of(lambda: win.step_windows(refs, 0.01))
    assert st == 1 and "nvsm_corpus_upload" in msg
    batch = ca.expand_windows(first, refs, w)
    win.step(batch, 0.01)
    ref.step(batch, 0.01)
    assert_same_state(win, ref)
    win.upload_corpus(None)                                     # freeing twice is fine


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["document", "end"])
def test_a_bad_reference_is_clamped_and_reported_once(bad):
    w = 3
    corpus = hand_corpus(w)
    spec = small_spec(w, "sgd", lam=0.0)
    win, ref = twins(spec, 8)
    win.upload_corpus(corpus)
    lengths = np.diff(corpus.doc_offsets)
    refs = np.array([[corpus.num_documents, 0]] if bad == "document" else [[4, lengths[4] - w + 1]], np.uint32)
    ids = np.array([0, 3, 5, 7, 9], np.int64)                   # the label a clamped window gets, and four negatives
    before = state_of(win)
    win.step_windows(refs, 0.1, entity_ids=ids)                 # queued: nothing has been waited for yet
    st, msg = status_of(win.synchronize)
    # NVSM_ERR_INVALID_ARGUMENT, as for every id of the index contract (include/cunvsm_amd.h)
    assert st == 1 and "window reference" in msg
    win.synchronize()                                           # reported once
    # the clamped window is word 0 x w with label 0 and their weights: the twin of exactly that batch
    clamped = ca.Batch(np.zeros(w, np.int64), np.zeros(1, np.int64), np.full(w, corpus.term_weights[0], np.float32), corpus.doc_weights[:1])
    ref.step(clamped, 0.1, entity_ids=ids)
    assert_same_state(win, ref)
    after = state_of(win)
    W0, W1 = (x["word_representations-representations"].reshape(60, 24) for x in (before, after))
    E0, E1 = (x["entity_representations-representations"].reshape(40, 20) for x in (before, after))
    assert np.array_equal(W0[1:], W1[1:]) and not np.array_equal(W0[0], W1[0])
    rest = np.setdiff1d(np.arange(40), ids)
    assert np.array_equal(E0[rest], E1[rest]) and not np.array_equal(E0[ids], E1[ids])
    # ... and the handle trains on
    good = hand_refs(corpus, w, 8, np.random.RandomState(0))
    cw = win.step_windows(good, 0.1, want_cost=True)
    cr = ref.step(ca.expand_windows(corpus, good, w), 0.1, want_cost=True)
    assert cw == cr and np.isfinite(cw)
    assert_same_state(win, ref)


@pytest.mark.parametrize("source", ["host", "device"])
def test_a_bad_reference_under_the_host_sampler_gets_label_0_on_the_host_too(source):
    """No entity_ids: the host takes the labels from the references (read back first when they are on the device) and must reach
    the device's verdict — label 0 for a bad reference — from its copy of the offsets, or the negatives and the generator would
    part from the twin of the clamped batch."""
    w, B = 3, 8
    corpus = hand_corpus(w)
    lengths = np.diff(corpus.doc_offsets)
    refs = hand_refs(corpus, w, B, np.random.RandomState(6))
    refs[2] = (corpus.num_documents + 3, 0)                     # no such document
    refs[5] = (4, lengths[4] - w + 1)                           # one token over the end of the long document
    refs[7] = (2, 0)                                            # the empty document holds no window
    bad = np.array([2, 5, 7])
    valid = refs.copy()
    valid[bad] = refs[0]
    batch = ca.expand_windows(corpus, valid, w)
    f, fw = batch.features.reshape(B, w), batch.feature_weights.reshape(B, w)
    f[bad], fw[bad], batch.labels[bad], batch.weights[bad] = 0, corpus.term_weights[0], 0, corpus.doc_weights[0]
    win, ref = twins(small_spec(w, "sgd", lam=0.0), B, sampler=ca.SAMPLER_HOST_MINSTD)
    win.upload_corpus(corpus)
    if source == "device":
        import torch
        given = torch.from_numpy(refs.view(np.int32)).cuda()
    else:
        given = refs
    for step in range(2):
        win.step_windows(given, 0.1)
        st, msg = status_of(win.synchronize)
        assert st == 1 and "window reference" in msg
        ref.step(batch, 0.1)
        ids_w, ids_r = win.get_tensor("entity_ids").reshape(B, -1), ref.get_tensor("entity_ids").reshape(B, -1)
        assert np.array_equal(ids_w, ids_r) and np.all(ids_w[bad, 0] == 0)
        assert_same_state(win, ref)


def test_a_refused_upload_leaves_the_earlier_corpus_in_place():
    w, B = 3, 8
    corpus = hand_corpus(w)
    win, ref = twins(small_spec(w, "sparse_adam"), B)
    win.upload_corpus(corpus)
    before = win.describe()
    worse = ca.Corpus(np.array([1, 2, 60, 3], np.int32), [0, 4])            # word 60 of 60
    st, msg = status_of(lambda: win.upload_corpus(worse))
    assert st == 1 and "token" in msg
    assert win.describe() == before
    refs = hand_refs(corpus, w, B, np.random.RandomState(9))
    win.step_windows(refs, 0.001)
    ref.step(ca.expand_windows(corpus, refs, w), 0.001)
    assert_same_state(win, ref)


def test_upload_errors_name_their_field():
    m = gpu_model(small_spec(), 8)
    L = ca.lib()
    tokens = np.arange(12, dtype=np.int32)

    def upload(tok, offsets, num_tokens=None, num_documents=None):
        off = np.asarray(offsets, np.int64)
        c = ca.NvsmCorpus(tok.ctypes.data, off.ctypes.data, None, None, tok.size if num_tokens is None else num_tokens,
                          off.size - 1 if num_documents is None else num_documents)
        return L.nvsm_corpus_upload(m._h, C.byref(c)), L.nvsm_last_error().decode()

    st, msg = upload(tokens, [1, 4, 12])
    assert st == 1 and "doc_offsets must start at 0" in msg
    st, msg = upload(tokens, [0, 7, 4, 12])
    assert st == 1 and "doc_offsets must not decrease" in msg
    st, msg = upload(tokens, [0, 4, 11])
    assert st == 1 and "last of doc_offsets" in msg and "num_tokens" in msg
    st, msg = upload(tokens, np.concatenate([np.zeros(41, np.int64), [12]]))
    assert st == 1 and "num_documents" in msg and "num_entities" in msg
    for value in (60, -1):
        bad = tokens.copy()
        bad[7] = value
        st, msg = upload(bad, [0, 4, 12])
        assert st == 1 and "token" in msg and "num_words" in msg
    c = ca.NvsmCorpus(tokens.ctypes.data, None, None, None, 12, 2)
    assert L.nvsm_corpus_upload(m._h, C.byref(c)) == 1 and "doc_offsets" in L.nvsm_last_error().decode()
    assert "corpus" not in m.describe()                          # none of them left a corpus behind
    assert upload(tokens, [0, 4, 12])[0] == 0 and "corpus=" in m.describe()
    assert upload(np.zeros(0, np.int32), [0])[0] == 0            # an empty corpus is a corpus: every reference into it is bad
    m.step_windows(np.zeros((2, 2), np.uint32), 0.1)
    st, msg = status_of(m.synchronize)
    assert st == 1 and "window reference" in msg


def test_calls_without_a_corpus_and_under_data_parallelism_are_refused():
    refs = np.zeros((4, 2), np.uint32)
    m = gpu_model(small_spec(), 8)
    for call in (lambda: m.compute_cost_windows(refs), lambda: m.step_windows(refs, 0.1), lambda: m.step_windows_deferred(refs, 0.1)):
        st, msg = status_of(call)
        assert st == 1 and "nvsm_corpus_upload" in msg
    corpus = hand_corpus(3)
    m.upload_corpus(corpus)
    st, msg = status_of(lambda: m.step_windows(np.zeros((9, 2), np.uint32), 0.1))
    assert st == 1 and "num_instances" in msg
    dp = gpu_model(small_spec(), 8, world_size=2, rank=0)
    dp.upload_corpus(corpus)
    for call in (lambda: dp.compute_cost_windows(refs), lambda: dp.step_windows(refs, 0.1), lambda: dp.step_windows_deferred(refs, 0.1)):
        st, msg = status_of(call)
        assert st == 2 and "world_size" in msg
    dp.upload_corpus(None)                                       # the handle stays usable
    m.step_windows(hand_refs(corpus, 3, 8, np.random.RandomState(1)), 0.1)
    assert np.isfinite(m.get_cost())


# ---- 7. no change for others --------------------------------------------------------------------------------------------------
def test_describe_of_a_handle_without_a_corpus_does_not_change():
    plain, other = gpu_model(small_spec(), 8), gpu_model(small_spec(), 8)
    before = plain.describe()
    assert "corpus" not in before
    other.upload_corpus(hand_corpus(3))
    assert plain.describe() == before
    d = other.describe()
    assert "corpus=" in d and d[:d.index(" | corpus=")] + d[d.index(" | switches"):] == before
