"""Host-side mirror of ``Model<TextEntity::Objective>`` and ``TextEntity::Batch`` over the C ABI.

Same method names and argument meaning as the reference (include/cuNVSM/model.h:97-115):
``initialize``, ``compute_cost``, ``compute_gradients``, ``update``, ``get_cost``; the forward result
and the gradients live inside the handle (the reference returns owning pointers, cpp/main.cu:405-411).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NvsmBatch, NvsmConfig, NvsmCorpus, NvsmWindowBatch, NvsmMixture, NvsmPairBatch, NvsmNeighborOptions, NvsmNeighborQueries, NvsmNgramOptions, NvsmTsneOptions, NvsmTsneSparseOptions, NvsmKmeansOptions, NvsmJudgments, NvsmQueries, NvsmRankOptions, check, lib

# --update_method of the reference CLI (cpp/main.cu:479-485)
UPDATE_METHODS = {
    "sgd": (_lib.SGD, _lib.ADAM_NONE),
    "adagrad": (_lib.ADAGRAD, _lib.ADAM_NONE),
    "sparse_adam": (_lib.ADAM, _lib.ADAM_SPARSE),
    "dense_adam": (_lib.ADAM, _lib.ADAM_DENSE_UPDATE),
    "full_adam": (_lib.ADAM, _lib.ADAM_DENSE_UPDATE_DENSE_VARIANCE),
}
NONLINEARITIES = {"tanh": _lib.TANH, "hard_tanh": _lib.HARD_TANH}      # cpp/main.cu:487-490

PARAM_NAMES = (
    "word_representations-representations",
    "entity_representations-representations",
    "word_entity_mapping-transform",
    "word_entity_mapping-bias",
)


def default_config(**overrides):
    """nvsm_config with the reference CLI defaults, then keyword overrides.
    ``update_method`` / ``nonlinearity`` accept the CLI strings."""
    cfg = NvsmConfig()
    lib().nvsm_config_default(C.byref(cfg))
    for k, v in overrides.items():
        if k == "update_method" and isinstance(v, str):
            cfg.update_method, cfg.adam_mode = UPDATE_METHODS[v]
        elif k == "nonlinearity" and isinstance(v, str):
            cfg.nonlinearity = NONLINEARITIES[v]
        else:
            if not hasattr(cfg, k):
                raise AttributeError("nvsm_config has no field %r" % k)
            setattr(cfg, k, int(v) if isinstance(v, (bool, np.bool_)) else v)
    return cfg


class PinnedArray:
    """A numpy array over page-locked host memory from nvsm_host_alloc — what the reference's Batch allocates with
    cudaHostAlloc (cpp/data.cu:8-40): host→device copies from it are asynchronous. `.array` is the numpy view."""

    def __init__(self, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        self._ptr = C.c_void_p()
        check(lib().nvsm_host_alloc(max(1, n * dtype.itemsize), C.byref(self._ptr)))
        buf = (C.c_char * (n * dtype.itemsize)).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

    def __del__(self):
        try:
            if self._ptr:
                lib().nvsm_host_free(self._ptr)
                self._ptr = None
        except Exception:   # pragma: no cover  (interpreter shutdown)
            pass


def pinned_copy(a):
    """Copy of `a` in page-locked memory; keep the returned PinnedArray alive as long as its .array is in use."""
    a = np.asarray(a)
    p = PinnedArray(a.shape, a.dtype)
    p.array[...] = a
    return p


class Batch:
    """TextEntity::Batch (include/cuNVSM/data.h:114-177): features [B*w] int64, feature_weights [B*w] float,
    labels [B] int64, weights [B] float. Arrays may be numpy (host) or torch CUDA tensors (already in HBM)."""

    def __init__(self, features, labels, feature_weights=None, weights=None):
        self.features, self.labels = features, labels
        self.feature_weights, self.weights = feature_weights, weights
        self.on_device = hasattr(features, "data_ptr")
        if self.on_device:
            import torch
            assert features.dtype == torch.int64 and labels.dtype == torch.int64
            for t in (feature_weights, weights):
                assert t is None or t.dtype == torch.float32
            self.num_instances = int(labels.numel())
        else:
            self.features = np.ascontiguousarray(features, dtype=np.int64)
            self.labels = np.ascontiguousarray(labels, dtype=np.int64)
            if feature_weights is not None:
                self.feature_weights = np.ascontiguousarray(feature_weights, dtype=np.float32)
            if weights is not None:
                self.weights = np.ascontiguousarray(weights, dtype=np.float32)
            self.num_instances = int(self.labels.size)

    def _ptr(self, a):
        if a is None:
            return None
        return a.data_ptr() if self.on_device else a.ctypes.data

    def check_shapes(self, window_size):
        """The ABI takes bare pointers: the element counts it will read are asserted here (include/cunvsm_amd.h,
        index contract). Id RANGES are checked on the device."""
        size = (lambda a: int(a.numel())) if self.on_device else (lambda a: int(a.size))
        B = self.num_instances
        if size(self.features) != B * window_size:
            raise ValueError("features holds %d ids, expected num_instances * window_size = %d" % (size(self.features), B * window_size))
        if self.feature_weights is not None and size(self.feature_weights) != B * window_size:
            raise ValueError("feature_weights holds %d values, expected %d" % (size(self.feature_weights), B * window_size))
        if self.weights is not None and size(self.weights) != B:
            raise ValueError("weights holds %d values, expected %d" % (size(self.weights), B))

    def as_struct(self):
        return NvsmBatch(self._ptr(self.features), self._ptr(self.feature_weights), self._ptr(self.labels),
                         self._ptr(self.weights), self.num_instances, int(self.on_device))


class PairBatch:
    """nvsm_pair_batch — the batch of the entity-entity similarity objective (RepresentationSimilarity::Batch,
    cpp/data.cu:316-334): M pairs of document ids, given as an [M, 2] array (or flat, interleaved a_0 b_0 a_1 b_1 ...), and
    optional weights [M]. Arrays may be numpy (host) or torch CUDA tensors. Element counts are checked here; id RANGES on the device."""

    def __init__(self, pairs, weights=None):
        self.on_device = hasattr(pairs, "data_ptr")
        if self.on_device:
            import torch
            if pairs.dtype != torch.int64:
                raise ValueError("pairs must be int64")
            if weights is not None and weights.dtype != torch.float32:
                raise ValueError("weights must be float32")
            if not pairs.is_contiguous() or (weights is not None and not weights.is_contiguous()):
                raise ValueError("device arrays must be contiguous")
            shape, n = tuple(pairs.shape), int(pairs.numel())
            wn = None if weights is None else int(weights.numel())
            self.pairs, self.weights = pairs, weights
        else:
            a = np.asarray(pairs)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("pairs must hold integer document ids")
            shape, n = a.shape, int(a.size)
            self.pairs = np.ascontiguousarray(a, dtype=np.int64).ravel()
            self.weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).ravel()
            wn = None if weights is None else int(self.weights.size)
        if len(shape) == 2 and shape[1] != 2:
            raise ValueError("pairs has shape %s, expected [num_pairs][2]" % (shape,))
        if len(shape) not in (1, 2) or n % 2 != 0:
            raise ValueError("pairs must be [num_pairs][2] or a flat, interleaved list of 2 * num_pairs ids")
        self.num_pairs = n // 2
        if self.num_pairs < 1:
            raise ValueError("pairs is empty: a pair batch needs at least one pair")
        if wn is not None and wn != self.num_pairs:
            raise ValueError("weights holds %d values, expected num_pairs = %d" % (wn, self.num_pairs))

    def _ptr(self, a):
        if a is None:
            return None
        return a.data_ptr() if self.on_device else a.ctypes.data

    def as_struct(self):
        return NvsmPairBatch(self._ptr(self.pairs), self._ptr(self.weights), self.num_pairs, int(self.on_device))


class Corpus:
    """nvsm_corpus — a collection as the GPU trains from it (nvsm_corpus_upload): tokens [num_tokens] int32 model word ids,
    documents back to back; doc_offsets [num_documents + 1] int64 (first 0, non-decreasing, last num_tokens); optional
    doc_weights [num_documents] float32 (the instance weight of every window of the document) and term_weights [num_words]
    float32 (the feature weight of every occurrence of the word). Host arrays. What needs no device is checked here; that
    the tokens name words of the model, and the lengths that depend on the model, by Model.upload_corpus."""

    def __init__(self, tokens, doc_offsets, doc_weights=None, term_weights=None):
        def as_array(a, dtype, kind, name):
            a = np.asarray(a)
            if a.ndim != 1:
                raise ValueError("%s must be a flat array" % name)
            if a.size and not np.issubdtype(a.dtype, kind):
                raise ValueError("%s must hold %s" % (name, "integers" if kind is np.integer else "floats"))
            return a, np.ascontiguousarray(a, dtype=dtype)

        raw, self.tokens = as_array(tokens, np.int32, np.integer, "tokens")
        if raw.size and (raw.min() < 0 or raw.max() >= 2 ** 31):
            raise ValueError("a token is outside int32")
        _, self.doc_offsets = as_array(doc_offsets, np.int64, np.integer, "doc_offsets")
        off = self.doc_offsets
        if off.size < 1 or off[0] != 0:
            raise ValueError("doc_offsets must start at 0")
        if (off[1:] < off[:-1]).any():
            raise ValueError("doc_offsets must not decrease")
        if off[-1] != self.tokens.size:
            raise ValueError("the last of doc_offsets is %d, expected num_tokens = %d" % (off[-1], self.tokens.size))
        self.num_tokens, self.num_documents = int(self.tokens.size), int(off.size - 1)
        self.doc_weights = self.term_weights = None
        if doc_weights is not None:
            _, self.doc_weights = as_array(doc_weights, np.float32, np.number, "doc_weights")
            if self.doc_weights.size != self.num_documents:
                raise ValueError("doc_weights holds %d values, expected num_documents = %d" % (self.doc_weights.size, self.num_documents))
        if term_weights is not None:
            _, self.term_weights = as_array(term_weights, np.float32, np.number, "term_weights")

    def as_struct(self):
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        return NvsmCorpus(ptr(self.tokens), self.doc_offsets.ctypes.data, None if self.doc_weights is None else self.doc_weights.ctypes.data,
                          None if self.term_weights is None else self.term_weights.ctypes.data, self.num_tokens, self.num_documents)


class WindowBatch:
    """nvsm_window_batch — a batch as window references: refs [n, 2] uint32, (document, first token inside the document) per
    window. A numpy array (pageable, or the .array of a PinnedArray or a slice of it: page-locked), a torch CUDA tensor
    (uint32, or int32 holding the same bits), or a device pointer given as an int together with num_instances."""

    def __init__(self, refs, num_instances=None):
        if isinstance(refs, (int, np.integer)) and not isinstance(refs, bool):
            if num_instances is None or int(num_instances) < 1:
                raise ValueError("a device pointer needs num_instances >= 1")
            if int(refs) == 0:
                raise ValueError("refs is a null device pointer")
            self.refs, self.on_device, self.num_instances, self._address = None, True, int(num_instances), int(refs)
            return
        self.on_device = hasattr(refs, "data_ptr")
        if self.on_device:
            if str(refs.dtype) not in ("torch.uint32", "torch.int32"):
                raise ValueError("refs must be uint32")
            if not refs.is_contiguous():
                raise ValueError("device arrays must be contiguous")
            shape = tuple(refs.shape)
            self.refs = refs
        else:
            a = np.asarray(refs)
            if a.dtype != np.uint32:
                raise ValueError("refs must be uint32, not %s" % a.dtype)
            shape = a.shape
            self.refs = a if a.flags["C_CONTIGUOUS"] else np.ascontiguousarray(a)      # (a row slice of a pinned plan stays where it is)
        if len(shape) != 2 or shape[1] != 2:
            raise ValueError("refs has shape %s, expected [num_instances][2]" % (shape,))
        if shape[0] < 1:
            raise ValueError("refs is empty: a batch needs at least one window")
        if num_instances is not None and int(num_instances) != shape[0]:
            raise ValueError("num_instances = %d, but refs holds %d windows" % (int(num_instances), shape[0]))
        self.num_instances = int(shape[0])
        self._address = int(self.refs.data_ptr()) if self.on_device else int(self.refs.ctypes.data)

    def as_struct(self):
        return NvsmWindowBatch(self._address, self.num_instances, int(self.on_device))


def expand_windows(corpus, refs, window):
    """The Batch (host, numpy) that window references denote — the definition in include/cunvsm_amd.h, word for word:
    features[i, j] = tokens[doc_offsets[doc_i] + pos_i + j], feature_weights = term_weights[features] (None without
    term_weights), labels[i] = doc_i, weights[i] = doc_weights[doc_i] (None without doc_weights). Raises ValueError for a
    reference the device would flag: a document >= num_documents, or a window that reaches beyond its document."""
    refs = np.asarray(refs)
    if refs.ndim != 2 or refs.shape[1] != 2:
        raise ValueError("refs has shape %s, expected [num_instances][2]" % (refs.shape,))
    window = int(window)
    if window < 1:
        raise ValueError("window must be at least 1")
    doc, pos = refs[:, 0].astype(np.int64), refs[:, 1].astype(np.int64)
    if doc.size and (doc.min() < 0 or doc.max() >= corpus.num_documents):
        raise ValueError("a reference names a document outside [0, num_documents = %d)" % corpus.num_documents)
    off = corpus.doc_offsets
    if ((pos < 0) | (pos + window > off[doc + 1] - off[doc])).any():
        raise ValueError("a window reaches beyond its document's end")
    at = (off[doc] + pos)[:, None] + np.arange(window, dtype=np.int64)[None, :]
    features = corpus.tokens[at].astype(np.int64)
    fw = None if corpus.term_weights is None else corpus.term_weights[features].astype(np.float32)
    iw = None if corpus.doc_weights is None else corpus.doc_weights[doc].astype(np.float32)
    return Batch(features.ravel(), doc, None if fw is None else fw.ravel(), iw)


def mixture(text_weight, pair_weight):
    """nvsm_mixture; both weights must be > 0 (CHECK_NE(..., 0.0), cpp/objective.cu:708-709). No device needed."""
    if not (float(text_weight) > 0.0 and float(pair_weight) > 0.0):
        raise ValueError("text_weight and pair_weight of a mixture must both be > 0")
    return NvsmMixture(float(text_weight), float(pair_weight))


def self_information_weights(term_frequencies, total_terms):
    """-log(tf / total) per query term (py/nvsm/base.py:297-301): the weights py/query.py averages the word rows with."""
    tf = np.asarray(term_frequencies, dtype=np.float64)
    if tf.size and (tf <= 0).any():
        raise ValueError("term frequencies must be positive")
    if not total_terms > 0:
        raise ValueError("total_terms must be positive")
    return (-np.log(tf / float(total_terms))).astype(np.float32)


ACTIVATIONS = dict(NONLINEARITIES, model=_lib.ACT_MODEL, identity=_lib.ACT_IDENTITY, linear=_lib.ACT_IDENTITY)
_EMPTY_F64 = np.zeros(1, dtype=np.float64)      # what a call without queries hands over as its (unwritten) metric rows
SIMILARITIES = {"cosine": _lib.SIM_COSINE, "dot": _lib.SIM_DOT}


class Queries:
    """nvsm_queries: a list of word-id lists of any lengths (ragged), flattened to ids + offsets; optional per-word weights
    of the same shape. The element counts the ABI will read are checked here, as Batch.check_shapes does; id RANGES are
    checked on the device."""

    def __init__(self, queries, weights=None):
        rows = [np.asarray(q, dtype=np.int64).ravel() for q in queries]
        for q, r in zip(queries, rows):
            if np.asarray(q).ndim > 1:
                raise ValueError("a query must be a flat list of word ids")
        self.num_queries = len(rows)
        self.offsets = np.zeros(self.num_queries + 1, dtype=np.int64)
        if rows:
            np.cumsum([r.size for r in rows], out=self.offsets[1:])
        self.word_ids = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.int64), dtype=np.int64)
        self.word_weights = None
        if weights is not None:
            wrows = [np.asarray(w, dtype=np.float32).ravel() for w in weights]
            if len(wrows) != self.num_queries:
                raise ValueError("weights holds %d lists, expected one per query = %d" % (len(wrows), self.num_queries))
            for i, (r, w) in enumerate(zip(rows, wrows)):
                if r.size != w.size:
                    raise ValueError("weights[%d] holds %d values, query %d has %d words" % (i, w.size, i, r.size))
                if r.size and not abs(float(w.astype(np.float64).sum())) > 0.0:
                    raise ValueError("weights[%d] sum to zero" % i)
            self.word_weights = np.ascontiguousarray(np.concatenate(wrows) if wrows else np.zeros(0, np.float32), dtype=np.float32)

    def rows(self):
        """the queries as lists of word ids again"""
        return [self.word_ids[self.offsets[i]:self.offsets[i + 1]] for i in range(self.num_queries)]

    def as_struct(self):
        return NvsmQueries(self.word_ids.ctypes.data, None if self.word_weights is None else self.word_weights.ctypes.data,
                           self.offsets.ctypes.data, self.num_queries)


def rank_options(num_entities, top_k=None, bias_coefficient=1.0, activation="model", similarity="cosine"):
    """nvsm_rank_options from keywords; raises ValueError for what the ABI would refuse (no device needed)."""
    opt = NvsmRankOptions()
    opt.bias_coefficient, opt.activation, opt.similarity, opt.top_k = 1.0, _lib.ACT_MODEL, _lib.SIM_COSINE, 1000
    if isinstance(activation, str):
        if activation not in ACTIVATIONS:
            raise ValueError("unknown activation %r (one of %s)" % (activation, sorted(ACTIVATIONS)))
        activation = ACTIVATIONS[activation]
    if isinstance(similarity, str):
        if similarity not in SIMILARITIES:
            raise ValueError("unknown similarity %r (one of %s)" % (similarity, sorted(SIMILARITIES)))
        similarity = SIMILARITIES[similarity]
    opt.bias_coefficient, opt.activation, opt.similarity = float(bias_coefficient), int(activation), int(similarity)
    if top_k is not None:
        if not 1 <= int(top_k) <= int(num_entities):
            raise ValueError("top_k = %d outside [1, num_entities = %d]" % (int(top_k), int(num_entities)))
        opt.top_k = int(top_k)
    return opt


def candidate_arrays(num_entities, num_queries, candidates):
    """(flat ids, offsets) of per-query candidate lists as nvsm_rank_options reads them; raises ValueError for what the ABI
    would refuse."""
    rows = [np.asarray(c, dtype=np.int64).ravel() for c in candidates]
    if len(rows) != num_queries:
        raise ValueError("candidates holds %d lists, expected one per query = %d" % (len(rows), num_queries))
    off = np.zeros(num_queries + 1, dtype=np.int64)
    if rows:
        np.cumsum([r.size for r in rows], out=off[1:])
    flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.int64), dtype=np.int64)
    if flat.size and (flat.min() < 0 or flat.max() >= num_entities):
        raise ValueError("a candidate document id is outside [0, num_entities = %d)" % num_entities)
    return flat, off


class Judgments:
    """nvsm_judgments: per query a list of (model document id, grade) pairs, flattened to ids + grades + offsets. Id -1 is a
    judged document the model does not hold (it counts towards num_rel and can never be retrieved); grade >= 1 is relevant.
    What needs no device is checked here: pair shape, and an id >= 0 given twice for one query. The id RANGE is checked by
    Model.evaluate, which knows num_entities."""

    def __init__(self, lists):
        ids, grades = [], []
        for i, pairs in enumerate(lists):
            a = np.asarray(list(pairs), dtype=np.int64)
            if a.size == 0:
                a = a.reshape(0, 2)
            if a.ndim != 2 or a.shape[1] != 2:
                raise ValueError("judgments[%d] must be a list of (document id, grade) pairs" % i)
            if a.size and (np.abs(a[:, 1]) >= 2 ** 31).any():
                raise ValueError("judgments[%d] holds a grade outside int32" % i)
            held = np.sort(a[a[:, 0] >= 0, 0])
            if held.size > 1 and (held[1:] == held[:-1]).any():
                raise ValueError("judgments[%d] judges a document id twice" % i)
            ids.append(a[:, 0])
            grades.append(a[:, 1].astype(np.int32))
        self.num_queries = len(ids)
        self.offsets = np.zeros(self.num_queries + 1, dtype=np.int64)
        if ids:
            np.cumsum([r.size for r in ids], out=self.offsets[1:])
        self.doc_ids = np.ascontiguousarray(np.concatenate(ids) if ids else np.zeros(0, np.int64), dtype=np.int64)
        self.grades = np.ascontiguousarray(np.concatenate(grades) if grades else np.zeros(0, np.int32), dtype=np.int32)

    def as_struct(self, cutoffs):
        """cutoffs: a contiguous int32 array the caller keeps alive."""
        j = NvsmJudgments()
        j.doc_ids = self.doc_ids.ctypes.data if self.doc_ids.size else None
        j.grades = self.grades.ctypes.data if self.grades.size else None
        j.offsets = self.offsets.ctypes.data
        j.cutoffs = cutoffs.ctypes.data if cutoffs.size else None
        j.num_cutoffs = int(cutoffs.size)
        return j


def eval_cutoffs(cutoffs):
    """The cutoffs of Model.evaluate as an int32 array; raises ValueError for what nvsm_evaluate would refuse."""
    c = np.asarray(list(cutoffs), dtype=np.int64).ravel()
    if c.size > _lib.EVAL_MAX_CUTOFFS:
        raise ValueError("%d cutoffs, at most %d" % (c.size, _lib.EVAL_MAX_CUTOFFS))
    if c.size and (c.min() < 1 or c.max() >= 2 ** 31):
        raise ValueError("a cutoff is outside [1, 2^31)")
    if c.size > 1 and (c[1:] <= c[:-1]).any():
        raise ValueError("cutoffs must ascend")
    return np.ascontiguousarray(c, dtype=np.int32)


EVAL_FIXED_NAMES = ("num_ret", "num_rel", "num_rel_ret", "map", "Rprec", "recip_rank", "ndcg")


def eval_metric_names(cutoffs):
    """The columns of a metric row of nvsm_evaluate, by trec_eval's names."""
    names = list(EVAL_FIXED_NAMES)
    for c in cutoffs:
        names += ["P_%d" % c, "recall_%d" % c, "ndcg_cut_%d" % c]
    return names


LEXICAL_METHODS = {"jm": _lib.LEX_JM, "dirichlet": _lib.LEX_DIRICHLET}
NORMALIZERS = {"standardize": _lib.NORM_STANDARDIZE, "minmax": _lib.NORM_MINMAX, "none": _lib.NORM_NONE}


def lexical_options(method="jm", param=None, top_k=1000):
    """nvsm_lexical_options from keywords (param None or "auto": 0 = auto); raises ValueError for what the ABI would refuse
    without a device. top_k against the corpus is checked by the library, which holds it."""
    opt = _lib.NvsmLexicalOptions()
    if isinstance(method, str):
        if method not in LEXICAL_METHODS:
            raise ValueError("unknown lexical method %r (one of %s)" % (method, sorted(LEXICAL_METHODS)))
        method = LEXICAL_METHODS[method]
    value = 0.0 if param is None or param == "auto" else float(param)
    if method == _lib.LEX_JM and value != 0.0 and not 0.0 < value < 1.0:
        raise ValueError("lambda = %r outside (0, 1)" % (param,))
    if method == _lib.LEX_DIRICHLET and value < 0.0:
        raise ValueError("mu = %r is negative" % (param,))
    if int(top_k) < 1:
        raise ValueError("top_k = %d is smaller than 1" % int(top_k))
    opt.method, opt.param, opt.top_k = int(method), value, int(top_k)
    return opt


def sdm_options(weights=(0.85, 0.10, 0.05), window=8):
    """nvsm_sdm_options from keywords: weights = (terms, ordered pairs, unordered pairs); raises ValueError for what the ABI would
    refuse. An NvsmSdmOptions, a dict of these keywords or True (the defaults) are taken as they are."""
    if isinstance(weights, _lib.NvsmSdmOptions):
        return weights
    if weights is True:
        weights = (0.85, 0.10, 0.05)
    if isinstance(weights, dict):
        return sdm_options(**weights)
    w = [float(x) for x in weights]
    if len(w) != 3:
        raise ValueError("sdm weights are (terms, ordered, unordered), got %d values" % len(w))
    if any(not np.isfinite(x) or x < 0.0 for x in w):
        raise ValueError("an sdm weight in %r is negative or not finite" % (tuple(w),))
    if not any(np.float32(x) > 0 for x in w):
        raise ValueError("the three sdm weights are all zero")
    if not 2 <= int(window) <= _lib.SDM_MAX_WINDOW:
        raise ValueError("window = %d outside [2, %d]" % (int(window), _lib.SDM_MAX_WINDOW))
    opt = _lib.NvsmSdmOptions()
    opt.w_term, opt.w_ordered, opt.w_unordered, opt.window = w[0], w[1], w[2], int(window)
    return opt


def ensemble_options(alpha=0.5, normalizer="standardize"):
    """nvsm_ensemble_options from keywords; raises ValueError for what the ABI would refuse."""
    opt = _lib.NvsmEnsembleOptions()
    if isinstance(normalizer, str):
        if normalizer not in NORMALIZERS:
            raise ValueError("unknown normalizer %r (one of %s)" % (normalizer, sorted(NORMALIZERS)))
        normalizer = NORMALIZERS[normalizer]
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha = %r outside [0, 1]" % (alpha,))
    opt.alpha, opt.normalizer = float(alpha), int(normalizer)
    return opt


def alpha_grid(stepsize):
    """The reference's grid of fusion weights, np.arange(0.0, 1.0, stepsize) restated: ceil(1.0 / stepsize) points computed in
    fp64, alpha_i = float32(i * stepsize); 1.0 itself is excluded. More than SWEEP_MAX_ALPHAS points are refused."""
    step = float(stepsize)
    if not (np.isfinite(step) and 0.0 < step <= 1.0):
        raise ValueError("stepsize = %r outside (0, 1]" % (stepsize,))
    n = int(np.ceil(1.0 / step))
    if n > _lib.SWEEP_MAX_ALPHAS:
        raise ValueError("stepsize = %r gives %d alphas, at most %d" % (stepsize, n, _lib.SWEEP_MAX_ALPHAS))
    return (np.arange(n, dtype=np.float64) * step).astype(np.float32)


def sweep_alphas(alphas):
    """The alphas of Model.ensemble_sweep as a float32 array; raises ValueError for what nvsm_ensemble_sweep would refuse."""
    a = np.ascontiguousarray(np.asarray(alphas, dtype=np.float32).ravel())
    if not 1 <= a.size <= _lib.SWEEP_MAX_ALPHAS:
        raise ValueError("%d alphas, expected 1 to %d" % (a.size, _lib.SWEEP_MAX_ALPHAS))
    if not (np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0):
        raise ValueError("an alpha is outside [0, 1] or not finite")
    return a


def sweep_options(alphas, normalizer="standardize", depth=0):
    """nvsm_sweep_options over a float32 array the caller keeps alive; raises ValueError for what the ABI would refuse."""
    opt = _lib.NvsmSweepOptions()
    if isinstance(normalizer, str):
        if normalizer not in NORMALIZERS:
            raise ValueError("unknown normalizer %r (one of %s)" % (normalizer, sorted(NORMALIZERS)))
        normalizer = NORMALIZERS[normalizer]
    if int(depth) < 0:
        raise ValueError("depth = %d is negative" % int(depth))
    opt.alphas, opt.num_alphas, opt.normalizer, opt.depth = alphas.ctypes.data, int(alphas.size), int(normalizer), int(depth)
    return opt


def feedback_options(fb_docs=10, fb_terms=10, orig_weight=0.5):
    """nvsm_feedback_options from keywords; raises ValueError for what the ABI would refuse without a device. fb_docs against the
    corpus and fb_terms against the vocabulary are checked by the library, which holds them."""
    opt = _lib.NvsmFeedbackOptions()
    if not 1 <= int(fb_docs) <= _lib.FEEDBACK_MAX_DOCS:
        raise ValueError("fb_docs = %d outside [1, %d]" % (int(fb_docs), _lib.FEEDBACK_MAX_DOCS))
    if int(fb_terms) < 1:
        raise ValueError("fb_terms = %d is smaller than 1" % int(fb_terms))
    if not 0.0 <= float(orig_weight) <= 1.0:
        raise ValueError("orig_weight = %r outside [0, 1]" % (orig_weight,))
    opt.fb_docs, opt.fb_terms, opt.orig_weight = int(fb_docs), int(fb_terms), float(orig_weight)
    return opt


IDFS = {"robertson": _lib.IDF_ROBERTSON, "okapi": _lib.IDF_OKAPI}
FIRST_STAGES = {"tfidf": _lib.STAGE_TFIDF, "lexical": _lib.STAGE_LEXICAL}
INDEX_USES = {"auto": _lib.INDEX_AUTO, "always": _lib.INDEX_ALWAYS, "never": _lib.INDEX_NEVER}


def tfidf_options(k1=None, b=None, idf="robertson", top_k=1000):
    """nvsm_tfidf_options from keywords (k1 / b None or "auto": 0 = auto 1.2 / 0.75); raises ValueError for what the ABI would refuse
    without a device. top_k against the corpus is checked by the library, which holds it."""
    opt = _lib.NvsmTfidfOptions()
    if isinstance(idf, str):
        if idf not in IDFS:
            raise ValueError("unknown idf %r (one of %s)" % (idf, sorted(IDFS)))
        idf = IDFS[idf]
    k1v = 0.0 if k1 is None or k1 == "auto" else float(k1)
    bv = 0.0 if b is None or b == "auto" else float(b)
    if not (np.isfinite(k1v) and k1v >= 0.0):
        raise ValueError("k1 = %r must be finite and positive" % (k1,))
    if not 0.0 <= bv <= 1.0:
        raise ValueError("b = %r outside (0, 1]" % (b,))
    if int(top_k) < 1:
        raise ValueError("top_k = %d is smaller than 1" % int(top_k))
    opt.k1, opt.b, opt.idf, opt.top_k = k1v, bv, int(idf), int(top_k)
    return opt


def as_feedback_options(feedback):
    """feedback given as an NvsmFeedbackOptions, a dict of feedback_options' keywords, a (fb_docs, fb_terms, orig_weight) tuple, or True
    for the defaults"""
    if isinstance(feedback, _lib.NvsmFeedbackOptions):
        return feedback
    if feedback is True:
        return feedback_options()
    if isinstance(feedback, dict):
        return feedback_options(**feedback)
    return feedback_options(*feedback)


def weighted_queries(queries, weights):
    """Queries whose per-word weights are those of the weighted lexical scorer: float32, each finite and >= 0 (a weight 0 drops its
    term, so a query's weights may well sum to zero — unlike rank()'s averaging weights)."""
    q = Queries(queries)
    rows = [np.asarray(w, dtype=np.float32).ravel() for w in weights]
    if len(rows) != q.num_queries:
        raise ValueError("weights holds %d lists, expected one per query = %d" % (len(rows), q.num_queries))
    for i, w in enumerate(rows):
        n = int(q.offsets[i + 1] - q.offsets[i])
        if w.size != n:
            raise ValueError("weights[%d] holds %d values, query %d has %d words" % (i, w.size, i, n))
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("weights[%d] holds a value that is negative or not finite" % i)
    q.word_weights = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.float32), dtype=np.float32)
    if q.word_weights.size == 0:
        q.word_weights = np.zeros(1, np.float32)      # (the ABI wants a pointer even where there is nothing to read)
    return q


SPACES = {"words": _lib.SPACE_WORDS, "projected_words": _lib.SPACE_PROJECTED_WORDS, "entities": _lib.SPACE_ENTITIES}


def space_shape(cfg, space):
    """(enum, rows, dimension) of a searched or source space of nvsm_neighbors: "words" | "projected_words" | "entities"."""
    if isinstance(space, str):
        if space not in SPACES:
            raise ValueError("unknown space %r (one of %s)" % (space, sorted(SPACES)))
        space = SPACES[space]
    if space == _lib.SPACE_WORDS:
        return space, int(cfg.num_words), int(cfg.word_repr_size)
    if space == _lib.SPACE_PROJECTED_WORDS:
        return space, int(cfg.num_words), int(cfg.entity_repr_size)
    if space == _lib.SPACE_ENTITIES:
        return space, int(cfg.num_entities), int(cfg.entity_repr_size)
    raise ValueError("unknown space %r" % (space,))


def neighbor_arguments(cfg, space, ids=None, vectors=None, source=None, top_k=30, exclude_self=False, similarity="cosine",
                       bias_coefficient=1.0, activation="model"):
    """(nvsm_neighbor_queries, nvsm_neighbor_options, arrays to keep alive) from keywords; raises ValueError for what the ABI
    would refuse (no device needed)."""
    space, rows, dim = space_shape(cfg, space)
    if (ids is None) == (vectors is None):
        raise ValueError("exactly one of ids and vectors must be given")
    ropt = rank_options(rows, None, bias_coefficient=bias_coefficient, activation=activation, similarity=similarity)
    q = NvsmNeighborQueries()
    if ids is not None:
        src, src_rows, src_dim = space_shape(cfg, space if source is None else source)
        if src_dim != dim:
            raise ValueError("the source space's dimension %d differs from the searched space's dimension %d" % (src_dim, dim))
        if np.asarray(ids).ndim > 1:
            raise ValueError("ids must be a flat list of row ids")
        data = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        if data.size and (data.min() < 0 or data.max() >= src_rows):
            raise ValueError("a query row id is outside [0, %d)" % src_rows)
        if exclude_self and src != space:
            raise ValueError("exclude_self needs queries given as row ids of the searched space")
        q.ids, q.vectors, q.num_queries, q.source_space, q.dim = data.ctypes.data, None, data.size, src, dim
    else:
        if source is not None:
            raise ValueError("source names the space of ids; vectors have none")
        if exclude_self:
            raise ValueError("exclude_self needs queries given as row ids of the searched space")
        data = np.ascontiguousarray(vectors, dtype=np.float32)
        if data.ndim == 1:
            data = data.reshape(1, -1)
        if data.ndim != 2 or data.shape[1] != dim:
            raise ValueError("vectors has shape %s, expected [num_queries][dimension of the searched space = %d]" % (data.shape, dim))
        q.ids, q.vectors, q.num_queries, q.source_space, q.dim = None, data.ctypes.data, data.shape[0], space, dim
    if not 1 <= int(top_k) <= rows:
        raise ValueError("top_k = %d outside [1, rows of the searched space = %d]" % (int(top_k), rows))
    opt = NvsmNeighborOptions()
    opt.space, opt.similarity, opt.top_k, opt.exclude_self = space, ropt.similarity, int(top_k), int(bool(exclude_self))
    opt.bias_coefficient, opt.activation = ropt.bias_coefficient, ropt.activation
    return q, opt, data


# -- n-grams of terms in document space (TermBruteforcer, py/nvsm/base.py:106-162; nvsm_ngram_search) --------------------------
NGRAM_MAX_ROWS = 1 << 31      # the phrase stack stays below it (the selection keys' limit): 65 535 words for 2-grams


def ngram_rows(vocabulary_size, max_cardinality):
    """Rows of the phrase stack over `vocabulary_size` words (nvsm_ngram_rows): m 1-grams, then the m(m - 1)/2 2-grams; -1 where
    that is not below 2^31, for fewer than one word and for a cardinality outside {1, 2}. Needs no library."""
    m, c = int(vocabulary_size), int(max_cardinality)
    if m < 1 or c not in (1, 2):
        return -1
    rows = m if c == 1 else m + m * (m - 1) // 2
    return rows if rows < NGRAM_MAX_ROWS else -1


def ngram_encode(terms, vocabulary_size):
    """Phrase rows of `terms` [..., 2] (or [..., 1]): POSITIONS in the vocabulary, (a, -1) a 1-gram, (a, b) with a < b a 2-gram, in
    the order of np.vstack over itertools.combinations: row of (a, b) = m + a(2m - a - 1)/2 + (b - a - 1)."""
    m = int(vocabulary_size)
    t = np.asarray(terms, dtype=np.int64)
    if t.ndim == 0 or t.shape[-1] not in (1, 2):
        raise ValueError("terms must end in an axis of 1 or 2 positions")
    a = t[..., 0]
    b = t[..., 1] if t.shape[-1] == 2 else np.full_like(a, -1)
    pair = b >= 0
    if ((a < 0) | (a >= m)).any() or (pair & ((b <= a) | (b >= m))).any() or (b < -1).any():
        raise ValueError("positions must satisfy 0 <= a < m, and b = -1 or a < b < m (m = %d)" % m)
    return np.where(pair, m + a * (2 * m - a - 1) // 2 + (b - a - 1), a)


def ngram_decode(phrase_rows, vocabulary_size, max_cardinality=2):
    """The inverse of ngram_encode: positions [..., max_cardinality] int64 of phrase rows, -1 in unused slots (the second of a 1-gram,
    both of a row of -1: a slot beyond counts[q])."""
    m, c = int(vocabulary_size), int(max_cardinality)
    rows = ngram_rows(m, c)
    if rows < 0:
        raise ValueError("no phrase stack for vocabulary_size = %d, max_cardinality = %d" % (m, c))
    p = np.asarray(phrase_rows, dtype=np.int64)
    if ((p < -1) | (p >= rows)).any():
        raise ValueError("a phrase row is outside [-1, %d)" % rows)
    out = np.full(p.shape + (c,), -1, np.int64)
    one = (p >= 0) & (p < m)
    out[..., 0][one] = p[one]
    two = p >= m
    if two.any():
        t = p[two] - m
        start = lambda a: a * (2 * m - a - 1) // 2      # noqa: E731
        w = 2 * m - 1
        a = ((w - np.sqrt(np.maximum(w * w - 8.0 * t, 0.0))) / 2).astype(np.int64).clip(0, m - 2)
        for _ in range(4):      # the float estimate is off by one at most; integer fix-up against the runs' first rows
            a = np.where(start(a) > t, a - 1, a)
            a = np.where((a < m - 2) & (start(np.minimum(a + 1, m - 2)) <= t), a + 1, a)
        out[..., 0][two] = a
        out[..., 1][two] = a + 1 + (t - start(a))
    return out


def ngram_arguments(cfg, entity_ids=None, word_ids=None, vectors=None, vocabulary=None, max_cardinality=2, top_k=20, similarity="cosine",
                    bias_coefficient=1.0, activation="model"):
    """(nvsm_neighbor_queries, nvsm_ngram_options, vocabulary as int64 array or None, arrays to keep alive) from keywords; raises
    ValueError for everything nvsm_ngram_search would refuse (no device needed)."""
    if int(max_cardinality) not in (1, 2):
        raise ValueError("max_cardinality = %r outside {1, 2}" % (max_cardinality,))
    ropt = rank_options(1, None, bias_coefficient=bias_coefficient, activation=activation, similarity=similarity)
    if ropt.similarity not in SIMILARITIES.values():
        raise ValueError("unknown similarity %r" % (similarity,))
    if ropt.activation not in ACTIVATIONS.values():
        raise ValueError("unknown activation %r" % (activation,))
    if not np.isfinite(ropt.bias_coefficient):
        raise ValueError("bias_coefficient is not finite")
    V, de = int(cfg.num_words), int(cfg.entity_repr_size)
    voc = None
    if vocabulary is not None:
        if np.asarray(vocabulary).ndim != 1:
            raise ValueError("vocabulary must be a flat list of word ids")
        voc = np.ascontiguousarray(np.asarray(vocabulary, dtype=np.int64))
        if voc.size < 1:
            raise ValueError("vocabulary_size must be at least 1")
        if voc.min() < 0 or voc.max() >= V:
            raise ValueError("a vocabulary word id is outside [0, %d)" % V)
        if (np.diff(voc) <= 0).any():
            raise ValueError("the vocabulary must be strictly ascending")
    m = V if voc is None else voc.size
    rows = ngram_rows(m, max_cardinality)
    if rows < 0:
        raise ValueError("the phrase stack over %d words reaches the row limit 2^31 (at most 65535 words for 2-grams)" % m)
    given = [x is not None for x in (entity_ids, word_ids, vectors)]
    if sum(given) != 1:
        raise ValueError("exactly one of entity_ids, word_ids and vectors must be given")
    q = NvsmNeighborQueries()
    if vectors is None:
        ids = entity_ids if word_ids is None else word_ids
        src, src_rows = (_lib.SPACE_ENTITIES, int(cfg.num_entities)) if word_ids is None else (_lib.SPACE_PROJECTED_WORDS, V)
        if np.asarray(ids).ndim > 1:
            raise ValueError("ids must be a flat list of row ids")
        data = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        if data.size and (data.min() < 0 or data.max() >= src_rows):
            raise ValueError("a query row id is outside [0, %d)" % src_rows)
        q.ids, q.vectors, q.num_queries, q.source_space, q.dim = data.ctypes.data, None, data.size, src, de
    else:
        data = np.ascontiguousarray(vectors, dtype=np.float32)
        if data.ndim == 1:
            data = data.reshape(1, -1)
        if data.ndim != 2 or data.shape[1] != de:
            raise ValueError("vectors has shape %s, expected [num_queries][dimension of document space = %d]" % (data.shape, de))
        q.ids, q.vectors, q.num_queries, q.source_space, q.dim = None, data.ctypes.data, data.shape[0], _lib.SPACE_ENTITIES, de
    if not 1 <= int(top_k) <= rows:
        raise ValueError("top_k = %d outside [1, rows of the phrase stack = %d]" % (int(top_k), rows))
    opt = NvsmNgramOptions()
    opt.max_cardinality, opt.similarity, opt.top_k = int(max_cardinality), ropt.similarity, int(top_k)
    opt.bias_coefficient, opt.activation = ropt.bias_coefficient, ropt.activation
    opt.vocabulary, opt.vocabulary_size = (None, 0) if voc is None else (voc.ctypes.data, voc.size)
    return q, opt, voc, data


# -- exact t-SNE of document or word rows (py/visualize.py's sklearn.manifold.TSNE; nvsm_tsne) ----------------------------------
def tsne_arguments(cfg, space="entities", ids=None, limit=None, l2_normalize=False, perplexity=30.0, early_exaggeration=12.0,
                   learning_rate="auto", max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=0,
                   method="exact", n_neighbors=None):
    """(nvsm_tsne_options, number of rows, arrays to keep alive) from keywords; raises ValueError for what the ABI would refuse, in
    its order (no device needed). ids: row ids in any order (visualize.py --filter_unclassified); limit: the first rows (--limit);
    neither: every row. init: "pca", "random" (sklearn's 1e-4 · RandomState(random_state).standard_normal((n, 2))) or an [n][2] array.
    method: "exact" (nvsm_tsne) or "sparse" (nvsm_tsne_sparse: sklearn's barnes_hut at angle 0, up to TSNE_SPARSE_MAX_ROWS rows, with
    n_neighbors per row — None: sklearn's min(n − 1, int(3·perplexity + 1))); with "sparse" the kept arrays end with the
    nvsm_tsne_sparse_options."""
    if method not in ("exact", "sparse"):
        raise ValueError("unknown method %r (\"exact\" or \"sparse\")" % (method,))
    if method == "exact" and n_neighbors is not None:
        raise ValueError("n_neighbors belongs to method=\"sparse\"")
    max_rows = _lib.TSNE_MAX_ROWS if method == "exact" else _lib.TSNE_SPARSE_MAX_ROWS
    space, rows, _ = space_shape(cfg, space)
    if space == _lib.SPACE_PROJECTED_WORDS:
        raise ValueError("unknown space for t-SNE: \"entities\" or \"words\" (projected words are not served)")
    if ids is not None and limit is not None:
        raise ValueError("at most one of ids and limit may be given")
    id_array = None
    if ids is not None:
        if np.asarray(ids).ndim > 1:
            raise ValueError("ids must be a flat list of row ids")
        id_array = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        n = int(id_array.size)
    else:
        n = rows if limit is None else int(limit)
    if n < 2:
        raise ValueError("num_rows = %d: t-SNE needs at least 2 rows" % n)
    if id_array is None and n > rows:
        raise ValueError("limit = %d exceeds the rows of the space = %d" % (n, rows))
    if id_array is not None and (id_array.min() < 0 or id_array.max() >= rows):
        raise ValueError("a row id is outside [0, %d)" % rows)
    if n > max_rows:
        raise ValueError("num_rows = %d above the limit of %d rows" % (n, max_rows))
    perplexity = float(np.float32(perplexity))
    if not (np.isfinite(perplexity) and 0.0 < perplexity < n):
        raise ValueError("perplexity = %r must be finite, positive and below num_rows = %d" % (perplexity, n))
    early_exaggeration = float(np.float32(early_exaggeration))
    if not (np.isfinite(early_exaggeration) and early_exaggeration > 0.0):
        raise ValueError("early_exaggeration = %r must be finite and positive" % early_exaggeration)
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError("learning_rate must be a number or \"auto\"")
        learning_rate = 0.0
    elif not float(learning_rate) > 0.0 or not np.isfinite(float(learning_rate)):
        raise ValueError("learning_rate = %r must be finite and positive (or \"auto\")" % (learning_rate,))
    if not np.isfinite(float(min_grad_norm)):
        raise ValueError("min_grad_norm is not finite")
    given = None
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError("unknown init %r (\"pca\", \"random\" or an [n][2] array)" % init)
        if init == "random":
            given = (1e-4 * np.random.RandomState(random_state).standard_normal(size=(n, 2))).astype(np.float32)
    else:
        given = np.ascontiguousarray(init, dtype=np.float32)
        if given.shape != (n, 2):
            raise ValueError("init has shape %s, expected (%d, 2)" % (given.shape, n))
        if not np.isfinite(given).all():
            raise ValueError("init holds a value that is not finite")
    if int(max_iter) < 1:
        raise ValueError("max_iter = %d must be at least 1" % int(max_iter))
    if int(n_iter_without_progress) < 0:
        raise ValueError("n_iter_without_progress is negative")
    opt = NvsmTsneOptions()
    opt.space, opt.l2_normalize = space, int(bool(l2_normalize))
    opt.ids, opt.num_rows = (None if id_array is None else id_array.ctypes.data), n
    opt.perplexity, opt.early_exaggeration, opt.learning_rate, opt.min_grad_norm = perplexity, early_exaggeration, float(learning_rate), float(min_grad_norm)
    opt.max_iter, opt.n_iter_without_progress = int(max_iter), int(n_iter_without_progress)
    opt.init = _lib.TSNE_INIT_PCA if given is None else _lib.TSNE_INIT_GIVEN
    opt.init_embedding = None if given is None else given.ctypes.data
    if method == "exact":
        return opt, n, (id_array, given)
    sparse = NvsmTsneSparseOptions()
    if n_neighbors is None:
        if min(n - 1, int(3.0 * perplexity + 1.0)) > _lib.TSNE_SPARSE_MAX_NEIGHBORS:
            raise ValueError("perplexity = %r asks for more than the limit of %d neighbours" % (perplexity, _lib.TSNE_SPARSE_MAX_NEIGHBORS))
        k = min(n - 1, int(3.0 * perplexity + 1.0))
    else:
        k = int(n_neighbors)
        if not 1 <= k <= min(n - 1, _lib.TSNE_SPARSE_MAX_NEIGHBORS):
            raise ValueError("n_neighbors = %d outside [1, min(num_rows - 1, %d)]" % (k, _lib.TSNE_SPARSE_MAX_NEIGHBORS))
        sparse.n_neighbors = k
    if 2 * n * k >= 2 ** 31:
        raise ValueError("2 * num_rows * n_neighbors = %d: sparse t-SNE numbers fewer than 2^31 directed entries" % (2 * n * k))
    return opt, n, (id_array, given, sparse)


def fold_summation():
    """(chunk_entries, group_chunks) of nvsm_step_fold's summation order (nvsm_fold_summation)."""
    c, g = C.c_int32(), C.c_int32()
    lib().nvsm_fold_summation(C.byref(c), C.byref(g))
    return c.value, g.value


def minstd_canonical(seed, count):
    """`count` draws of std::generate_canonical<float, 1>(std::minstd_rand0(seed)) as float32 — the generator nvsm_initialize draws
    Glorot's uniforms from (x' = 16807 x mod 2^31 - 1; (x' - 1) / 2^31 in float, a result of 1 stepped down to the float below)."""
    m, a = 2147483647, 16807
    x = int(seed) % m
    if x == 0:
        x = 1
    block = min(int(count), 1 << 16)
    pows = np.empty(block, dtype=np.uint64)
    p = 1
    for i in range(block):
        p = p * a % m
        pows[i] = p
    out = np.empty(int(count), dtype=np.float32)
    done = 0
    while done < count:
        n = min(block, count - done)
        xs = (np.uint64(x) * pows[:n]) % np.uint64(m)
        out[done:done + n] = (xs - np.uint64(1)).astype(np.float32) / np.float32(2147483648.0)
        x = int(xs[-1])
        done += n
    np.minimum(out, np.nextafter(np.float32(1), np.float32(0)), out=out)
    return out


def grow_documents(params, new_rows, seed):
    """The four tensors of a model with `new_rows` more documents, for a fold-in (Model.step_fold): W, T and b as they are, the old
    rows of E copied, the new rows Glorot's U(-a, a) with a = sqrt(6 / (entity_repr_size + num_entities)) at the GROWN num_entities
    — the bound nvsm_initialize uses for the whole table of such a model —, drawn from std::minstd_rand0(seed) in row-major order.
    `params`: name -> array for the four PARAM_NAMES (Model.get_data())."""
    if new_rows < 0:
        raise ValueError("new_rows must be >= 0")
    if int(seed) <= 0:
        raise ValueError("seed must be > 0")
    out = {n: np.ascontiguousarray(params[n], dtype=np.float32).ravel().copy() for n in PARAM_NAMES}
    de = out["word_entity_mapping-bias"].size
    old = out["entity_representations-representations"]
    if old.size % de:
        raise ValueError("the documents table holds no whole rows of %d values" % de)
    n_total = old.size // de + int(new_rows)
    bound = np.float32(np.sqrt(6.0 / float(de + n_total)))
    u = minstd_canonical(seed, int(new_rows) * de)
    fresh = (np.float64(np.float32(2) * bound) * (u.astype(np.float64) - 0.5)).astype(np.float32)
    out["entity_representations-representations"] = np.concatenate([old, fresh])
    return out


# -- k-means of document or word rows (sklearn.cluster.KMeans(algorithm='lloyd', n_init=1); nvsm_kmeans) --------------------------
def kmeans_arguments(cfg, space="entities", num_clusters=8, ids=None, limit=None, l2_normalize=False, max_iter=300, tol=1e-4,
                     init="k-means++", seed=1):
    """(nvsm_kmeans_options, number of rows, dimension, arrays to keep alive) from keywords; raises ValueError for what the ABI would
    refuse, in its order (no device needed). ids: row ids in any order, duplicates allowed; limit: the first rows; neither: every
    row. init: "k-means++" (one candidate per draw from std::minstd_rand0(seed)) or a [num_clusters][dim] array."""
    space, rows, dim = space_shape(cfg, space)
    if space == _lib.SPACE_PROJECTED_WORDS:
        raise ValueError("unknown space for k-means: \"entities\" or \"words\" (projected words are not served)")
    if ids is not None and limit is not None:
        raise ValueError("at most one of ids and limit may be given")
    id_array = None
    if ids is not None:
        if np.asarray(ids).ndim > 1:
            raise ValueError("ids must be a flat list of row ids")
        id_array = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).ravel())
        n = int(id_array.size)
    else:
        n = rows if limit is None else int(limit)
    if n < 1:
        raise ValueError("num_rows = %d: k-means needs at least 1 row" % n)
    if id_array is None and n > rows:
        raise ValueError("limit = %d exceeds the rows of the space = %d" % (n, rows))
    if id_array is not None and (id_array.min() < 0 or id_array.max() >= rows):
        raise ValueError("a row id is outside [0, %d)" % rows)
    k = int(num_clusters)
    if k < 1 or k > n:
        raise ValueError("num_clusters = %d must be in [1, num_rows = %d]" % (k, n))
    if k > _lib.KMEANS_MAX_CLUSTERS:
        raise ValueError("num_clusters = %d above the limit of %d clusters" % (k, _lib.KMEANS_MAX_CLUSTERS))
    if int(max_iter) < 1:
        raise ValueError("max_iter = %d must be at least 1" % int(max_iter))
    tol = float(tol)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol = %r must be finite and not negative" % tol)
    given = None
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError("unknown init %r (\"k-means++\" or a [num_clusters][dim] array)" % init)
        if int(seed) < 1:
            raise ValueError("seed = %d must be at least 1" % int(seed))
    else:
        given = np.ascontiguousarray(init, dtype=np.float32)
        if given.shape != (k, dim):
            raise ValueError("init has shape %s, expected (%d, %d)" % (given.shape, k, dim))
        if not np.isfinite(given).all():
            raise ValueError("init holds a value that is not finite")
    opt = NvsmKmeansOptions()
    opt.space, opt.l2_normalize = space, int(bool(l2_normalize))
    opt.ids, opt.num_rows = (None if id_array is None else id_array.ctypes.data), n
    opt.num_clusters, opt.max_iter, opt.tol = k, int(max_iter), tol
    opt.init = _lib.KMEANS_INIT_PLUSPLUS if given is None else _lib.KMEANS_INIT_GIVEN
    opt.init_centers = None if given is None else given.ctypes.data
    opt.seed = int(seed) if given is None else 0
    return opt, n, dim, (id_array, given)


def cluster_agreement(labels, classes):
    """(purity, nmi, ari) of a clustering against a labelling of the same items, on the host: purity = Σ_j max_c n_jc / n; NMI with
    arithmetic-mean normalisation and natural logarithms (sklearn's normalized_mutual_info_score); ARI as sklearn's
    adjusted_rand_score. Labels and classes may be any values numpy can sort (strings included)."""
    labels, classes = np.asarray(labels).ravel(), np.asarray(classes).ravel()
    if labels.size != classes.size or labels.size == 0:
        raise ValueError("labels and classes must have the same, non-zero length")
    _, li = np.unique(labels, return_inverse=True)
    _, ci = np.unique(classes, return_inverse=True)
    t = np.zeros((int(li.max()) + 1, int(ci.max()) + 1), dtype=np.float64)
    np.add.at(t, (li.ravel(), ci.ravel()), 1.0)
    n = float(labels.size)
    a, b = t.sum(axis=1), t.sum(axis=0)
    purity = float(t.max(axis=1).sum() / n)

    def entropy(c):
        c = c[c > 0]
        return float(-np.sum(c / n * (np.log(c) - np.log(n))))

    eps = float(np.finfo(np.float64).eps)
    if a.size == 1 and b.size == 1:
        nmi = 1.0      # (one group on both sides: sklearn's special case)
    else:
        nz = t > 0
        mi = float(np.sum(t[nz] / n * np.log(n * t[nz] / np.outer(a, b)[nz])))
        mi = max(mi, 0.0)
        nmi = 0.0 if mi < eps else mi / max(0.5 * (entropy(a) + entropy(b)), eps)
    # pair counts, as sklearn's pair_confusion_matrix
    sum_sq = float(np.sum(t * t))
    n11 = sum_sq - n
    n01 = float(np.sum(t.dot(b))) - sum_sq
    n10 = float(np.sum(t.T.dot(a))) - sum_sq
    n00 = n * n - n01 - n10 - sum_sq
    if n10 == 0.0 and n01 == 0.0:
        ari = 1.0
    else:
        ari = 2.0 * (n11 * n00 - n10 * n01) / ((n11 + n10) * (n10 + n00) + (n11 + n01) * (n01 + n00))
    return purity, float(nmi), float(ari)


class Model:
    def __init__(self, cfg):
        self.cfg = cfg
        self._h = C.c_void_p()
        check(lib().nvsm_create(C.byref(cfg), C.byref(self._h)))
        self._cb = None

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().nvsm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- Model::initialize(RNG*) ------------------------------------------------------------------
    def initialize(self, seed):
        check(lib().nvsm_initialize(self._h, seed))

    @property
    def rng_state(self):
        s = C.c_uint64()
        check(lib().nvsm_rng_get_state(self._h, C.byref(s)))
        return s.value

    @rng_state.setter
    def rng_state(self, s):
        check(lib().nvsm_rng_set_state(self._h, s))

    # -- the step ----------------------------------------------------------------------------------
    def compute_cost(self, batch, entity_ids=None):
        ids = None
        if entity_ids is not None:
            ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
        st = self._checked(batch, ids)
        self._keep = (batch, ids)
        check(lib().nvsm_compute_cost(self._h, C.byref(st), None if ids is None else ids.ctypes.data))

    def _checked(self, batch, ids):
        batch.check_shapes(self.cfg.window_size)
        if ids is not None and ids.size != batch.num_instances * (self.cfg.num_random_entities + 1):
            raise ValueError("entity_ids holds %d ids, expected num_instances * (num_random_entities + 1) = %d"
                             % (ids.size, batch.num_instances * (self.cfg.num_random_entities + 1)))
        return batch.as_struct()

    def compute_gradients(self):
        check(lib().nvsm_compute_gradients(self._h))

    def update(self, learning_rate, scaled_regularization_lambda=None):
        if scaled_regularization_lambda is None:
            scaled_regularization_lambda = self.scaled_regularization_lambda()
        check(lib().nvsm_update(self._h, learning_rate, scaled_regularization_lambda))

    def get_cost(self):
        c = C.c_float()
        check(lib().nvsm_get_cost(self._h, C.byref(c)))
        return c.value

    def scaled_regularization_lambda(self):
        return lib().nvsm_scaled_regularization_lambda(self._h)

    def step(self, batch, learning_rate, entity_ids=None, want_cost=False):
        ids = None
        if entity_ids is not None:
            ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
        st = self._checked(batch, ids)
        self._keep = (batch, ids)
        c = C.c_float()
        check(lib().nvsm_step(self._h, C.byref(st), None if ids is None else ids.ctypes.data, learning_rate,
                              C.byref(c) if want_cost else None))
        return c.value if want_cost else None

    def step_fold(self, batch, learning_rate, first_document, entity_ids=None, want_cost=True):
        """nvsm_step_fold: compute_cost, then the documents update on rows [first_document, num_entities) alone; W, T, b and the
        rows below stay bit for bit as they are. Returns the cost (what compute_cost + get_cost return) unless want_cost is False."""
        ids = None
        if entity_ids is not None:
            ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
        st = self._checked(batch, ids)
        self._keep = (batch, ids)
        opt = _lib.NvsmFoldOptions()
        lib().nvsm_fold_options_default(C.byref(opt))
        opt.first_document = int(first_document)
        c = C.c_float()
        check(lib().nvsm_step_fold(self._h, C.byref(st), None if ids is None else ids.ctypes.data, C.byref(opt), learning_rate,
                                   C.byref(c) if want_cost else None))
        return c.value if want_cost else None

    # -- training from an HBM-resident corpus: window references instead of batches -------------------------------
    def upload_corpus(self, corpus):
        """nvsm_corpus_upload: the corpus into HBM (synchronous; replaces an earlier one; None frees it)."""
        if corpus is None:
            check(lib().nvsm_corpus_upload(self._h, None))
            return
        if corpus.term_weights is not None and corpus.term_weights.size != self.cfg.num_words:
            raise ValueError("term_weights holds %d values, expected num_words = %d" % (corpus.term_weights.size, self.cfg.num_words))
        st = corpus.as_struct()
        check(lib().nvsm_corpus_upload(self._h, C.byref(st)))

    # -- the inverted index of the uploaded corpus ------------------------------------------------
    def index_corpus(self, use="auto", positions=False):
        """nvsm_corpus_index: builds the postings of the uploaded corpus in HBM (once; a later call only sets `use`) and says
        which fill the lexical rounds take: "never" the arena scan, "always" the postings, "auto" chosen per round. Results do
        not depend on it. Returns {"num_postings", "bytes", "max_df", "use"}; with positions=True the positional layer is built
        behind the index (index_positions) and its dictionary is returned under "positions"."""
        if isinstance(use, str):
            if use not in INDEX_USES:
                raise ValueError("unknown index use %r (one of %s)" % (use, sorted(INDEX_USES)))
            use = INDEX_USES[use]
        opt = _lib.NvsmIndexOptions()
        lib().nvsm_index_options_default(C.byref(opt))
        opt.use = int(use)
        info = _lib.NvsmIndexInfo()
        check(lib().nvsm_corpus_index(self._h, C.byref(opt), C.byref(info)))
        names = {v: k for k, v in INDEX_USES.items()}
        out = {"num_postings": info.num_postings, "bytes": info.bytes, "max_df": info.max_df, "use": names[info.use]}
        if positions:
            out["positions"] = self.index_positions()
        return out

    def index_positions(self):
        """nvsm_corpus_index_positions: builds the positional layer of the index (once): every posting's in-document offsets.
        With it the SDM rounds may be served from the postings (the same bits). Returns {"num_positions", "bytes"}."""
        info = _lib.NvsmPositionsInfo()
        check(lib().nvsm_corpus_index_positions(self._h, C.byref(info)))
        return {"num_positions": info.num_positions, "bytes": info.bytes}

    def positions(self, word, document):
        """nvsm_corpus_positions: the 0-based offsets of `word` inside `document`, ascending, int64 [tf] (empty: not held)."""
        n = C.c_int64()
        st = lib().nvsm_corpus_positions(self._h, int(word), int(document), 0, None, C.byref(n))
        if n.value == 0:
            check(st)      # an empty run is a success; a refusal (no layer, an id out of range) is raised
        out = np.empty(n.value, dtype=np.int64)
        if n.value:
            check(lib().nvsm_corpus_positions(self._h, int(word), int(document), n.value, out.ctypes.data, C.byref(n)))
        return out

    def drop_positions(self):
        """nvsm_corpus_index_positions_free: frees the positional layer, the index stays (no layer: nothing happens)."""
        check(lib().nvsm_corpus_index_positions_free(self._h))

    def postings(self, word):
        """nvsm_corpus_postings: (doc ids int64 [df], tfs int32 [df]) of one word, documents ascending."""
        n = C.c_int64()
        st = lib().nvsm_corpus_postings(self._h, int(word), 0, None, None, C.byref(n))
        if n.value == 0:
            check(st)      # an empty list is a success; a refusal (no corpus, no index, word out of range) is raised
        ids = np.empty(n.value, dtype=np.int64)
        tfs = np.empty(n.value, dtype=np.int32)
        if n.value:
            check(lib().nvsm_corpus_postings(self._h, int(word), n.value, ids.ctypes.data, tfs.ctypes.data, C.byref(n)))
        return ids, tfs

    def drop_index(self):
        """nvsm_corpus_index_free: frees the index, the corpus stays (no index: nothing happens)."""
        check(lib().nvsm_corpus_index_free(self._h))

    def _checked_windows(self, windows, entity_ids):
        if not isinstance(windows, WindowBatch):
            windows = WindowBatch(windows)
        ids = None
        if entity_ids is not None:
            ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
            if ids.size != windows.num_instances * (self.cfg.num_random_entities + 1):
                raise ValueError("entity_ids holds %d ids, expected num_instances * (num_random_entities + 1) = %d"
                                 % (ids.size, windows.num_instances * (self.cfg.num_random_entities + 1)))
        self._keep = (windows, ids)
        return windows.as_struct(), ids

    def compute_cost_windows(self, windows, entity_ids=None):
        """nvsm_compute_cost_windows: compute_cost on the batch the references denote in the uploaded corpus."""
        st, ids = self._checked_windows(windows, entity_ids)
        check(lib().nvsm_compute_cost_windows(self._h, C.byref(st), None if ids is None else ids.ctypes.data))

    def step_windows(self, windows, learning_rate, entity_ids=None, want_cost=False):
        st, ids = self._checked_windows(windows, entity_ids)
        c = C.c_float()
        check(lib().nvsm_step_windows(self._h, C.byref(st), None if ids is None else ids.ctypes.data, float(learning_rate),
                                      C.byref(c) if want_cost else None))
        return c.value if want_cost else None

    def step_windows_deferred(self, windows, learning_rate, entity_ids=None):
        """nvsm_step_windows_deferred; returns the ticket for deferred_cost()."""
        st, ids = self._checked_windows(windows, entity_ids)
        t = C.c_int64()
        check(lib().nvsm_step_windows_deferred(self._h, C.byref(st), None if ids is None else ids.ctypes.data, float(learning_rate), C.byref(t)))
        return t.value

    # -- the entity-entity similarity objective, alone (batch None) or mixed into the text objective ----------------
    def _checked_mixed(self, batch, pairs, entity_ids, weights):
        if not isinstance(pairs, PairBatch):
            pairs = PairBatch(pairs)
        if pairs.num_pairs > self.cfg.max_batch_size:
            raise ValueError("num_pairs = %d exceeds max_batch_size = %d" % (pairs.num_pairs, self.cfg.max_batch_size))
        ids, st, mix = None, None, None
        if batch is not None:
            if entity_ids is not None:
                ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
            st = self._checked(batch, ids)
            mix = mixture(*weights)
        self._keep = (batch, ids, pairs)
        return st, ids, pairs.as_struct(), mix

    def compute_cost_mixed(self, batch, pairs, weights=(0.5, 0.5), entity_ids=None):
        """nvsm_compute_cost_mixed: `pairs` (a PairBatch) with the text `batch`, mixed with weights = (text, pairs); batch None:
        the pair objective alone. compute_gradients / update / get_cost / get_tensor then act on that result."""
        st, ids, ps, mix = self._checked_mixed(batch, pairs, entity_ids, weights)
        check(lib().nvsm_compute_cost_mixed(self._h, None if st is None else C.byref(st), None if ids is None else ids.ctypes.data,
                                            C.byref(ps), None if mix is None else C.byref(mix)))

    def step_mixed(self, batch, pairs, learning_rate, weights=(0.5, 0.5), entity_ids=None, want_cost=False):
        """nvsm_step_mixed: compute_cost_mixed + compute_gradients + update with the scaled lambda, as one multi-stream step."""
        st, ids, ps, mix = self._checked_mixed(batch, pairs, entity_ids, weights)
        c = C.c_float()
        check(lib().nvsm_step_mixed(self._h, None if st is None else C.byref(st), None if ids is None else ids.ctypes.data,
                                    C.byref(ps), None if mix is None else C.byref(mix), learning_rate, C.byref(c) if want_cost else None))
        return c.value if want_cost else None

    # -- the term-term similarity objective on the words table: `pairs` holds model word ids, weights = (text, term pairs) --
    def compute_cost_term_mixed(self, batch, pairs, weights=(0.5, 0.5), entity_ids=None):
        """nvsm_compute_cost_term_mixed: `pairs` (a PairBatch of model word ids) with the text `batch`, mixed with weights =
        (text, pairs); batch None: the term-pair objective alone."""
        st, ids, ps, mix = self._checked_mixed(batch, pairs, entity_ids, weights)
        check(lib().nvsm_compute_cost_term_mixed(self._h, None if st is None else C.byref(st), None if ids is None else ids.ctypes.data,
                                                 C.byref(ps), None if mix is None else C.byref(mix)))

    def step_term_mixed(self, batch, pairs, learning_rate, weights=(0.5, 0.5), entity_ids=None, want_cost=False):
        """nvsm_step_term_mixed: compute_cost_term_mixed + compute_gradients + update with the scaled lambda, as one step."""
        st, ids, ps, mix = self._checked_mixed(batch, pairs, entity_ids, weights)
        c = C.c_float()
        check(lib().nvsm_step_term_mixed(self._h, None if st is None else C.byref(st), None if ids is None else ids.ctypes.data,
                                         C.byref(ps), None if mix is None else C.byref(mix), learning_rate, C.byref(c) if want_cost else None))
        return c.value if want_cost else None

    def get_cost_f64(self):
        c = C.c_double()
        check(lib().nvsm_get_cost_f64(self._h, C.byref(c)))
        return c.value

    def increment_parameter(self, name, index, delta):
        check(lib().nvsm_increment_parameter(self._h, name.encode(), int(index), float(delta)))

    # -- Model::infer (cpp/model.cu:105-133) and the ranking of py/nvsm/base.py:362-430 ---------------
    def infer(self, queries, weights=None, **opts):
        """Projected query representations [Q, entity_repr_size] float32: f(T·mean + c·b), no batch normalisation.
        queries: a list of word-id lists (any lengths >= 1); weights: per-word weights of the same shape or None.
        opts: bias_coefficient (1), activation ("model" | "tanh" | "hard_tanh" | "identity")."""
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        opt = rank_options(self.cfg.num_entities, None, **opts)
        out = np.empty((q.num_queries, self.cfg.entity_repr_size), dtype=np.float32)
        st = q.as_struct()
        check(lib().nvsm_infer(self._h, C.byref(st), C.byref(opt), out.ctypes.data))
        return out

    def rank(self, queries, top_k=1000, weights=None, candidates=None, **opts):
        """The top_k documents per query: (ids [Q, k] int64, scores [Q, k] float32, counts [Q] int64), by score descending,
        ties by ascending id; slots beyond counts[q] hold (-1, -inf). candidates: optional per-query lists of document ids
        (duplicates and any order allowed): only those are scored. opts: as infer, plus similarity ("cosine" | "dot")."""
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        opt = rank_options(self.cfg.num_entities, top_k, **opts)
        keep = None
        if candidates is not None:
            flat, off = keep = candidate_arrays(self.cfg.num_entities, q.num_queries, candidates)
            opt.candidates, opt.candidate_offsets = flat.ctypes.data if flat.size else None, off.ctypes.data
        k = opt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        check(lib().nvsm_rank(self._h, C.byref(st), C.byref(opt), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        del keep
        return ids, scores, counts

    def evaluate(self, queries, judgments, top_k=1000, cutoffs=(5, 10, 20, 100, 1000), weights=None, candidates=None,
                 return_ranking=False, **opts):
        """Ranks as rank() does and computes every query's retrieval metrics on the device (nvsm_evaluate; the formulas are in
        include/cunvsm_amd.h). judgments: a Judgments, or per query a list of (document id, grade) pairs. Returns a dict of
        float64 arrays [Q] keyed num_ret, num_rel, num_rel_ret, map, Rprec, recip_rank, ndcg and, per cutoff c, P_<c>,
        recall_<c>, ndcg_cut_<c>; with return_ranking also (ids, scores, counts) as rank() returns them. The ranking's ties
        are broken by ascending document id, not by docno as trec_eval would."""
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        j = judgments if isinstance(judgments, Judgments) else Judgments(judgments)
        if j.num_queries != q.num_queries:
            raise ValueError("judgments holds %d lists, expected one per query = %d" % (j.num_queries, q.num_queries))
        if j.doc_ids.size and (j.doc_ids.min() < -1 or j.doc_ids.max() >= self.cfg.num_entities):
            raise ValueError("a judged document id is outside [-1, num_entities = %d)" % self.cfg.num_entities)
        cut = eval_cutoffs(cutoffs)
        opt = rank_options(self.cfg.num_entities, top_k, **opts)
        keep = None
        if candidates is not None:
            flat, off = keep = candidate_arrays(self.cfg.num_entities, q.num_queries, candidates)
            opt.candidates, opt.candidate_offsets = flat.ctypes.data if flat.size else None, off.ctypes.data
        k = opt.top_k
        names = eval_metric_names(cut.tolist())
        metrics = np.empty((q.num_queries, len(names)), dtype=np.float64)
        ids = scores = counts = None
        if return_ranking:
            ids = np.empty((q.num_queries, k), dtype=np.int64)
            scores = np.empty((q.num_queries, k), dtype=np.float32)
            counts = np.empty(q.num_queries, dtype=np.int64)
        st, js = q.as_struct(), j.as_struct(cut)
        check(lib().nvsm_evaluate(self._h, C.byref(st), C.byref(opt), C.byref(js), metrics.ctypes.data if metrics.size else _EMPTY_F64.ctypes.data,
                                  None if ids is None else ids.ctypes.data, None if scores is None else scores.ctypes.data,
                                  None if counts is None else counts.ctypes.data))
        del keep
        result = {name: np.ascontiguousarray(metrics[:, i]) for i, name in enumerate(names)}
        return (result, ids, scores, counts) if return_ranking else result

    # -- query-likelihood ranking over the uploaded corpus, and its fusion with rank()'s list --------
    def lexical_rank(self, queries, method="jm", param=None, top_k=1000, weights=None):
        """nvsm_lexical_rank: the top_k documents of the uploaded corpus per query under the query-likelihood model with
        Jelinek-Mercer ("jm", param = lambda) or Dirichlet ("dirichlet", param = mu) smoothing; param None = auto (lambda 0.5,
        mu the average document length). Returns (ids [Q, k], scores [Q, k], counts [Q]) as rank() does; a document is
        retrieved only if it holds a query term, so counts[q] may be smaller than top_k. weights (per query a list of float32
        weights >= 0, one per word): nvsm_lexical_rank_weighted, the score is the weighted sum of the terms' logs and a term of
        weight 0 is dropped."""
        if weights is not None:
            q = weighted_queries(queries.rows() if isinstance(queries, Queries) else queries, weights)
        else:
            q = queries if isinstance(queries, Queries) else Queries(queries)
        opt = lexical_options(method, param, top_k)
        k = opt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        call = lib().nvsm_lexical_rank if weights is None else lib().nvsm_lexical_rank_weighted
        check(call(self._h, C.byref(st), C.byref(opt), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    def relevance_model(self, queries, fb_docs=10, fb_terms=10, method="jm", param=None):
        """nvsm_relevance_model: per query the fb_terms words of largest probability under the relevance model of its fb_docs best
        documents (the unweighted lexical_rank at top_k = fb_docs; include/cunvsm_amd.h has the formula). Returns
        (term ids [Q, fb_terms] int64, probabilities [Q, fb_terms] float32, counts [Q]); slots beyond counts[q] hold (-1, -inf)."""
        q = queries if isinstance(queries, Queries) else Queries(queries)
        opt = lexical_options(method, param, 1)
        fb = feedback_options(fb_docs, fb_terms)
        ids = np.empty((q.num_queries, fb.fb_terms), dtype=np.int64)
        probs = np.empty((q.num_queries, fb.fb_terms), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        check(lib().nvsm_relevance_model(self._h, C.byref(st), C.byref(opt), C.byref(fb), ids.ctypes.data, probs.ctypes.data, counts.ctypes.data))
        return ids, probs, counts

    def lexical_rank_prf(self, queries, fb_docs=10, fb_terms=10, orig_weight=0.5, method="jm", param=None, top_k=1000):
        """nvsm_lexical_rank_prf: lexical_rank of the RM3 query — the original terms with weight orig_weight / L each, then the
        relevance model's expansion terms sharing 1 - orig_weight in proportion to their probabilities. Returns what lexical_rank does."""
        q = queries if isinstance(queries, Queries) else Queries(queries)
        opt = lexical_options(method, param, top_k)
        fb = feedback_options(fb_docs, fb_terms, orig_weight)
        k = opt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        check(lib().nvsm_lexical_rank_prf(self._h, C.byref(st), C.byref(opt), C.byref(fb), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    # -- sequential dependence: terms, ordered pairs, unordered pairs in a window --------
    def sdm_rank(self, queries, method="jm", param=None, top_k=1000, weights=(0.85, 0.10, 0.05), window=8):
        """nvsm_sdm_rank: lexical_rank()'s retrieved set ranked by the sequential dependence model — the mean log term of the query's
        words, of its adjacent pairs as exact phrases, and of those pairs co-occurring within `window` positions, mixed with
        weights = (terms, ordered, unordered) normalised over the groups that have members (include/cunvsm_amd.h has the formula).
        Returns what lexical_rank does."""
        q = queries if isinstance(queries, Queries) else Queries(queries)
        opt = lexical_options(method, param, top_k)
        sopt = sdm_options(weights, window)
        k = opt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        check(lib().nvsm_sdm_rank(self._h, C.byref(st), C.byref(opt), C.byref(sopt), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    def sdm_pair_counts(self, queries, window=8):
        """nvsm_sdm_pair_counts: (ordered, unordered) collection counts, uint64, of every adjacent pair of every query, concatenated in
        query order: a query of L words holds max(L - 1, 0) pairs."""
        q = queries if isinstance(queries, Queries) else Queries(queries)
        sopt = sdm_options(window=window)
        sizes = np.asarray([max(len(row) - 1, 0) for row in q.rows()], dtype=np.int64)
        n = int(sizes.sum())
        ordered = np.zeros(max(n, 1), dtype=np.uint64)
        unordered = np.zeros(max(n, 1), dtype=np.uint64)
        st = q.as_struct()
        check(lib().nvsm_sdm_pair_counts(self._h, C.byref(st), C.byref(sopt), ordered.ctypes.data, unordered.ctypes.data))
        return ordered[:n], unordered[:n]

    def rank_ensemble(self, queries, alpha=0.5, normalizer="standardize", judgments=None, top_k=1000, method="jm", param=None,
                      cutoffs=(5, 10, 20, 100, 1000), weights=None, feedback=None, dependence=None, **opts):
        """nvsm_rank_ensemble: rank()'s list and lexical_rank()'s list of every query, each normalised over its returned
        entries ("standardize" | "minmax" | "none") and fused with weights alpha and 1 - alpha (include/cunvsm_amd.h has the
        formula). Returns (ids [Q, 2k], scores [Q, 2k], counts [Q]); with judgments, (metrics, ids, scores, counts) where
        metrics is evaluate()'s dict computed on the fused list. feedback (True, a dict of fb_docs / fb_terms / orig_weight, such a
        tuple, or an NvsmFeedbackOptions): nvsm_rank_ensemble_prf, the lexical list is lexical_rank_prf()'s. dependence (True, a
        (terms, ordered, unordered) tuple, a dict of weights / window, or an NvsmSdmOptions): nvsm_rank_ensemble_sdm, the lexical list
        is sdm_rank()'s; not together with feedback. opts: as rank()."""
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        ropt = rank_options(self.cfg.num_entities, top_k, **opts)
        lopt = lexical_options(method, param, top_k)
        eopt = ensemble_options(alpha, normalizer)
        fopt = None if feedback is None or feedback is False else as_feedback_options(feedback)
        sopt = None if dependence is None or dependence is False else sdm_options(dependence)
        if fopt is not None and sopt is not None:
            raise ValueError("feedback and dependence cannot be combined: list B is either lexical_rank_prf()'s or sdm_rank()'s")
        k = ropt.top_k
        ids = np.empty((q.num_queries, 2 * k), dtype=np.int64)
        scores = np.empty((q.num_queries, 2 * k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        js = metrics = names = cut = None
        if judgments is not None:
            j = judgments if isinstance(judgments, Judgments) else Judgments(judgments)
            if j.num_queries != q.num_queries:
                raise ValueError("judgments holds %d lists, expected one per query = %d" % (j.num_queries, q.num_queries))
            if j.doc_ids.size and (j.doc_ids.min() < -1 or j.doc_ids.max() >= self.cfg.num_entities):
                raise ValueError("a judged document id is outside [-1, num_entities = %d)" % self.cfg.num_entities)
            cut = eval_cutoffs(cutoffs)
            names = eval_metric_names(cut.tolist())
            metrics = np.empty((q.num_queries, len(names)), dtype=np.float64)
            js = j.as_struct(cut)
        tail = (C.byref(eopt), None if js is None else C.byref(js),
                None if js is None else (metrics.ctypes.data if metrics.size else _EMPTY_F64.ctypes.data),
                ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
        if sopt is not None:
            check(lib().nvsm_rank_ensemble_sdm(self._h, C.byref(st), C.byref(ropt), C.byref(lopt), C.byref(sopt), *tail))
        elif fopt is None:
            check(lib().nvsm_rank_ensemble(self._h, C.byref(st), C.byref(ropt), C.byref(lopt), *tail))
        else:
            check(lib().nvsm_rank_ensemble_prf(self._h, C.byref(st), C.byref(ropt), C.byref(lopt), C.byref(fopt), *tail))
        if js is None:
            return ids, scores, counts
        result = {name: np.ascontiguousarray(metrics[:, i]) for i, name in enumerate(names)}
        return result, ids, scores, counts

    # -- TF-IDF first-stage retrieval and re-ranking of its candidates on the device --------
    def tfidf_rank(self, queries, k1=None, b=None, idf="robertson", top_k=1000, weights=None):
        """nvsm_tfidf_rank: the top_k documents of the uploaded corpus per query under BM25's saturating tf with Robertson's
        ("robertson") or Okapi's ("okapi") idf (include/cunvsm_amd.h has the formula); k1 / b None = auto (1.2 / 0.75). Returns
        (ids [Q, k], scores [Q, k], counts [Q]) as lexical_rank() does. weights (per query a list of float32 weights >= 0, one
        per word): every term times its weight, a term of weight 0 is dropped."""
        if weights is not None:
            q = weighted_queries(queries.rows() if isinstance(queries, Queries) else queries, weights)
        else:
            q = queries if isinstance(queries, Queries) else Queries(queries)
        opt = tfidf_options(k1, b, idf, top_k)
        k = opt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        if weights is None:
            st.word_weights = None
        check(lib().nvsm_tfidf_rank(self._h, C.byref(st), C.byref(opt), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids, scores, counts

    def rerank(self, queries, first_stage="tfidf", depth=1000, top_k=1000, judgments=None, cutoffs=(5, 10, 20, 100, 1000), weights=None,
               k1=None, b=None, idf="robertson", method="jm", param=None, **opts):
        """nvsm_rerank: rank() over the candidates the first stage retrieves at top_k = depth — tfidf_rank() ("tfidf": k1, b, idf) or
        lexical_rank() ("lexical": method, param), unweighted — handed over on the device: bit for bit rank(candidates = the first
        stage's ids). weights shape only the neural stage's query representation. Returns (ids [Q, top_k], scores, counts); with
        judgments, (metrics, ids, scores, counts), metrics being evaluate()'s dict for those candidates. opts: as rank()."""
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        if isinstance(first_stage, str):
            if first_stage not in FIRST_STAGES:
                raise ValueError("unknown first stage %r (one of %s)" % (first_stage, sorted(FIRST_STAGES)))
            first_stage = FIRST_STAGES[first_stage]
        ropt = rank_options(self.cfg.num_entities, top_k, **opts)
        # (depth against the corpus, the cap and top_k is checked by the library, which holds the corpus)
        topt = tfidf_options(k1, b, idf, int(depth))
        lopt = lexical_options(method, param, int(depth))
        rr = _lib.NvsmRerankOptions()
        rr.first_stage, rr.depth = int(first_stage), int(depth)
        rr.tfidf, rr.lexical = C.pointer(topt), C.pointer(lopt)
        k = ropt.top_k
        ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        st = q.as_struct()
        js = metrics = names = cut = None
        if judgments is not None:
            j = judgments if isinstance(judgments, Judgments) else Judgments(judgments)
            if j.num_queries != q.num_queries:
                raise ValueError("judgments holds %d lists, expected one per query = %d" % (j.num_queries, q.num_queries))
            if j.doc_ids.size and (j.doc_ids.min() < -1 or j.doc_ids.max() >= self.cfg.num_entities):
                raise ValueError("a judged document id is outside [-1, num_entities = %d)" % self.cfg.num_entities)
            cut = eval_cutoffs(cutoffs)
            names = eval_metric_names(cut.tolist())
            metrics = np.empty((q.num_queries, len(names)), dtype=np.float64)
            js = j.as_struct(cut)
        check(lib().nvsm_rerank(self._h, C.byref(st), C.byref(ropt), C.byref(rr), None if js is None else C.byref(js),
                                None if js is None else (metrics.ctypes.data if metrics.size else _EMPTY_F64.ctypes.data),
                                ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        if js is None:
            return ids, scores, counts
        result = {name: np.ascontiguousarray(metrics[:, i]) for i, name in enumerate(names)}
        return result, ids, scores, counts

    # -- supervised fusion: the alpha sweep and the k-fold choice of alpha --------
    def _sweep_arguments(self, queries, judgments, alphas, normalizer, depth, top_k, method, param, cutoffs, weights, feedback, opts):
        q = queries if isinstance(queries, Queries) else Queries(queries, weights)
        if judgments is None:
            raise ValueError("judgments are required")
        j = judgments if isinstance(judgments, Judgments) else Judgments(judgments)
        if j.num_queries != q.num_queries:
            raise ValueError("judgments holds %d lists, expected one per query = %d" % (j.num_queries, q.num_queries))
        if j.doc_ids.size and (j.doc_ids.min() < -1 or j.doc_ids.max() >= self.cfg.num_entities):
            raise ValueError("a judged document id is outside [-1, num_entities = %d)" % self.cfg.num_entities)
        a = sweep_alphas(alphas)
        sopt = sweep_options(a, normalizer, depth)
        ropt = rank_options(self.cfg.num_entities, top_k, **opts)
        lopt = lexical_options(method, param, top_k)
        fopt = None if feedback is None or feedback is False else as_feedback_options(feedback)
        cut = eval_cutoffs(cutoffs)
        return q, j, a, sopt, ropt, lopt, fopt, cut

    def ensemble_sweep(self, queries, judgments, alphas, normalizer="standardize", depth=0, top_k=1000, method="jm", param=None,
                       cutoffs=(5, 10, 20, 100, 1000), weights=None, feedback=None, **opts):
        """nvsm_ensemble_sweep: rank()'s and lexical_rank()'s (feedback: lexical_rank_prf()'s) lists made once, then the metrics of
        their fusion at every alpha of `alphas` (float32 in [0, 1], at most SWEEP_MAX_ALPHAS), over the first `depth` entries of each
        fused list (0: all). Returns a dict of float64 arrays [A, Q] keyed as evaluate()'s; with depth 0 row [a] holds the bits
        rank_ensemble(alpha=alphas[a], judgments=...) returns."""
        q, j, a, sopt, ropt, lopt, fopt, cut = self._sweep_arguments(queries, judgments, alphas, normalizer, depth, top_k, method, param,
                                                                      cutoffs, weights, feedback, opts)
        names = eval_metric_names(cut.tolist())
        table = np.empty((a.size, q.num_queries, len(names)), dtype=np.float64)
        st, js = q.as_struct(), j.as_struct(cut)
        check(lib().nvsm_ensemble_sweep(self._h, C.byref(st), C.byref(ropt), C.byref(lopt), None if fopt is None else C.byref(fopt),
                                        C.byref(sopt), C.byref(js), table.ctypes.data if table.size else _EMPTY_F64.ctypes.data))
        return {name: np.ascontiguousarray(table[:, :, i]) for i, name in enumerate(names)}

    def rank_ensemble_cv(self, queries, judgments, alphas=None, stepsize=0.05, num_folds=20, measure="map", depth=1000, fold_of=None,
                         normalizer="standardize", top_k=1000, method="jm", param=None, cutoffs=(5, 10, 20, 100, 1000), weights=None,
                         feedback=None, return_sweep=False, **opts):
        """nvsm_rank_ensemble_cv, the reference's combine_runs.py --qrel: ensemble_sweep over `alphas` (None: alpha_grid(stepsize)),
        then per fold the alpha with the best mean `measure` (a key of the metric dict) over the queries outside the fold — on a tie the
        largest alpha — fuses the fold's queries. fold_of: per query its fold in [0, num_folds), None: contiguous folds in query order.
        Returns (fold_alphas [F] float32, fold_train_measures [F] float64, metrics, ids [Q, 2k], scores [Q, 2k], counts [Q]); metrics is
        evaluate()'s dict of the returned lists cut at depth; with return_sweep the sweep's dict [A, Q] follows."""
        if alphas is None:
            alphas = alpha_grid(stepsize)
        q, j, a, sopt, ropt, lopt, fopt, cut = self._sweep_arguments(queries, judgments, alphas, normalizer, depth, top_k, method, param,
                                                                      cutoffs, weights, feedback, opts)
        names = eval_metric_names(cut.tolist())
        if measure not in names:
            raise ValueError("unknown measure %r (one of %s)" % (measure, names))
        if names.index(measure) < _lib.EVAL_AP:
            raise ValueError("measure %r is not offered as a training measure" % (measure,))
        Q, F = q.num_queries, int(num_folds)
        if not 2 <= F <= Q:
            raise ValueError("num_folds = %d outside [2, num_queries = %d]" % (F, Q))
        copt = _lib.NvsmCvOptions()
        copt.measure, copt.num_folds = names.index(measure), F
        folds = None
        if fold_of is not None:
            folds = np.ascontiguousarray(np.asarray(fold_of, dtype=np.int64).ravel())
            if folds.size != Q:
                raise ValueError("fold_of holds %d entries, expected one per query = %d" % (folds.size, Q))
            if folds.min() < 0 or folds.max() >= F:
                raise ValueError("a fold_of entry is outside [0, num_folds = %d)" % F)
            if np.bincount(folds, minlength=F).max() == Q:
                raise ValueError("a fold holds every query: its training set is empty")
            folds = folds.astype(np.int32)
            copt.fold_of = folds.ctypes.data
        k = ropt.top_k
        fold_alpha = np.empty(F, dtype=np.float32)
        fold_train = np.empty(F, dtype=np.float64)
        ids = np.empty((Q, 2 * k), dtype=np.int64)
        scores = np.empty((Q, 2 * k), dtype=np.float32)
        counts = np.empty(Q, dtype=np.int64)
        metrics = np.empty((Q, len(names)), dtype=np.float64)
        table = np.empty((a.size, Q, len(names)), dtype=np.float64) if return_sweep else None
        st, js = q.as_struct(), j.as_struct(cut)
        check(lib().nvsm_rank_ensemble_cv(self._h, C.byref(st), C.byref(ropt), C.byref(lopt), None if fopt is None else C.byref(fopt),
                                          C.byref(sopt), C.byref(copt), C.byref(js), fold_alpha.ctypes.data, fold_train.ctypes.data,
                                          ids.ctypes.data, scores.ctypes.data, counts.ctypes.data, metrics.ctypes.data,
                                          None if table is None else table.ctypes.data))
        result = {name: np.ascontiguousarray(metrics[:, i]) for i, name in enumerate(names)}
        out = (fold_alpha, fold_train, result, ids, scores, counts)
        if return_sweep:
            out += ({name: np.ascontiguousarray(table[:, :, i]) for i, name in enumerate(names)},)
        return out

    # -- nearest neighbours in word, projected-word and document space (py/nvsm/base.py:106-162, 325-353, 362-430) ----
    def neighbors(self, space, ids=None, vectors=None, source=None, top_k=30, exclude_self=False, similarity="cosine",
                  **projection_opts):
        """The top_k rows of `space` ("words" | "projected_words" | "entities") nearest to each query:
        (ids [Q, k] int64, scores [Q, k] float32, counts [Q] int64), by score descending, ties by ascending id; slots beyond
        counts[q] hold (-1, -inf). Queries: `ids`, row ids of `source` (default: the searched space), or `vectors` [Q, dim]
        float32. exclude_self (ids of the searched space only) leaves a query's own row out. projection_opts
        (bias_coefficient, activation: as infer) apply where projected words are searched or are the source."""
        q, opt, keep = neighbor_arguments(self.cfg, space, ids, vectors, source, top_k, exclude_self, similarity, **projection_opts)
        k = opt.top_k
        out_ids = np.empty((q.num_queries, k), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        check(lib().nvsm_neighbors(self._h, C.byref(q), C.byref(opt), out_ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        del keep
        return out_ids, scores, counts

    def similarity(self, space, a, b, similarity="cosine"):
        """Scores of row a[i] against row b[i] of one space, float32 [n] (nvsm_similarity)."""
        space, rows, _ = space_shape(self.cfg, space)
        if isinstance(similarity, str):
            if similarity not in SIMILARITIES:
                raise ValueError("unknown similarity %r (one of %s)" % (similarity, sorted(SIMILARITIES)))
            similarity = SIMILARITIES[similarity]
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int64).ravel())
        b = np.ascontiguousarray(np.asarray(b, dtype=np.int64).ravel())
        if a.size != b.size:
            raise ValueError("a holds %d ids, b holds %d" % (a.size, b.size))
        for x in (a, b):
            if x.size and (x.min() < 0 or x.max() >= rows):
                raise ValueError("a row id is outside [0, %d)" % rows)
        out = np.empty(a.size, dtype=np.float32)
        check(lib().nvsm_similarity(self._h, space, a.ctypes.data, b.ctypes.data, a.size, int(similarity), out.ctypes.data))
        return out

    def related_terms(self, word_ids, top_k=30):
        """NVSM.related_terms (base.py:325-342): the cosine neighbours of words among the word rows, the word itself included."""
        return self.neighbors("words", ids=word_ids, top_k=top_k)

    def term_similarity(self, a, b):
        """NVSM.term_similarity (base.py:344-353): cosine similarity of word rows a[i] and b[i]; a float for two scalars."""
        out = self.similarity("words", a, b)
        return float(out[0]) if np.ndim(a) == 0 and np.ndim(b) == 0 else out

    def nearest_terms(self, entity_ids=None, vectors=None, top_k=20, **projection_opts):
        """TermBruteforcer (base.py:106-162, cardinality 1): the words whose projection f(T·W[w] + c·b) lies closest to
        document rows (entity_ids) or to vectors of document space."""
        return self.neighbors("projected_words", ids=entity_ids, vectors=vectors, source=None if entity_ids is None else "entities",
                              top_k=top_k, **projection_opts)

    def nearest_ngrams(self, entity_ids=None, word_ids=None, vectors=None, vocabulary=None, max_cardinality=2, top_k=20,
                       similarity="cosine", bias_coefficient=1.0, activation="model"):
        """TermBruteforcer up to 2-grams (base.py:106-162; nvsm_ngram_search): the 1- and 2-grams of `vocabulary` (strictly ascending
        word ids; None: every word) whose projection f(T·mean(W[s_a], W[s_b]) + c·b) lies closest to document rows (entity_ids), to
        projected words (word_ids) or to vectors of document space. Returns (phrase_rows [Q, k] int64, terms [Q, k, max_cardinality]
        int64 model word ids with -1 in unused slots, scores [Q, k] float32, counts [Q] int64), by score descending, ties by ascending
        phrase row (ngram_decode gives positions in the vocabulary); slots beyond counts[q] hold (-1, -1 ..., -inf)."""
        q, opt, voc, keep = ngram_arguments(self.cfg, entity_ids, word_ids, vectors, vocabulary, max_cardinality, top_k, similarity,
                                            bias_coefficient, activation)
        k, c = opt.top_k, opt.max_cardinality
        rows = np.empty((q.num_queries, k), dtype=np.int64)
        terms = np.empty((q.num_queries, k, c), dtype=np.int64)
        scores = np.empty((q.num_queries, k), dtype=np.float32)
        counts = np.empty(q.num_queries, dtype=np.int64)
        check(lib().nvsm_ngram_search(self._h, C.byref(q), C.byref(opt), rows.ctypes.data, terms.ctypes.data, scores.ctypes.data,
                                      counts.ctypes.data))
        del keep, voc
        return rows, terms, scores, counts

    def tsne(self, space="entities", ids=None, limit=None, l2_normalize=False, perplexity=30.0, early_exaggeration=12.0,
             learning_rate="auto", max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=0,
             method="exact", n_neighbors=None):
        """py/visualize.py's sklearn.manifold.TSNE(n_components=2, init='pca', random_state=0) with the exact gradient, on the device
        (nvsm_tsne): the rows `ids` of `space` ("entities" | "words"), its first `limit` rows, or all of them. Returns
        (embedding [n, 2] float32, kl_divergence, n_iter) as sklearn's embedding_, kl_divergence_ and n_iter_.
        method="sparse" (nvsm_tsne_sparse): sklearn's default barnes_hut method at angle 0 — n_neighbors affinities per row (None:
        sklearn's 3·perplexity + 1) and the exact repulsion, no n × n memory: up to TSNE_SPARSE_MAX_ROWS rows."""
        opt, n, keep = tsne_arguments(self.cfg, space, ids, limit, l2_normalize, perplexity, early_exaggeration, learning_rate, max_iter,
                                      n_iter_without_progress, min_grad_norm, init, random_state, method, n_neighbors)
        embedding = np.empty((n, 2), dtype=np.float32)
        kl, it = C.c_double(0.0), C.c_int32(0)
        if method == "sparse":
            check(lib().nvsm_tsne_sparse(self._h, C.byref(opt), C.byref(keep[2]), embedding.ctypes.data, C.byref(kl), C.byref(it)))
        else:
            check(lib().nvsm_tsne(self._h, C.byref(opt), embedding.ctypes.data, C.byref(kl), C.byref(it)))
        del keep
        return embedding, kl.value, it.value

    def kmeans(self, space="entities", num_clusters=8, ids=None, limit=None, l2_normalize=False, max_iter=300, tol=1e-4,
               init="k-means++", seed=1, return_distances=False):
        """sklearn.cluster.KMeans(n_clusters, n_init=1, algorithm='lloyd') of table rows on the device (nvsm_kmeans): the rows `ids` of
        `space` ("entities" | "words"), its first `limit` rows, or all of them. Returns (labels [n] int32, centers [k, dim] float32,
        counts [k] int64, inertia, n_iter) and, with return_distances, the rows' squared distances to their centres [n] float32."""
        opt, n, dim, keep = kmeans_arguments(self.cfg, space, num_clusters, ids, limit, l2_normalize, max_iter, tol, init, seed)
        k = int(opt.num_clusters)
        labels = np.empty(n, dtype=np.int32)
        centers = np.empty((k, dim), dtype=np.float32)
        counts = np.empty(k, dtype=np.int64)
        distances = np.empty(n, dtype=np.float32) if return_distances else None
        inertia, it = C.c_double(0.0), C.c_int32(0)
        check(lib().nvsm_kmeans(self._h, C.byref(opt), labels.ctypes.data, centers.ctypes.data, counts.ctypes.data,
                                None if distances is None else distances.ctypes.data, C.byref(inertia), C.byref(it)))
        del keep
        if return_distances:
            return labels, centers, counts, inertia.value, it.value, distances
        return labels, centers, counts, inertia.value, it.value

    def related_documents(self, entity_ids, top_k=10, exclude_self=False):
        """Documents near documents (query_using_projected_query, base.py:362-430, with document rows as the queries)."""
        return self.neighbors("entities", ids=entity_ids, top_k=top_k, exclude_self=exclude_self)

    # -- parameters / tensors ----------------------------------------------------------------------
    def step_deferred(self, batch, learning_rate, entity_ids=None):
        """nvsm_step + an asynchronous read-back of its loss; returns the ticket for deferred_cost()."""
        ids = None
        if entity_ids is not None:
            ids = np.ascontiguousarray(entity_ids, dtype=np.int64)
        st = self._checked(batch, ids)
        self._keep = (batch, ids)
        t = C.c_int64()
        check(lib().nvsm_step_deferred(self._h, C.byref(st), ids.ctypes.data if ids is not None else None, float(learning_rate), C.byref(t)))
        return t.value

    def deferred_cost(self, ticket):
        c = C.c_float()
        check(lib().nvsm_deferred_cost(self._h, int(ticket), C.byref(c)))
        return c.value

    def wait_inputs(self):
        check(lib().nvsm_wait_inputs(self._h))

    def get_param(self, name):
        n = C.c_int64()
        check(lib().nvsm_param_size(self._h, name.encode(), C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        check(lib().nvsm_get_param(self._h, name.encode(), out.ctypes.data, n.value))
        return out

    def set_param(self, name, value):
        v = np.ascontiguousarray(value, dtype=np.float32).ravel()
        check(lib().nvsm_set_param(self._h, name.encode(), v.ctypes.data, v.size))

    def _row_width(self, name):
        n = C.c_int64()
        check(lib().nvsm_param_size(self._h, name.encode(), C.byref(n)))
        rows = self.cfg.num_words if name.startswith("word_representations") else self.cfg.num_entities
        return max(1, n.value // rows)

    def get_param_rows(self, name, first_row, rows):
        """nvsm_get_param_rows: rows [first_row, first_row + rows) of an embedding table or of its per-row optimiser state, as
        [rows, width] float32 (width 1 for the per-row scalars)."""
        out = np.empty((max(int(rows), 0), self._row_width(name)), dtype=np.float32)
        buf = out if out.size else np.empty(1, dtype=np.float32)      # (an empty range still passes a buffer: NULL is refused)
        check(lib().nvsm_get_param_rows(self._h, name.encode(), int(first_row), int(rows), buf.ctypes.data))
        return out

    def set_param_rows(self, name, first_row, value):
        """nvsm_set_param_rows: `value` ([rows, width] or flat) replaces the rows from first_row on."""
        v = np.ascontiguousarray(value, dtype=np.float32).ravel()
        width = self._row_width(name)
        if v.size % width:
            raise ValueError("%d values are no whole rows of width %d" % (v.size, width))
        check(lib().nvsm_set_param_rows(self._h, name.encode(), int(first_row), v.size // width, v.ctypes.data))

    def get_data(self):
        """ModelBase::get_data() (cpp/model.cu:64-93): the four tensors the HDF5 writer dumps."""
        return {n: self.get_param(n) for n in PARAM_NAMES}

    def get_tensor(self, name):
        n = C.c_int64()
        check(lib().nvsm_tensor_size(self._h, name.encode(), C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        check(lib().nvsm_get_tensor(self._h, name.encode(), out.ctypes.data, n.value))
        return out

    # -- runtime -----------------------------------------------------------------------------------
    def synchronize(self):
        check(lib().nvsm_synchronize(self._h))

    def set_stream(self, stream_ptr):
        check(lib().nvsm_set_stream(self._h, stream_ptr))

    def comm_init(self, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(lib().nvsm_comm_init(self._h, buf))

    def describe(self, batch=None):
        """Which kernels a step of `batch` windows takes on this handle, table modes, switches off their defaults (nvsm_describe)."""
        buf = C.create_string_buffer(2048)
        check(lib().nvsm_describe(self._h, int(batch if batch is not None else self.cfg.max_batch_size), buf, 2048))
        return buf.value.decode()

    def comm_size(self):
        """Ranks of the engine's RCCL communicator as ncclCommCount reports them (0: none built)."""
        n = C.c_int()
        check(lib().nvsm_comm_size(self._h, C.byref(n)))
        return n.value

    def dp_average_tables(self):
        """Collective: word / document tables ← mean over the ranks' replicas (see include/cunvsm_amd.h)."""
        check(lib().nvsm_dp_average_tables(self._h))

    def set_allreduce_callback(self, fn):
        """fn(numpy float64 array) must sum the array in place across ranks."""
        def tramp(ptr, n, _user):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(n,)))
                return 0
            except Exception:  # pragma: no cover
                return 1
        self._cb = _lib.ALLREDUCE_FN(tramp)
        check(lib().nvsm_set_allreduce_callback(self._h, self._cb, None))

    def profile_enable(self, on=True):
        check(lib().nvsm_profile_enable(self._h, int(on)))

    def profile_select(self, kernel=None):
        """Time only this kernel group (None = all of them)."""
        check(lib().nvsm_profile_select(self._h, kernel.encode() if kernel else None))

    def debug_delay(self, microseconds):
        """Spin kernel on the model's stream (profiling aid: lets the host queue a whole step ahead of the GPU)."""
        check(lib().nvsm_debug_delay(self._h, int(microseconds)))

    def profile_reset(self):
        check(lib().nvsm_profile_reset(self._h))

    def profile(self):
        """{kernel name: (total_ms, launches)} measured with HIP events on the model's stream."""
        buf = C.create_string_buffer(1 << 14)
        check(lib().nvsm_profile_names(self._h, buf, len(buf)))
        names = [n.decode() for n in buf.raw.split(b"\0\0")[0].split(b"\0") if n]
        out = {}
        for n in names:
            ms, cnt = C.c_double(), C.c_int64()
            check(lib().nvsm_profile_get(self._h, n.encode(), C.byref(ms), C.byref(cnt)))
            out[n] = (ms.value, cnt.value)
        return out


def comm_unique_id():
    buf = C.create_string_buffer(128)
    check(lib().nvsm_comm_unique_id(buf))
    return buf.raw
