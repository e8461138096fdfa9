"""ctypes binding of include/cunvsm_amd.h (the stub a maintainer would write)."""
import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.environ.get("CUNVSM_AMD_LIB") or os.path.join(_HERE, "libcunvsm_amd.so")      # override: A/B of two builds
_HEADER = os.path.join(_ROOT, "include", "cunvsm_amd.h")
_HOOKS_SO = os.path.join(_HERE, "libcunvsm_amd_testhooks.so")      # nvsm_debug_*: unit-test / profiling hooks, NOT in the product library
_HOOKS_HEADER = os.path.join(_ROOT, "include", "cunvsm_amd_test_hooks.h")

TANH, HARD_TANH = 0, 1
SGD, ADAGRAD, ADAM = 0, 1, 2
ADAM_NONE, ADAM_SPARSE, ADAM_DENSE_UPDATE, ADAM_DENSE_UPDATE_DENSE_VARIANCE = 0, 1, 2, 3
SAMPLER_HOST_MINSTD, SAMPLER_DEVICE = 0, 1
SIM_COSINE, SIM_DOT = 0, 1
SPACE_WORDS, SPACE_PROJECTED_WORDS, SPACE_ENTITIES = 0, 1, 2
ACT_MODEL, ACT_IDENTITY = -1, -2
LEX_JM, LEX_DIRICHLET = 0, 1
NORM_STANDARDIZE, NORM_MINMAX, NORM_NONE = 0, 1, 2
LEXICAL_MAX_QUERY_TERMS = 1024
ENSEMBLE_MAX_TOP_K = 1024
FEEDBACK_MAX_DOCS = 1024
SWEEP_MAX_ALPHAS = 1024

STATUS = {0: "OK", 1: "INVALID_ARGUMENT", 2: "UNSUPPORTED", 3: "DEVICE", 4: "STATE", 5: "NO_DEVICE"}


class NvsmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("nvsm status %d (%s): %s" % (status, STATUS.get(status, "?"), message))
        self.status = status


class NvsmConfig(C.Structure):
    _fields_ = [
        ("num_words", C.c_int64), ("num_entities", C.c_int64),
        ("word_repr_size", C.c_int32), ("entity_repr_size", C.c_int32),
        ("batch_normalization", C.c_int32), ("nonlinearity", C.c_int32),
        ("clip_sigmoid", C.c_int32), ("bias_negative_samples", C.c_int32),
        ("l2_normalize_phrase_reprs", C.c_int32), ("l2_normalize_entity_reprs", C.c_int32),
        ("window_size", C.c_int32), ("num_random_entities", C.c_int32),
        ("regularization_lambda", C.c_float),
        ("update_method", C.c_int32), ("adam_mode", C.c_int32), ("max_batch_size", C.c_int32),
        ("device", C.c_int32), ("sampler", C.c_int32),
        ("world_size", C.c_int32), ("rank", C.c_int32), ("sync_batch_norm", C.c_int32),
        ("dp_exact_tables", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class NvsmBatch(C.Structure):
    _fields_ = [
        ("features", C.c_void_p), ("feature_weights", C.c_void_p), ("labels", C.c_void_p), ("weights", C.c_void_p),
        ("num_instances", C.c_int64), ("on_device", C.c_int32),
    ]


class NvsmFoldOptions(C.Structure):
    _fields_ = [("first_document", C.c_int64), ("reserved", C.c_int32 * 6)]


INDEX_AUTO, INDEX_ALWAYS, INDEX_NEVER = 0, 1, 2


class NvsmIndexOptions(C.Structure):
    _fields_ = [("use", C.c_int32), ("reserved", C.c_int32 * 7)]


class NvsmIndexInfo(C.Structure):
    _fields_ = [("num_postings", C.c_int64), ("bytes", C.c_int64), ("max_df", C.c_int64), ("use", C.c_int32), ("reserved", C.c_int32 * 9)]


class NvsmPositionsInfo(C.Structure):
    _fields_ = [("num_positions", C.c_int64), ("bytes", C.c_int64), ("reserved", C.c_int32 * 12)]


class NvsmPairBatch(C.Structure):
    _fields_ = [("pairs", C.c_void_p), ("weights", C.c_void_p), ("num_pairs", C.c_int64), ("on_device", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class NvsmCorpus(C.Structure):
    _fields_ = [("tokens", C.c_void_p), ("doc_offsets", C.c_void_p), ("doc_weights", C.c_void_p), ("term_weights", C.c_void_p),
                ("num_tokens", C.c_int64), ("num_documents", C.c_int64), ("reserved", C.c_int32 * 4)]


class NvsmWindowBatch(C.Structure):
    _fields_ = [("refs", C.c_void_p), ("num_instances", C.c_int64), ("on_device", C.c_int32), ("reserved", C.c_int32 * 3)]


class NvsmMixture(C.Structure):
    _fields_ = [("text_weight", C.c_float), ("pair_weight", C.c_float), ("reserved", C.c_int32 * 2)]


class NvsmQueries(C.Structure):
    _fields_ = [("word_ids", C.c_void_p), ("word_weights", C.c_void_p), ("offsets", C.c_void_p), ("num_queries", C.c_int64)]


class NvsmRankOptions(C.Structure):
    _fields_ = [
        ("bias_coefficient", C.c_float), ("activation", C.c_int32), ("similarity", C.c_int32), ("top_k", C.c_int32),
        ("candidates", C.c_void_p), ("candidate_offsets", C.c_void_p),
        ("reserved", C.c_int32 * 4),
    ]


EVAL_MAX_CUTOFFS = 8
# columns of a metric row (include/cunvsm_amd.h NVSM_EVAL_*); then per cutoff j: P, recall, ndcg at EVAL_FIXED + 3 j + {0, 1, 2}
EVAL_NUM_RET, EVAL_NUM_REL, EVAL_NUM_REL_RET, EVAL_AP, EVAL_RPREC, EVAL_RECIP_RANK, EVAL_NDCG, EVAL_FIXED = range(8)


class NvsmJudgments(C.Structure):
    _fields_ = [
        ("doc_ids", C.c_void_p), ("grades", C.c_void_p), ("offsets", C.c_void_p), ("cutoffs", C.c_void_p),
        ("num_cutoffs", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


class NvsmLexicalOptions(C.Structure):
    _fields_ = [("method", C.c_int32), ("param", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32 * 5)]


class NvsmEnsembleOptions(C.Structure):
    _fields_ = [("alpha", C.c_float), ("normalizer", C.c_int32), ("reserved", C.c_int32 * 6)]


SDM_MAX_WINDOW = 64


class NvsmSdmOptions(C.Structure):
    _fields_ = [("w_term", C.c_float), ("w_ordered", C.c_float), ("w_unordered", C.c_float), ("window", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class NvsmFeedbackOptions(C.Structure):
    _fields_ = [("fb_docs", C.c_int32), ("fb_terms", C.c_int32), ("orig_weight", C.c_float), ("reserved", C.c_int32 * 5)]


class NvsmSweepOptions(C.Structure):
    _fields_ = [("alphas", C.c_void_p), ("num_alphas", C.c_int32), ("normalizer", C.c_int32), ("depth", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class NvsmCvOptions(C.Structure):
    _fields_ = [("measure", C.c_int32), ("num_folds", C.c_int32), ("fold_of", C.c_void_p), ("reserved", C.c_int32 * 4)]


IDF_ROBERTSON, IDF_OKAPI = 0, 1
STAGE_TFIDF, STAGE_LEXICAL = 0, 1
RERANK_MAX_DEPTH = 4096


class NvsmTfidfOptions(C.Structure):
    _fields_ = [("k1", C.c_float), ("b", C.c_float), ("idf", C.c_int32), ("top_k", C.c_int32), ("reserved", C.c_int32 * 4)]


class NvsmRerankOptions(C.Structure):
    _fields_ = [("first_stage", C.c_int32), ("depth", C.c_int32), ("tfidf", C.POINTER(NvsmTfidfOptions)),
                ("lexical", C.POINTER(NvsmLexicalOptions)), ("reserved", C.c_int32 * 4)]


class NvsmNeighborQueries(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("vectors", C.c_void_p), ("num_queries", C.c_int64), ("source_space", C.c_int32), ("dim", C.c_int32)]


class NvsmNeighborOptions(C.Structure):
    _fields_ = [
        ("space", C.c_int32), ("similarity", C.c_int32), ("top_k", C.c_int32), ("exclude_self", C.c_int32),
        ("bias_coefficient", C.c_float), ("activation", C.c_int32),
        ("reserved", C.c_int32 * 6),
    ]


class NvsmNgramOptions(C.Structure):
    _fields_ = [
        ("max_cardinality", C.c_int32), ("similarity", C.c_int32), ("top_k", C.c_int32), ("bias_coefficient", C.c_float),
        ("activation", C.c_int32), ("reserved0", C.c_int32), ("vocabulary", C.c_void_p), ("vocabulary_size", C.c_int64),
        ("reserved", C.c_int32 * 4),
    ]


TSNE_MAX_ROWS = 32768
TSNE_INIT_PCA, TSNE_INIT_GIVEN = 0, 1


class NvsmTsneOptions(C.Structure):
    _fields_ = [
        ("space", C.c_int32), ("l2_normalize", C.c_int32), ("ids", C.c_void_p), ("num_rows", C.c_int64),
        ("perplexity", C.c_float), ("early_exaggeration", C.c_float), ("learning_rate", C.c_float), ("min_grad_norm", C.c_float),
        ("max_iter", C.c_int32), ("n_iter_without_progress", C.c_int32), ("init", C.c_int32), ("reserved0", C.c_int32),
        ("init_embedding", C.c_void_p), ("reserved", C.c_int32 * 6),
    ]


TSNE_SPARSE_MAX_ROWS = 1048576
TSNE_SPARSE_MAX_NEIGHBORS = 1024


class NvsmTsneSparseOptions(C.Structure):
    _fields_ = [("n_neighbors", C.c_int32), ("reserved", C.c_int32 * 7)]


KMEANS_MAX_CLUSTERS = 4096
KMEANS_INIT_PLUSPLUS, KMEANS_INIT_GIVEN = 0, 1


class NvsmKmeansOptions(C.Structure):
    _fields_ = [
        ("space", C.c_int32), ("l2_normalize", C.c_int32), ("ids", C.c_void_p), ("num_rows", C.c_int64),
        ("num_clusters", C.c_int32), ("max_iter", C.c_int32), ("tol", C.c_double), ("init", C.c_int32), ("reserved0", C.c_int32),
        ("init_centers", C.c_void_p), ("seed", C.c_int64), ("reserved", C.c_int32 * 6),
    ]


class GemmEpilogueArgs(C.Structure):
    """nvsm_debug_gemm_epilogue_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("kernel", C.c_int), ("b_layout", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("alpha", C.c_float), ("bias", C.c_void_p),
        ("colstats", C.c_void_p), ("rowsq", C.c_void_p), ("rowsq_scale", C.c_float),
        ("pre", C.c_void_p), ("mean", C.c_void_p), ("inv_std", C.c_void_p), ("sums", C.c_void_p), ("n_global", C.c_double),
        ("dbeta", C.c_void_p), ("dgamma", C.c_void_p), ("grad_bias", C.c_void_p),
        ("table", C.c_void_p), ("table_rows", C.c_int64), ("idx", C.c_void_p), ("wts", C.c_void_p), ("window", C.c_int),
        ("A_out", C.c_void_p), ("launched", C.POINTER(C.c_int)),
    ]


class TablePassArgs(C.Structure):
    """nvsm_debug_table_pass_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("table", C.c_int), ("kind", C.c_int), ("rows", C.c_int64), ("dim", C.c_int),
        ("n", C.c_int64), ("keys", C.c_void_p), ("div", C.c_int), ("num_src", C.c_int64),
        ("X", C.c_void_p), ("coef", C.c_void_p), ("sq_src", C.c_void_p), ("src_scale", C.c_void_p),
        ("P", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("sc_in", C.c_void_p), ("sc_out", C.c_void_p),
        ("lr", C.c_float), ("lambda_", C.c_float), ("decay", C.c_float), ("bc", C.c_float), ("dense", C.c_int),
        ("wide", C.c_int), ("nt", C.c_int), ("max_entries", C.c_int64), ("adam", C.c_int),
        ("one_launch", C.c_int), ("chunk_order", C.c_int), ("fill_in_bounds", C.c_int), ("entry_walk_min", C.c_int64),
        ("prev_n", C.c_int64), ("prev_keys", C.c_void_p),
        ("path", C.POINTER(C.c_int)), ("chunk", C.POINTER(C.c_int)), ("num_chunks", C.POINTER(C.c_int)),
        ("max_chunks", C.POINTER(C.c_int)), ("max_chunks2", C.POINTER(C.c_int)), ("arrive_left", C.POINTER(C.c_int)),
        ("stamp", C.c_void_p), ("lazy_decay", C.c_void_p), ("now", C.c_int), ("stamp_out", C.c_void_p),
    ]


class LazyRefreshArgs(C.Structure):
    """nvsm_debug_lazy_refresh_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("rows", C.c_int64), ("dim", C.c_int),
        ("P", C.c_void_p), ("m", C.c_void_p), ("sc", C.c_void_p), ("sc_snapshot", C.c_void_p),
        ("stamp", C.c_void_p), ("stamp_out", C.c_void_p), ("list", C.c_void_p), ("n_list", C.c_int64),
        ("now", C.c_int), ("s_m", C.c_float), ("s_v", C.c_float), ("decay", C.c_void_p), ("scalars_only", C.c_int),
    ]


class LossArgs(C.Structure):
    """nvsm_debug_loss_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("B", C.c_int64), ("de", C.c_int), ("R", C.c_int), ("k", C.c_int),
        ("pre", C.c_void_p), ("bn", C.c_int), ("bn_sums", C.c_void_p), ("bn_n", C.c_double), ("bias", C.c_void_p),
        ("E", C.c_void_p), ("rows", C.c_int64), ("ids", C.c_void_p), ("inst_w", C.c_void_p),
        ("nonlinearity", C.c_int), ("clip_sigmoid", C.c_int), ("bias_negative_samples", C.c_int), ("l2_entity", C.c_int),
        ("b_global", C.c_double),
        ("stamp", C.c_void_p), ("decay", C.c_void_p), ("now", C.c_int), ("rows_for_dispatch", C.c_int64), ("repeats", C.c_int),
        ("proj", C.c_void_p), ("dy", C.c_void_p), ("coef", C.c_void_p), ("probs", C.c_void_p), ("pp", C.c_void_p),
        ("bn_mean", C.c_void_p), ("bn_inv_std", C.c_void_p), ("loss", C.c_void_p), ("colstats", C.c_void_p),
        ("plan", C.POINTER(C.c_int)), ("arrive_left", C.POINTER(C.c_int)),
    ]


class BnDxArgs(C.Structure):
    """nvsm_debug_bn_dx_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("rows", C.c_int64), ("dim", C.c_int),
        ("dy", C.c_void_p), ("pre", C.c_void_p), ("mean", C.c_void_p), ("inv_std", C.c_void_p),
        ("sums", C.c_void_p), ("n_global", C.c_double),
        ("dy_out", C.c_void_p), ("dbeta", C.c_void_p), ("dgamma", C.c_void_p), ("grad_bias", C.c_void_p),
    ]


ROW_MEANSQ, ROW_L2_FORWARD, ROW_L2_BACKWARD, ROW_MATERIALIZE, ROW_MATERIALIZE_L2 = range(5)


class RowOpArgs(C.Structure):
    """nvsm_debug_row_op_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("op", C.c_int), ("rows", C.c_int64), ("dim", C.c_int),
        ("x", C.c_void_p), ("g", C.c_void_p), ("norms", C.c_void_p), ("coef", C.c_void_p),
        ("E", C.c_void_p), ("table_rows", C.c_int64), ("ids", C.c_void_p), ("R", C.c_int),
        ("scale", C.c_float), ("in_place", C.c_int),
        ("out", C.c_void_p), ("out_scalar", C.c_void_p),
    ]


class TransformUpdateArgs(C.Structure):
    """nvsm_debug_transform_update_args (include/cunvsm_amd_test_hooks.h)."""
    _fields_ = [
        ("method", C.c_int), ("dw", C.c_int), ("de", C.c_int),
        ("lr", C.c_float), ("lambda_", C.c_float), ("t_transform", C.c_uint64),
        ("T", C.c_void_p), ("b", C.c_void_p), ("gT", C.c_void_p), ("gb", C.c_void_p),
        ("s0T", C.c_void_p), ("s0b", C.c_void_p), ("s1T", C.c_void_p), ("s1b", C.c_void_p),
        ("partial", C.c_void_p), ("slabs", C.c_int),
        ("plane_kind", C.c_int * 2), ("planes", C.c_void_p * 2), ("fresh", C.c_void_p * 2),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_void_p)


def library_path():
    return _SO


def build_library(force=False):
    """Compiles the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(_SO):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j8"] + (["-B"] if force else []))
    return _SO


def _declared(header):
    with open(header) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nvsm_[a-z0-9_]+)\s*\(", src)) - {"nvsm_allreduce_fn"})


def abi_symbols():
    """Every function the public header declares (used by the CPU-side ABI test)."""
    return _declared(_HEADER)


def hook_symbols():
    """Every function include/cunvsm_amd_test_hooks.h declares: exported by libcunvsm_amd_testhooks.so, never by the product library."""
    return _declared(_HOOKS_HEADER)


class _Library:
    """The product library; a name it does not export (nvsm_debug_*) is looked up in the test-hooks library, loaded on first use."""

    def __init__(self, product):
        self.__dict__["product"] = product
        self.__dict__["hooks"] = None

    def __getattr__(self, name):
        try:
            return getattr(self.product, name)
        except AttributeError:
            if not name.startswith("nvsm_debug_"):
                raise
        if self.hooks is None:
            if not os.path.exists(_HOOKS_SO):
                raise AttributeError("%s lives in %s, which is missing (make -C cunvsm_amd/csrc)" % (name, _HOOKS_SO))
            H = C.CDLL(_HOOKS_SO, mode=C.RTLD_GLOBAL)      # (its launchers resolve against the product library already loaded)
            vp, i64 = C.c_void_p, C.c_int64
            P = C.POINTER
            for hook, (res, args) in {
                "nvsm_debug_delay": (C.c_int, [vp, C.c_int]),
                "nvsm_debug_set_table_pass_form": (C.c_int, [C.c_int]),
                "nvsm_debug_neighbors_force_plain": (C.c_int, [C.c_int]),
                "nvsm_debug_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
                "nvsm_debug_gemm_epilogue": (C.c_int, [P(GemmEpilogueArgs)]),
                "nvsm_debug_table_pass": (C.c_int, [P(TablePassArgs)]),
                "nvsm_debug_loss": (C.c_int, [P(LossArgs)]),
                "nvsm_debug_gemm_plan": (C.c_int, [C.c_int] * 7 + [P(C.c_int), P(C.c_uint)]),
                "nvsm_debug_rank_layout": (C.c_int, [i64] * 5 + [P(i64), P(i64)]),
                "nvsm_debug_gemm_time": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float)]),
                "nvsm_debug_dt_time": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float), P(C.c_float)]),
                "nvsm_debug_sort": (C.c_int, [i64, C.c_int, vp, vp, vp, C.c_int, P(C.c_float)]),
                "nvsm_debug_gather_mean": (C.c_int, [i64, C.c_int, vp, vp, vp, C.c_int, i64, vp]),
                "nvsm_debug_gather_mean_lazy": (C.c_int, [i64, C.c_int, vp, vp, vp, C.c_int, i64, vp, vp, C.c_int, vp, vp]),
                "nvsm_debug_lazy_refresh": (C.c_int, [P(LazyRefreshArgs)]),
                "nvsm_debug_lex_df": (C.c_int, [vp, i64, vp, i64, i64, i64, vp]),
                "nvsm_debug_ngram_rows":(C.c_int, [vp, i64, C.c_int, vp, C.c_float, C.c_int, i64, i64, vp, i64, i64]),
                "nvsm_debug_tsne_affinities": (C.c_int, [vp, i64, C.c_int, C.c_float, vp, vp]),
                "nvsm_debug_tsne_gradient": (C.c_int, [vp, vp, i64, C.c_float, vp, P(C.c_double)]),
                "nvsm_debug_tsne_pca": (C.c_int, [vp, i64, C.c_int, vp]),
                "nvsm_debug_tsne_descent": (C.c_int, [vp, vp, i64, P(NvsmTsneOptions), C.c_int, P(C.c_double), P(C.c_int32)]),
                "nvsm_debug_tsne_knn": (C.c_int, [vp, i64, C.c_int, C.c_int, i64, vp, vp]),
                "nvsm_debug_tsne_sparse_affinities": (C.c_int, [vp, i64, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp]),
                "nvsm_debug_tsne_sparse_gradient": (C.c_int, [vp, vp, vp, vp, i64, C.c_float, C.c_int, vp, P(C.c_double)]),
                "nvsm_debug_tsne_sparse_descent": (C.c_int, [vp, vp, vp, vp, i64, P(NvsmTsneOptions), C.c_int, P(C.c_double), P(C.c_int32)]),
                "nvsm_debug_kmeans_assign": (C.c_int, [vp, i64, C.c_int, vp, C.c_int, vp, vp]),
                "nvsm_debug_kmeans_update": (C.c_int, [vp, i64, C.c_int, vp, vp, C.c_int, vp, vp, P(C.c_double)]),
                "nvsm_debug_kmeans_plusplus": (C.c_int, [vp, i64, C.c_int, C.c_int, i64, vp, vp]),
                "nvsm_debug_adam_u": (C.c_int, [i64, C.c_int, vp, vp, vp, C.c_int, i64, C.c_float, C.c_float, vp]),
                "nvsm_debug_adagrad_scale": (C.c_int, [i64, vp, vp, C.c_int, i64, C.c_float, vp]),
                "nvsm_debug_bn_dx": (C.c_int, [P(BnDxArgs)]),
                "nvsm_debug_row_op": (C.c_int, [P(RowOpArgs)]),
                "nvsm_debug_slab_sum": (C.c_int, [C.c_int, vp, C.c_int, i64, i64, vp]),
                "nvsm_debug_plane_sizes": (C.c_int, [C.c_int, C.c_int, C.c_int, P(i64), P(i64)]),
                "nvsm_debug_transform_update": (C.c_int, [P(TransformUpdateArgs)]),
            }.items():
                fn = getattr(H, hook)
                fn.restype = res
                fn.argtypes = args
            self.__dict__["hooks"] = H
        return getattr(self.hooks, name)


_lib = None


def lib():
    """Loads libcunvsm_amd.so; fails loudly when the HIP extension is missing (no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(cunvsm_amd has no CPU fallback)" % _SO)
    try:
        # PyTorch ships its own libamdhip64 / librccl; load it first so one HIP runtime serves both.
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(_SO, mode=C.RTLD_GLOBAL)
    vp, i64, cp = C.c_void_p, C.c_int64, C.c_char_p
    P = C.POINTER
    sig = {
        "nvsm_last_error": (cp, []), "nvsm_version": (cp, []), "nvsm_device_count": (C.c_int, []),
        "nvsm_config_default": (None, [P(NvsmConfig)]),
        "nvsm_create": (C.c_int, [P(NvsmConfig), P(vp)]), "nvsm_destroy": (None, [vp]),
        "nvsm_initialize": (C.c_int, [vp, C.c_uint64]), "nvsm_initialize_from_rng_state": (C.c_int, [vp]),
        "nvsm_host_alloc": (C.c_int, [C.c_size_t, P(vp)]), "nvsm_host_free": (C.c_int, [vp]),
        "nvsm_bind_host_thread": (C.c_int, [C.c_int, P(C.c_int)]),
        "nvsm_comm_selftest": (C.c_int, [C.c_int]),
        "nvsm_comm_latency": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float), P(i64)]),
        "nvsm_rng_get_state": (C.c_int, [vp, P(C.c_uint64)]), "nvsm_rng_set_state": (C.c_int, [vp, C.c_uint64]),
        "nvsm_param_size": (C.c_int, [vp, cp, P(i64)]),
        "nvsm_get_param": (C.c_int, [vp, cp, vp, i64]), "nvsm_set_param": (C.c_int, [vp, cp, vp, i64]),
        "nvsm_increment_parameter": (C.c_int, [vp, cp, i64, C.c_float]),
        "nvsm_compute_cost": (C.c_int, [vp, P(NvsmBatch), vp]), "nvsm_compute_gradients": (C.c_int, [vp]),
        "nvsm_update": (C.c_int, [vp, C.c_float, C.c_float]), "nvsm_get_cost": (C.c_int, [vp, P(C.c_float)]), "nvsm_get_cost_f64": (C.c_int, [vp, P(C.c_double)]),
        "nvsm_scaled_regularization_lambda": (C.c_float, [vp]),
        "nvsm_step": (C.c_int, [vp, P(NvsmBatch), vp, C.c_float, P(C.c_float)]),
        "nvsm_fold_options_default": (None, [P(NvsmFoldOptions)]),
        "nvsm_step_fold": (C.c_int, [vp, P(NvsmBatch), vp, P(NvsmFoldOptions), C.c_float, P(C.c_float)]),
        "nvsm_fold_summation": (None, [P(C.c_int32), P(C.c_int32)]),
        "nvsm_get_param_rows": (C.c_int, [vp, cp, i64, i64, vp]), "nvsm_set_param_rows": (C.c_int, [vp, cp, i64, i64, vp]),
        "nvsm_compute_cost_mixed": (C.c_int, [vp, P(NvsmBatch), vp, P(NvsmPairBatch), P(NvsmMixture)]),
        "nvsm_step_mixed": (C.c_int, [vp, P(NvsmBatch), vp, P(NvsmPairBatch), P(NvsmMixture), C.c_float, P(C.c_float)]),
        "nvsm_compute_cost_term_mixed": (C.c_int, [vp, P(NvsmBatch), vp, P(NvsmPairBatch), P(NvsmMixture)]),
        "nvsm_step_term_mixed": (C.c_int, [vp, P(NvsmBatch), vp, P(NvsmPairBatch), P(NvsmMixture), C.c_float, P(C.c_float)]),
        "nvsm_corpus_upload": (C.c_int, [vp, P(NvsmCorpus)]),
        "nvsm_index_options_default": (None, [P(NvsmIndexOptions)]),
        "nvsm_corpus_index": (C.c_int, [vp, P(NvsmIndexOptions), P(NvsmIndexInfo)]),
        "nvsm_corpus_index_free": (C.c_int, [vp]),
        "nvsm_corpus_postings": (C.c_int, [vp, i64, i64, vp, vp, P(i64)]),
        "nvsm_corpus_index_positions": (C.c_int, [vp, P(NvsmPositionsInfo)]),
        "nvsm_corpus_index_positions_free": (C.c_int, [vp]),
        "nvsm_corpus_positions": (C.c_int, [vp, i64, i64, i64, vp, P(i64)]),
        "nvsm_compute_cost_windows": (C.c_int, [vp, P(NvsmWindowBatch), vp]),
        "nvsm_step_windows": (C.c_int, [vp, P(NvsmWindowBatch), vp, C.c_float, P(C.c_float)]),
        "nvsm_step_windows_deferred": (C.c_int, [vp, P(NvsmWindowBatch), vp, C.c_float, P(i64)]),
        "nvsm_step_deferred": (C.c_int, [vp, P(NvsmBatch), vp, C.c_float, P(i64)]),
        "nvsm_deferred_cost": (C.c_int, [vp, i64, P(C.c_float)]), "nvsm_wait_inputs": (C.c_int, [vp]),
        "nvsm_tensor_size": (C.c_int, [vp, cp, P(i64)]), "nvsm_get_tensor": (C.c_int, [vp, cp, vp, i64]),
        "nvsm_rank_options_default": (None, [P(NvsmRankOptions)]),
        "nvsm_infer": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), vp]),
        "nvsm_rank": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), vp, vp, vp]),
        "nvsm_evaluate": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmJudgments), vp, vp, vp, vp]),
        "nvsm_lexical_options_default": (None, [P(NvsmLexicalOptions)]),
        "nvsm_ensemble_options_default": (None, [P(NvsmEnsembleOptions)]),
        "nvsm_lexical_rank": (C.c_int, [vp, P(NvsmQueries), P(NvsmLexicalOptions), vp, vp, vp]),
        "nvsm_rank_ensemble": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmLexicalOptions), P(NvsmEnsembleOptions),
                                         P(NvsmJudgments), vp, vp, vp, vp]),
        "nvsm_sdm_options_default": (None, [P(NvsmSdmOptions)]),
        "nvsm_sdm_rank": (C.c_int, [vp, P(NvsmQueries), P(NvsmLexicalOptions), P(NvsmSdmOptions), vp, vp, vp]),
        "nvsm_sdm_pair_counts": (C.c_int, [vp, P(NvsmQueries), P(NvsmSdmOptions), vp, vp]),
        "nvsm_rank_ensemble_sdm": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmLexicalOptions), P(NvsmSdmOptions),
                                             P(NvsmEnsembleOptions), P(NvsmJudgments), vp, vp, vp, vp]),
        "nvsm_feedback_options_default": (None, [P(NvsmFeedbackOptions)]),
        "nvsm_lexical_rank_weighted": (C.c_int, [vp, P(NvsmQueries), P(NvsmLexicalOptions), vp, vp, vp]),
        "nvsm_relevance_model": (C.c_int, [vp, P(NvsmQueries), P(NvsmLexicalOptions), P(NvsmFeedbackOptions), vp, vp, vp]),
        "nvsm_lexical_rank_prf": (C.c_int, [vp, P(NvsmQueries), P(NvsmLexicalOptions), P(NvsmFeedbackOptions), vp, vp, vp]),
        "nvsm_rank_ensemble_prf": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmLexicalOptions), P(NvsmFeedbackOptions),
                                             P(NvsmEnsembleOptions), P(NvsmJudgments), vp, vp, vp, vp]),
        "nvsm_sweep_options_default": (None, [P(NvsmSweepOptions)]), "nvsm_cv_options_default": (None, [P(NvsmCvOptions)]),
        "nvsm_ensemble_sweep": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmLexicalOptions), P(NvsmFeedbackOptions),
                                          P(NvsmSweepOptions), P(NvsmJudgments), vp]),
        "nvsm_rank_ensemble_cv": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmLexicalOptions), P(NvsmFeedbackOptions),
                                            P(NvsmSweepOptions), P(NvsmCvOptions), P(NvsmJudgments), vp, vp, vp, vp, vp, vp, vp]),
        "nvsm_tfidf_options_default": (None, [P(NvsmTfidfOptions)]), "nvsm_rerank_options_default": (None, [P(NvsmRerankOptions)]),
        "nvsm_tfidf_rank": (C.c_int, [vp, P(NvsmQueries), P(NvsmTfidfOptions), vp, vp, vp]),
        "nvsm_rerank": (C.c_int, [vp, P(NvsmQueries), P(NvsmRankOptions), P(NvsmRerankOptions), P(NvsmJudgments), vp, vp, vp, vp]),
        "nvsm_neighbor_options_default": (None, [P(NvsmNeighborOptions)]),
        "nvsm_neighbors": (C.c_int, [vp, P(NvsmNeighborQueries), P(NvsmNeighborOptions), vp, vp, vp]),
        "nvsm_similarity": (C.c_int, [vp, C.c_int32, vp, vp, i64, C.c_int32, vp]),
        "nvsm_ngram_options_default": (None, [P(NvsmNgramOptions)]),
        "nvsm_ngram_rows": (i64, [i64, C.c_int32]),
        "nvsm_ngram_search": (C.c_int, [vp, P(NvsmNeighborQueries), P(NvsmNgramOptions), vp, vp, vp, vp]),
        "nvsm_tsne_options_default": (None, [P(NvsmTsneOptions)]),
        "nvsm_tsne": (C.c_int, [vp, P(NvsmTsneOptions), vp, P(C.c_double), P(C.c_int32)]),
        "nvsm_tsne_sparse_options_default": (None, [P(NvsmTsneSparseOptions)]),
        "nvsm_tsne_sparse": (C.c_int, [vp, P(NvsmTsneOptions), P(NvsmTsneSparseOptions), vp, P(C.c_double), P(C.c_int32)]),
        "nvsm_kmeans_options_default": (None, [P(NvsmKmeansOptions)]),
        "nvsm_kmeans": (C.c_int, [vp, P(NvsmKmeansOptions), vp, vp, vp, vp, P(C.c_double), P(C.c_int32)]),
        "nvsm_set_stream": (C.c_int, [vp, vp]), "nvsm_synchronize": (C.c_int, [vp]),
        "nvsm_describe": (C.c_int, [vp, C.c_int64, C.c_char_p, C.c_int64]),
        "nvsm_comm_unique_id": (C.c_int, [vp]), "nvsm_comm_init": (C.c_int, [vp, vp]),
        "nvsm_set_allreduce_callback": (C.c_int, [vp, ALLREDUCE_FN, vp]),
        "nvsm_comm_size": (C.c_int, [vp, P(C.c_int)]), "nvsm_dp_average_tables": (C.c_int, [vp]),
        "nvsm_range_push": (None, [cp]), "nvsm_range_pop": (None, []),
        "nvsm_profile_enable": (C.c_int, [vp, C.c_int]), "nvsm_profile_reset": (C.c_int, [vp]),
        "nvsm_profile_names": (C.c_int, [vp, vp, i64]), "nvsm_profile_select": (C.c_int, [vp, cp]),
        "nvsm_profile_get": (C.c_int, [vp, cp, P(C.c_double), P(i64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = _Library(L)
    return _lib


def check(status):
    if status != 0:
        raise NvsmError(status, lib().nvsm_last_error().decode())


def device_count():
    return lib().nvsm_device_count()


def bind_host_thread(device=0):
    """nvsm_bind_host_thread: the calling thread onto the CPUs of the device's NUMA node. Returns that node (-1: unknown)."""
    node = C.c_int(-1)
    check(lib().nvsm_bind_host_thread(int(device), C.byref(node)))
    return node.value
