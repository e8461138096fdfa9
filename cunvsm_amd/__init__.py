"""cunvsm_amd — MI355X-native NVSM / LSE training hot path.

Python host-side mirror of cuNVSM's ``Model<TextEntity::Objective>`` (include/cuNVSM/model.h:75-131)
over the C ABI of ``libcunvsm_amd.so`` (include/cunvsm_amd.h). There is no CPU fallback: importing
works anywhere (so that the ABI can be inspected), but creating a model without the HIP library or
without a GPU raises.
"""
from ._lib import (  # noqa: F401
    ADAGRAD, ADAM, ADAM_DENSE_UPDATE, ADAM_DENSE_UPDATE_DENSE_VARIANCE, ADAM_NONE, ADAM_SPARSE, HARD_TANH,
    SAMPLER_DEVICE, SAMPLER_HOST_MINSTD, SGD, TANH, SIM_COSINE, SIM_DOT, ACT_MODEL, ACT_IDENTITY, NvsmBatch, NvsmConfig,
    SPACE_WORDS, SPACE_PROJECTED_WORDS, SPACE_ENTITIES, NvsmNeighborQueries, NvsmNeighborOptions,
    NvsmQueries, NvsmRankOptions, NvsmJudgments, EVAL_MAX_CUTOFFS, NvsmPairBatch, NvsmMixture, NvsmCorpus, NvsmWindowBatch, NvsmError, abi_symbols, build_library,
    bind_host_thread, device_count, lib, library_path,
    NvsmLexicalOptions, NvsmEnsembleOptions, NvsmFeedbackOptions, FEEDBACK_MAX_DOCS, LEX_JM, LEX_DIRICHLET, NORM_STANDARDIZE, NORM_MINMAX, NORM_NONE,
    NvsmSweepOptions, NvsmCvOptions, SWEEP_MAX_ALPHAS, NvsmNgramOptions, NvsmTsneOptions, NvsmTsneSparseOptions, TSNE_MAX_ROWS, TSNE_SPARSE_MAX_ROWS, TSNE_SPARSE_MAX_NEIGHBORS, TSNE_INIT_PCA, TSNE_INIT_GIVEN,
    NvsmSdmOptions, SDM_MAX_WINDOW,
    NvsmKmeansOptions, KMEANS_MAX_CLUSTERS, KMEANS_INIT_PLUSPLUS, KMEANS_INIT_GIVEN,
    NvsmIndexOptions, NvsmIndexInfo, NvsmPositionsInfo, INDEX_AUTO, INDEX_ALWAYS, INDEX_NEVER,
    NvsmTfidfOptions, NvsmRerankOptions, NvsmFoldOptions, IDF_ROBERTSON, IDF_OKAPI, STAGE_TFIDF, STAGE_LEXICAL, RERANK_MAX_DEPTH,
)
from . import dp  # noqa: F401
from .model import Batch, Corpus, WindowBatch, expand_windows, Judgments, Model, PairBatch, Queries, UPDATE_METHODS, default_config, self_information_weights, alpha_grid, ngram_rows, ngram_encode, ngram_decode, ngram_arguments, tsne_arguments, kmeans_arguments, cluster_agreement, grow_documents, fold_summation  # noqa: F401

__all__ = ["Model", "Batch", "Corpus", "WindowBatch", "expand_windows", "NvsmCorpus", "NvsmWindowBatch", "PairBatch", "NvsmPairBatch", "NvsmMixture", "Queries", "Judgments", "self_information_weights", "NvsmQueries", "NvsmRankOptions", "NvsmJudgments", "NvsmNeighborQueries", "NvsmNeighborOptions", "NvsmLexicalOptions", "NvsmEnsembleOptions", "NvsmFeedbackOptions", "NvsmSdmOptions", "NvsmSweepOptions", "NvsmCvOptions", "NvsmNgramOptions", "NvsmTsneOptions", "NvsmTfidfOptions", "NvsmRerankOptions", "NvsmFoldOptions", "NvsmIndexOptions", "NvsmIndexInfo", "NvsmPositionsInfo", "grow_documents", "fold_summation", "tsne_arguments", "NvsmKmeansOptions", "kmeans_arguments", "cluster_agreement", "alpha_grid", "ngram_rows", "ngram_encode", "ngram_decode", "ngram_arguments", "default_config", "UPDATE_METHODS", "NvsmConfig", "NvsmBatch", "NvsmError", "lib",
           "library_path", "build_library", "device_count", "bind_host_thread", "abi_symbols"]
