"""CPU-side checks of the feedback boundary (nvsm_lexical_rank_weighted, nvsm_relevance_model, nvsm_lexical_rank_prf,
nvsm_rank_ensemble_prf and nvsm_feedback_options): the symbols are declared and exported, the ctypes struct has the C size and the
older structs did not move, the defaults are the header's, null arguments are status codes that name the argument, the C++ wrapper
compiles, and the Python layer refuses without a device what needs none."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_feedback_options_default", "nvsm_lexical_rank_weighted", "nvsm_relevance_model", "nvsm_lexical_rank_prf", "nvsm_rank_ensemble_prf")


def test_the_header_declares_and_the_library_exports_the_feedback_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n


def test_struct_sizes_match_the_header_and_the_older_structs_did_not_move(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",\n'
                   '  sizeof(nvsm_feedback_options), offsetof(nvsm_feedback_options, fb_docs), offsetof(nvsm_feedback_options, fb_terms),\n'
                   '  offsetof(nvsm_feedback_options, orig_weight), offsetof(nvsm_feedback_options, reserved),\n'
                   '  sizeof(nvsm_lexical_options), sizeof(nvsm_ensemble_options), sizeof(nvsm_config), sizeof(nvsm_batch),\n'
                   '  sizeof(nvsm_rank_options), sizeof(nvsm_queries), sizeof(nvsm_judgments), sizeof(nvsm_corpus),\n'
                   '  NVSM_FEEDBACK_MAX_DOCS, NVSM_LEXICAL_MAX_QUERY_TERMS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F = ca.NvsmFeedbackOptions
    assert got[0] == C.sizeof(F) == 32
    assert got[1:5] == [F.fb_docs.offset, F.fb_terms.offset, F.orig_weight.offset, F.reserved.offset] == [0, 4, 8, 12]
    assert got[5:7] == [C.sizeof(ca.NvsmLexicalOptions), C.sizeof(ca.NvsmEnsembleOptions)] == [32, 32]
    assert got[7:9] == [112, 48]                                          # nvsm_config and nvsm_batch did not move
    assert got[9:13] == [C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmJudgments), C.sizeof(ca.NvsmCorpus)]
    assert got[9:13] == [48, 32, 48, 64]
    assert got[13] == ca.FEEDBACK_MAX_DOCS == 1024 and got[14] == 1024


def test_defaults():
    L = ca.lib()
    fb = ca.NvsmFeedbackOptions()
    C.memset(C.byref(fb), 0xFF, C.sizeof(fb))
    L.nvsm_feedback_options_default(C.byref(fb))
    assert (fb.fb_docs, fb.fb_terms, fb.orig_weight, list(fb.reserved)) == (10, 10, 0.5, [0] * 5)
    L.nvsm_feedback_options_default(None)                                 # a null pointer is ignored, as by the other defaults
    lex = ca.NvsmLexicalOptions()                                         # the lexical options keep their reserved words
    L.nvsm_lexical_options_default(C.byref(lex))
    assert list(lex.reserved) == [0] * 5


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, ro, lo, eo, fo, j = (ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmEnsembleOptions(), ca.NvsmFeedbackOptions(),
                            ca.NvsmJudgments())
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = (C.c_int64 * 4)()
    o = C.cast(out, C.c_void_p)
    weights = (C.c_float * 4)()
    q.word_weights = C.cast(weights, C.c_void_p)

    def refused(call, args, at, name):
        args = list(args)
        args[at] = None
        assert call(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), (name, L.nvsm_last_error())

    weighted = [fake, C.byref(q), C.byref(lo), o, o, o]
    for at, name in enumerate(("m", "queries", "lex", "doc_ids", "scores", "counts")):
        refused(L.nvsm_lexical_rank_weighted, weighted, at, name)
    unweighted = ca.NvsmQueries()                                         # the weighted call wants the weights, and says so
    assert L.nvsm_lexical_rank_weighted(fake, C.byref(unweighted), C.byref(lo), o, o, o) == 1
    assert b"null argument: queries->word_weights" in L.nvsm_last_error()
    model = [fake, C.byref(q), C.byref(lo), C.byref(fo), o, o, o]
    for at, name in enumerate(("m", "queries", "lex", "fb", "term_ids", "term_probs", "counts")):
        refused(L.nvsm_relevance_model, model, at, name)
    for at, name in enumerate(("m", "queries", "lex", "fb", "doc_ids", "scores", "counts")):
        refused(L.nvsm_lexical_rank_prf, model, at, name)
    ensemble = [fake, C.byref(q), C.byref(ro), C.byref(lo), C.byref(fo), C.byref(eo), None, None, o, o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "lex"), (4, "fb"), (5, "ens"), (8, "doc_ids"), (9, "scores"), (10, "counts")):
        refused(L.nvsm_rank_ensemble_prf, ensemble, at, name)
    args = list(ensemble)                   # judgments and metrics come together
    args[6] = C.byref(j)
    assert L.nvsm_rank_ensemble_prf(*args) == 1 and b"null argument: metrics" in L.nvsm_last_error()
    args = list(ensemble)
    args[7] = o
    assert L.nvsm_rank_ensemble_prf(*args) == 1 and b"null argument: judgments" in L.nvsm_last_error()


def test_the_cpp_wrapper_compiles_with_the_feedback_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const std::vector<int64_t>& w, const std::vector<int64_t>& o, const std::vector<float>& x,\n'
                   '       const nvsm_judgments& j) {\n'
                   '  nvsm_lexical_options lex; nvsm_lexical_options_default(&lex); nvsm_ensemble_options ens; nvsm_ensemble_options_default(&ens);\n'
                   '  nvsm_rank_options r; nvsm_rank_options_default(&r); nvsm_feedback_options fb; nvsm_feedback_options_default(&fb);\n'
                   '  cunvsm_amd::Model::Ranking a = m.lexical_rank_weighted(w, o, x, lex); (void)a;\n'
                   '  cunvsm_amd::Model::RelevanceModel t = m.relevance_model(w, o, lex, fb); (void)t.term_ids; (void)t.term_probs; (void)t.counts;\n'
                   '  a = m.lexical_rank_prf(w, o, lex, fb);\n'
                   '  cunvsm_amd::Model::Evaluation e = m.rank_ensemble_prf(w, o, r, lex, fb, ens, &j); (void)e;\n'
                   '  e = m.rank_ensemble_prf(w, o, r, lex, fb, ens); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_checks_need_no_device():
    fb = cm.feedback_options()
    assert (fb.fb_docs, fb.fb_terms, fb.orig_weight) == (10, 10, 0.5)
    fb = cm.feedback_options(3, 25, 0.25)
    assert (fb.fb_docs, fb.fb_terms, fb.orig_weight) == (3, 25, 0.25)
    assert cm.feedback_options(ca.FEEDBACK_MAX_DOCS).fb_docs == 1024
    for bad in (dict(fb_docs=0), dict(fb_docs=1025), dict(fb_terms=0), dict(orig_weight=-0.1), dict(orig_weight=1.5),
                dict(orig_weight=float("nan"))):
        with pytest.raises(ValueError):
            cm.feedback_options(**bad)
    assert cm.as_feedback_options(True).fb_terms == 10 and cm.as_feedback_options((2, 3, 1.0)).fb_docs == 2
    assert cm.as_feedback_options(dict(fb_terms=7)).fb_terms == 7 and cm.as_feedback_options(fb) is fb
    q = cm.weighted_queries([[1, 2], [], [3]], [[0.0, 2.5], [], [0.0]])   # weights that sum to zero are a query that retrieves nothing
    assert q.word_weights.dtype == np.float32 and list(q.word_weights) == [0.0, 2.5, 0.0] and q.as_struct().word_weights
    assert cm.weighted_queries([[]], [[]]).as_struct().word_weights       # a pointer even where there is nothing to read
    for bad in ([[1.0]], [[1.0, -2.0]], [[1.0, float("inf")]], [[float("nan"), 1.0]], [[1.0, 1.0], [1.0]]):
        with pytest.raises(ValueError):
            cm.weighted_queries([[1, 2]], bad)
