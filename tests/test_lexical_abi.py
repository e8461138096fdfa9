"""CPU-side checks of the lexical-ranking boundary (nvsm_lexical_rank / nvsm_rank_ensemble and their option structs): the symbols
are declared and exported, the ctypes structs have the C sizes and the older structs did not move, the defaults are the header's,
null arguments are status codes that name the argument, the C++ wrapper compiles, and the Python layer refuses without a device
what needs none."""
import ctypes as C
import os
import subprocess

import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_lexical_options_default", "nvsm_ensemble_options_default", "nvsm_lexical_rank", "nvsm_rank_ensemble")


def test_the_header_declares_and_the_library_exports_the_lexical_calls():
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
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n",\n'
                   '  sizeof(nvsm_lexical_options), sizeof(nvsm_ensemble_options), sizeof(nvsm_config), sizeof(nvsm_batch),\n'
                   '  sizeof(nvsm_rank_options), sizeof(nvsm_queries), sizeof(nvsm_judgments), sizeof(nvsm_corpus),\n'
                   '  offsetof(nvsm_lexical_options, top_k), offsetof(nvsm_ensemble_options, normalizer),\n'
                   '  NVSM_LEX_JM, NVSM_LEX_DIRICHLET, NVSM_NORM_STANDARDIZE, NVSM_NORM_MINMAX, NVSM_NORM_NONE,\n'
                   '  NVSM_LEXICAL_MAX_QUERY_TERMS, NVSM_ENSEMBLE_MAX_TOP_K); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:2] == [C.sizeof(ca.NvsmLexicalOptions), C.sizeof(ca.NvsmEnsembleOptions)] == [32, 32]
    assert got[2:4] == [112, 48]                                          # nvsm_config and nvsm_batch did not move
    assert got[4:8] == [C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmJudgments), C.sizeof(ca.NvsmCorpus)]
    assert got[4:8] == [48, 32, 48, 64]
    assert got[8:10] == [ca.NvsmLexicalOptions.top_k.offset, ca.NvsmEnsembleOptions.normalizer.offset] == [8, 4]
    assert got[10:15] == [ca.LEX_JM, ca.LEX_DIRICHLET, ca.NORM_STANDARDIZE, ca.NORM_MINMAX, ca.NORM_NONE]
    assert got[15] == 1024 and got[16] >= 1000                            # the fused path's limit is at least 1000
    from cunvsm_amd import _lib
    assert (_lib.LEXICAL_MAX_QUERY_TERMS, _lib.ENSEMBLE_MAX_TOP_K) == (got[15], got[16])


def test_defaults():
    L = ca.lib()
    lex, ens = ca.NvsmLexicalOptions(), ca.NvsmEnsembleOptions()
    C.memset(C.byref(lex), 0xFF, C.sizeof(lex))
    C.memset(C.byref(ens), 0xFF, C.sizeof(ens))
    L.nvsm_lexical_options_default(C.byref(lex))
    L.nvsm_ensemble_options_default(C.byref(ens))
    assert (lex.method, lex.param, lex.top_k, list(lex.reserved)) == (ca.LEX_JM, 0.0, 1000, [0] * 5)
    assert (ens.alpha, ens.normalizer, list(ens.reserved)) == (0.5, ca.NORM_STANDARDIZE, [0] * 6)
    L.nvsm_lexical_options_default(None)                                  # a null pointer is ignored, as by the other defaults
    L.nvsm_ensemble_options_default(None)


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, ro, lo, eo, j = ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmEnsembleOptions(), ca.NvsmJudgments()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = (C.c_int64 * 4)()
    o = C.cast(out, C.c_void_p)
    lexical = [fake, C.byref(q), C.byref(lo), o, o, o]
    for at, name in enumerate(("m", "queries", "lex", "doc_ids", "scores", "counts")):
        args = list(lexical)
        args[at] = None
        assert L.nvsm_lexical_rank(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    ensemble = [fake, C.byref(q), C.byref(ro), C.byref(lo), C.byref(eo), None, None, o, o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "lex"), (4, "ens"), (7, "doc_ids"), (8, "scores"), (9, "counts")):
        args = list(ensemble)
        args[at] = None
        assert L.nvsm_rank_ensemble(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    # judgments and metrics come together
    args = list(ensemble)
    args[5] = C.byref(j)
    assert L.nvsm_rank_ensemble(*args) == 1 and b"null argument: metrics" in L.nvsm_last_error()
    args = list(ensemble)
    args[6] = o
    assert L.nvsm_rank_ensemble(*args) == 1 and b"null argument: judgments" in L.nvsm_last_error()


def test_the_cpp_wrapper_compiles_with_the_lexical_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const std::vector<int64_t>& w, const std::vector<int64_t>& o, const nvsm_judgments& j) {\n'
                   '  nvsm_lexical_options lex; nvsm_lexical_options_default(&lex); nvsm_ensemble_options ens; nvsm_ensemble_options_default(&ens);\n'
                   '  nvsm_rank_options r; nvsm_rank_options_default(&r);\n'
                   '  cunvsm_amd::Model::Ranking a = m.lexical_rank(w, o, lex); (void)a;\n'
                   '  cunvsm_amd::Model::Evaluation e = m.rank_ensemble(w, o, r, lex, ens, &j); (void)e;\n'
                   '  e = m.rank_ensemble(w, o, r, lex, ens); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_checks_need_no_device():
    lex = cm.lexical_options("dirichlet", 2000, 10)
    assert (lex.method, lex.param, lex.top_k) == (ca.LEX_DIRICHLET, 2000.0, 10)
    assert cm.lexical_options("jm", None).param == 0.0 and cm.lexical_options("jm", "auto").param == 0.0
    assert cm.lexical_options().top_k == 1000
    ens = cm.ensemble_options(0.25, "minmax")
    assert (ens.alpha, ens.normalizer) == (0.25, ca.NORM_MINMAX)
    for bad in (dict(method="bm25"), dict(method="jm", param=1.0), dict(method="jm", param=-0.5), dict(method="dirichlet", param=-1),
                dict(top_k=0)):
        with pytest.raises(ValueError):
            cm.lexical_options(**bad)
    for bad in (dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(normalizer="zscore")):
        with pytest.raises(ValueError):
            cm.ensemble_options(**bad)
