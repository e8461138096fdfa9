"""CPU-side checks of the TF-IDF / re-ranking boundary (nvsm_tfidf_rank, nvsm_rerank and their option structs): the symbols are
declared and exported, the ctypes structs have the C sizes and the older structs did not move, the defaults are the header's, null
arguments are status codes that name the argument, the C++ wrapper compiles, and the Python layer refuses without a device what
needs none."""
import ctypes as C
import os
import subprocess

import pytest

import cunvsm_amd as ca
from cunvsm_amd import _lib
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_tfidf_options_default", "nvsm_rerank_options_default", "nvsm_tfidf_rank", "nvsm_rerank")


def test_the_header_declares_and_the_library_exports_the_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n
    assert "nvsm_debug_lex_df" in _lib.hook_symbols() and " T nvsm_debug_lex_df" not in exported      # the hook is not in the product


def test_struct_sizes_match_the_header_and_the_older_structs_did_not_move(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n",\n'
                   '  sizeof(nvsm_tfidf_options), sizeof(nvsm_rerank_options), sizeof(nvsm_lexical_options), sizeof(nvsm_rank_options),\n'
                   '  sizeof(nvsm_queries), sizeof(nvsm_judgments),\n'
                   '  offsetof(nvsm_tfidf_options, idf), offsetof(nvsm_tfidf_options, top_k), offsetof(nvsm_rerank_options, depth),\n'
                   '  offsetof(nvsm_rerank_options, tfidf), offsetof(nvsm_rerank_options, lexical),\n'
                   '  NVSM_IDF_ROBERTSON, NVSM_IDF_OKAPI, NVSM_STAGE_TFIDF, NVSM_STAGE_LEXICAL, NVSM_RERANK_MAX_DEPTH); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:2] == [C.sizeof(ca.NvsmTfidfOptions), C.sizeof(ca.NvsmRerankOptions)] == [32, 40]
    assert got[2:6] == [C.sizeof(ca.NvsmLexicalOptions), C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmJudgments)]
    assert got[2:6] == [32, 48, 32, 48]                                   # the older structs did not move
    assert got[6:8] == [ca.NvsmTfidfOptions.idf.offset, ca.NvsmTfidfOptions.top_k.offset] == [8, 12]
    assert got[8:11] == [ca.NvsmRerankOptions.depth.offset, ca.NvsmRerankOptions.tfidf.offset, ca.NvsmRerankOptions.lexical.offset] == [4, 8, 16]
    assert got[11:15] == [ca.IDF_ROBERTSON, ca.IDF_OKAPI, ca.STAGE_TFIDF, ca.STAGE_LEXICAL] == [0, 1, 0, 1]
    assert got[15] == ca.RERANK_MAX_DEPTH == 4096


def test_defaults():
    L = ca.lib()
    tf, rr = ca.NvsmTfidfOptions(), ca.NvsmRerankOptions()
    C.memset(C.byref(tf), 0xFF, C.sizeof(tf))
    C.memset(C.byref(rr), 0xFF, C.sizeof(rr))
    L.nvsm_tfidf_options_default(C.byref(tf))
    L.nvsm_rerank_options_default(C.byref(rr))
    assert (tf.k1, tf.b, tf.idf, tf.top_k, list(tf.reserved)) == (0.0, 0.0, ca.IDF_ROBERTSON, 1000, [0] * 4)
    assert (rr.first_stage, rr.depth, bool(rr.tfidf), bool(rr.lexical), list(rr.reserved)) == (ca.STAGE_TFIDF, 1000, False, False, [0] * 4)
    L.nvsm_tfidf_options_default(None)                                    # a null pointer is ignored, as by the other defaults
    L.nvsm_rerank_options_default(None)


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, ro, to, rr, j = ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmTfidfOptions(), ca.NvsmRerankOptions(), ca.NvsmJudgments()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = (C.c_int64 * 4)()
    o = C.cast(out, C.c_void_p)
    tfidf = [fake, C.byref(q), C.byref(to), o, o, o]
    for at, name in enumerate(("m", "queries", "opt", "doc_ids", "scores", "counts")):
        args = list(tfidf)
        args[at] = None
        assert L.nvsm_tfidf_rank(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    rerank = [fake, C.byref(q), C.byref(ro), C.byref(rr), None, None, o, o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "rr"), (6, "doc_ids"), (7, "scores"), (8, "counts")):
        args = list(rerank)
        args[at] = None
        assert L.nvsm_rerank(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    # judgments and metrics come together
    args = list(rerank)
    args[4] = C.byref(j)
    assert L.nvsm_rerank(*args) == 1 and b"null argument: metrics" in L.nvsm_last_error()
    args = list(rerank)
    args[5] = o
    assert L.nvsm_rerank(*args) == 1 and b"null argument: judgments" in L.nvsm_last_error()


def test_the_cpp_wrapper_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const std::vector<int64_t>& w, const std::vector<int64_t>& o, const std::vector<float>& x,\n'
                   '       const nvsm_judgments& j) {\n'
                   '  nvsm_tfidf_options tf; nvsm_tfidf_options_default(&tf); nvsm_rerank_options rr; nvsm_rerank_options_default(&rr);\n'
                   '  nvsm_rank_options r; nvsm_rank_options_default(&r); rr.tfidf = &tf;\n'
                   '  cunvsm_amd::Model::Ranking a = m.tfidf_rank(w, o, tf); a = m.tfidf_rank(w, o, tf, &x);\n'
                   '  cunvsm_amd::Model::Evaluation e = m.rerank(w, o, r, rr, &j); (void)e;\n'
                   '  e = m.rerank(w, o, r, rr); e = m.rerank(w, o, r, rr, nullptr, &x); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_checks_need_no_device():
    tf = cm.tfidf_options(0.9, 0.4, "okapi", 10)
    assert (round(tf.k1, 6), round(tf.b, 6), tf.idf, tf.top_k) == (0.9, 0.4, ca.IDF_OKAPI, 10)
    auto = cm.tfidf_options()
    assert (auto.k1, auto.b, auto.idf, auto.top_k) == (0.0, 0.0, ca.IDF_ROBERTSON, 1000)
    assert cm.tfidf_options("auto", "auto").k1 == 0.0 and cm.tfidf_options(b=1.0).b == 1.0
    for bad in (dict(idf="bm25"), dict(k1=-0.5), dict(k1=float("nan")), dict(k1=float("inf")), dict(b=1.5), dict(b=-0.1),
                dict(b=float("nan")), dict(top_k=0)):
        with pytest.raises(ValueError):
            cm.tfidf_options(**bad)
