"""CPU-side checks of the inverted-index entry points at the drop-in boundary (the pattern of tests/test_fold_abi.py): the product
library exports them, the ctypes mirrors have the header's sizes and offsets, and null handles are status codes."""
import ctypes as C
import os
import subprocess

import cunvsm_amd as ca
from cunvsm_amd import _lib
from tests.conftest import ROOT
from tests.test_fold_abi import declaration

NEW = ["nvsm_index_options_default", "nvsm_corpus_index", "nvsm_corpus_index_free", "nvsm_corpus_postings"]

CTYPE_OF = {"nvsm_model*": C.c_void_p, "const nvsm_index_options*": C.POINTER(ca.NvsmIndexOptions),
            "nvsm_index_options*": C.POINTER(ca.NvsmIndexOptions), "nvsm_index_info*": C.POINTER(ca.NvsmIndexInfo),
            "int64_t": C.c_int64, "int64_t*": None, "int32_t*": C.c_void_p}


def test_the_library_exports_the_index_symbols_and_the_header_declares_them():
    ca.build_library()
    L = ca.lib()
    declared = ca.abi_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert n in declared, n
        assert hasattr(L, n) and " T " + n in exported, n


def test_binding_argument_types_match_the_header():
    L = ca.lib()
    for n in NEW:
        ret, params = declaration(n)
        fn = getattr(L, n)
        assert fn.restype == (C.c_int if ret == "int" else None), n
        assert len(fn.argtypes) == len(params), (n, params)
        for got, ctype in zip(fn.argtypes, params):
            if ctype == "int64_t*":                   # a host destination array, or the count (an int64 out)
                assert got in (C.POINTER(C.c_int64), C.c_void_p), (n, ctype)
            else:
                assert got == CTYPE_OF[ctype], (n, ctype, got)


def test_struct_layouts_and_the_default(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu ", sizeof(nvsm_index_options), offsetof(nvsm_index_options, use), offsetof(nvsm_index_options, reserved));\n'
                   '    printf("%zu %zu %zu %zu %zu %zu ", sizeof(nvsm_index_info), offsetof(nvsm_index_info, num_postings), offsetof(nvsm_index_info, bytes),\n'
                   '           offsetof(nvsm_index_info, max_df), offsetof(nvsm_index_info, use), offsetof(nvsm_index_info, reserved));\n'
                   '    printf("%d %d %d\\n", NVSM_INDEX_AUTO, NVSM_INDEX_ALWAYS, NVSM_INDEX_NEVER);\n'
                   '    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, I = ca.NvsmIndexOptions, ca.NvsmIndexInfo
    assert got[:3] == [C.sizeof(O), O.use.offset, O.reserved.offset] == [32, 0, 4]
    assert got[3:9] == [C.sizeof(I), I.num_postings.offset, I.bytes.offset, I.max_df.offset, I.use.offset, I.reserved.offset] == [64, 0, 8, 16, 24, 28]
    assert got[9:] == [_lib.INDEX_AUTO, _lib.INDEX_ALWAYS, _lib.INDEX_NEVER] == [0, 1, 2]
    opt = O(use=2)
    opt.reserved[3] = 9
    ca.lib().nvsm_index_options_default(C.byref(opt))
    assert opt.use == _lib.INDEX_AUTO and list(opt.reserved) == [0] * 7
    ca.lib().nvsm_index_options_default(None)


def test_null_handles_are_status_codes():
    L = ca.lib()
    opt, info, n = ca.NvsmIndexOptions(), ca.NvsmIndexInfo(), C.c_int64(-7)
    assert L.nvsm_corpus_index(None, C.byref(opt), C.byref(info)) == 1
    assert b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_corpus_index_free(None) == 1
    assert L.nvsm_corpus_postings(None, 0, 0, None, None, C.byref(n)) == 1 and n.value == -7
