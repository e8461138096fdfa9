"""CPU-side checks of the fold-in entry points at the drop-in boundary (the pattern of tests/test_abi.py): the product library
exports them, the ctypes binding's argument types and struct layout are the header's, and null arguments are status codes."""
import ctypes as C
import os
import re
import subprocess

import cunvsm_amd as ca
from tests.conftest import ROOT

NEW = ["nvsm_fold_options_default", "nvsm_step_fold", "nvsm_fold_summation", "nvsm_get_param_rows", "nvsm_set_param_rows"]
HEADER = os.path.join(ROOT, "include", "cunvsm_amd.h")

# how a C parameter type appears in the binding
CTYPE_OF = {"nvsm_model*": C.c_void_p, "const nvsm_batch*": C.POINTER(ca.NvsmBatch), "const int64_t*": C.c_void_p,
            "const nvsm_fold_options*": C.POINTER(ca.NvsmFoldOptions), "nvsm_fold_options*": C.POINTER(ca.NvsmFoldOptions),
            "float": C.c_float, "float*": None, "const float*": C.c_void_p, "const char*": C.c_char_p, "int64_t": C.c_int64,
            "int32_t*": C.POINTER(C.c_int32)}


def declaration(name):
    with open(HEADER) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(2).split(",")]
    return m.group(1), [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params]


def test_the_library_exports_the_fold_symbols_and_the_header_declares_them():
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
            want = CTYPE_OF[ctype]
            if ctype == "float*":                     # the cost (a float out) or a host destination array
                assert got in (C.POINTER(C.c_float), C.c_void_p), (n, ctype)
            else:
                assert got == want, (n, ctype, got)


def test_fold_options_layout_and_default(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(nvsm_fold_options), offsetof(nvsm_fold_options, first_document), offsetof(nvsm_fold_options, reserved));\n'
                   '    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off_first, off_reserved = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(ca.NvsmFoldOptions) == 32
    assert off_first == ca.NvsmFoldOptions.first_document.offset == 0
    assert off_reserved == ca.NvsmFoldOptions.reserved.offset == 8
    opt = ca.NvsmFoldOptions(first_document=5)
    opt.reserved[2] = 9
    ca.lib().nvsm_fold_options_default(C.byref(opt))
    assert opt.first_document == 0 and list(opt.reserved) == [0] * 6


def test_null_arguments_and_constants():
    L = ca.lib()
    assert L.nvsm_step_fold(None, None, None, None, 0.1, None) == 1
    assert b"null" in L.nvsm_last_error()
    assert L.nvsm_get_param_rows(None, b"x", 0, 0, None) == 1
    assert L.nvsm_set_param_rows(None, b"x", 0, 0, None) == 1
    chunk, group = ca.fold_summation()
    assert chunk >= 1 and group >= 2
    L.nvsm_fold_summation(None, None)              # either may be NULL
