"""Cross filter requests without a GPU (include/gck.h gck_filter_cross_device): libgck.so and the
driver export the entry points, gck.h declares them with the argument lists of the ABI — the cross
device call's, with `sel` between now_us and d_out_packed — the Python mirror agrees, gck_select_rows'
layout included, and the ABI version stays."""
import ctypes
import os
import re
import subprocess
import sys

from gochugaru_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "const uint32_t* d_subjects",
         "size_t n_subjects", "const uint32_t* d_resources", "size_t n_resources", "const char* const* contexts",
         "const size_t* context_lens", "size_t n_contexts", "int64_t now_us"]
_TAIL = ["uint64_t* d_out_packed", "gck_item_error* d_out_errs", "size_t err_cap", "uint32_t* d_out_n_errs"]
_SYNC, _SUBMIT = ["void* stream", "uint64_t* out_revision"], ["uint32_t flags", "void* stream", "gck_batch** out"]
_SEL = ["const gck_select_rows* sel"]
DECLARED = {"gck_filter_cross_device": _HEAD + _SEL + _TAIL + _SYNC,
            "gck_filter_submit_cross_device": _HEAD + _SEL + _TAIL + _SUBMIT}
CROSS = {"gck_check_bulk_cross_device": _HEAD + _TAIL + _SYNC, "gck_check_submit_cross_device": _HEAD + _TAIL + _SUBMIT}

CTYPES = {"gck_engine*": (ctypes.c_void_p,), "const gck_consistency*": (ctypes.POINTER(E._Consistency),),
          "const gck_uniform*": (ctypes.POINTER(E.Uniform),), "uint32_t": (ctypes.c_uint32,),
          "const uint32_t*": (ctypes.c_void_p,), "uint32_t*": (ctypes.c_void_p,), "size_t": (ctypes.c_size_t,),
          "const char* const*": (ctypes.POINTER(ctypes.c_char_p),), "const size_t*": (ctypes.POINTER(ctypes.c_size_t),),
          "int64_t": (ctypes.c_int64,), "const gck_select_rows*": (ctypes.POINTER(E.SelectRows),),
          "uint64_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), "gck_item_error*": (ctypes.c_void_p,),
          "void*": (ctypes.c_void_p,), "gck_batch**": (ctypes.POINTER(ctypes.c_void_p),)}

FIELDS = ["uint32_t mask", "uint32_t row_limit", "uint32_t* d_out_row_off", "uint32_t* d_out_row_n",
          "uint32_t* d_out_ids", "uint32_t* d_out_col", "uint8_t* d_out_perm", "size_t cap", "uint32_t* d_out_n"]


def _declarations():
    with open(os.path.join(ROOT, "include", "gck.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _declared(text, name):
    m = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_libraries_export_the_cross_filter_symbols():
    lib = E.load_library()
    for name in list(DECLARED) + ["gck_test_select_rows"]:
        assert hasattr(lib, name), name
    drv = ctypes.CDLL(os.path.join(os.path.dirname(E.__file__), "libgck_driver.so"))
    assert hasattr(drv, "gckd_run_filter_cross_device")
    assert hasattr(E._driver(), "gckd_run_filter_cross_device")
    for name in ("filter_cross_device", "submit_filter_cross_device", "prepare_filter_cross_device",
                 "filter_cross_ids"):
        assert callable(getattr(E.Engine, name)), name
    assert issubclass(E.PreparedFilterCrossDevice, E._Prepared)
    from gochugaru_amd.client import Client
    assert callable(getattr(Client, "FilterCrossDevice"))


def test_header_declares_the_argument_lists():
    text = _declarations()
    for name, want in DECLARED.items():
        assert _declared(text, name) == want, name
    # the cross device call's own lists, with `sel` where gck_filter_list_device puts its own
    for name, want in CROSS.items():
        assert _declared(text, name) == want, name
    at = _declared(text, "gck_filter_list_device")
    assert at[at.index("int64_t now_us") + 1] == "const gck_select* sel" and at[at.index("const gck_select* sel") + 1] == _TAIL[0]
    assert re.search(r"#define GCK_ABI_VERSION 13\b", text)  # additive: the ABI version stays
    assert E.load_library().gck_abi_version() == 13


def test_python_mirror_matches_the_declarations():
    for name, params in DECLARED.items():
        restype, argtypes = E._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            t, _ = p.rsplit(" ", 1)
            assert a in CTYPES[t], (name, p, a)
    loop = E._driver().gckd_run_filter_cross_device
    assert loop.restype is ctypes.c_int and len(loop.argtypes) == 28


def test_select_rows_fields_match_the_header():
    text = _declarations()
    m = re.search(r"typedef struct gck_select_rows \{(.*?)\} gck_select_rows;", text, flags=re.S)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == FIELDS
    assert [n for n, _ in E.SelectRows._fields_] == [f.rsplit(" ", 1)[1] for f in fields]


def test_select_rows_layout_matches_the_c_struct(tmp_path):
    """sizeof and every offsetof of gck_select_rows, from a C program compiled against the header."""
    names = [n for n, _ in E.SelectRows._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gck.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gck_select_rows));\n'
                   + "".join(f'  printf(" %zu", offsetof(gck_select_rows, {n}));\n' for n in names)
                   + '  printf(" %d", GCK_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sys.maxsize > 2 ** 32  # (a 64-bit layout)
    assert got[0] == ctypes.sizeof(E.SelectRows) == 64
    assert got[1:1 + len(names)] == [getattr(E.SelectRows, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert got[-1] == 13
