"""Filter requests without a GPU (include/gck.h gck_filter_list_device): libgck.so and the driver
export the entry points, gck.h declares them with the argument lists of the ABI, the Python mirror
agrees — gck_select's layout and the GCK_SELECT_* values included — and the ABI version stays."""
import ctypes
import os
import re
import subprocess
import sys

from gochugaru_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "uint32_t fixed_id", "uint32_t vary",
         "const uint32_t* d_ids", "uint32_t first_id", "size_t n", "const char* const* contexts",
         "const size_t* context_lens", "size_t n_contexts", "int64_t now_us", "const gck_select* sel",
         "uint64_t* d_out_packed", "gck_item_error* d_out_errs", "size_t err_cap", "uint32_t* d_out_n_errs"]
DECLARED = {"gck_filter_list_device": _HEAD + ["void* stream", "uint64_t* out_revision"],
            "gck_filter_submit_list_device": _HEAD + ["uint32_t flags", "void* stream", "gck_batch** out"]}

CTYPES = {"gck_engine*": (ctypes.c_void_p,), "const gck_consistency*": (ctypes.POINTER(E._Consistency),),
          "const gck_uniform*": (ctypes.POINTER(E.Uniform),), "uint32_t": (ctypes.c_uint32,),
          "const uint32_t*": (ctypes.c_void_p,), "uint32_t*": (ctypes.c_void_p,), "size_t": (ctypes.c_size_t,),
          "const char* const*": (ctypes.POINTER(ctypes.c_char_p),), "const size_t*": (ctypes.POINTER(ctypes.c_size_t),),
          "int64_t": (ctypes.c_int64,), "const gck_select*": (ctypes.POINTER(E.Select),),
          "uint64_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), "gck_item_error*": (ctypes.c_void_p,),
          "void*": (ctypes.c_void_p,), "gck_batch**": (ctypes.POINTER(ctypes.c_void_p),)}


def _declarations():
    with open(os.path.join(ROOT, "include", "gck.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_libraries_export_the_filter_symbols():
    lib = E.load_library()
    for name in list(DECLARED) + ["gck_test_select_plane"]:
        assert hasattr(lib, name), name
    drv = ctypes.CDLL(os.path.join(os.path.dirname(E.__file__), "libgck_driver.so"))
    assert hasattr(drv, "gckd_run_filter_device")
    for name in ("filter_list_device", "submit_filter_list_device", "prepare_filter_device", "filter_ids"):
        assert callable(getattr(E.Engine, name)), name
    from gochugaru_amd.client import Client
    for name in ("FilterResourcesDevice", "FilterSubjectsDevice"):
        assert callable(getattr(Client, name)), name


def test_header_declares_the_argument_lists():
    text = _declarations()
    for name, want in DECLARED.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S)
        assert m, name
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == want, name
    assert re.search(r"#define GCK_ABI_VERSION 13\b", text)  # additive: the ABI version stays
    assert E.load_library().gck_abi_version() == 13


def test_python_mirror_matches_the_declarations():
    for name, params in DECLARED.items():
        restype, argtypes = E._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            t, _ = p.rsplit(" ", 1)
            assert a in CTYPES[t], (name, p, a)


def test_select_values_and_fields_match_the_header():
    text = _declarations()
    m = re.search(r"typedef struct gck_select \{(.*?)\} gck_select;", text, flags=re.S)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["uint32_t mask", "uint32_t reserved", "uint32_t* d_out_ids", "uint32_t* d_out_pos",
                      "uint8_t* d_out_perm", "size_t cap", "uint32_t* d_out_n"]
    assert [n for n, _ in E.Select._fields_] == [f.rsplit(" ", 1)[1] for f in fields]
    assert (E.SELECT_NO, E.SELECT_HAS, E.SELECT_CONDITIONAL, E.SELECT_LOOKUP) == (2, 4, 8, 12)
    for name, perm in (("NO", "NO"), ("HAS", "HAS"), ("CONDITIONAL", "CONDITIONAL")):
        assert re.search(r"#define GCK_SELECT_%s\s+\(1u << GCK_PERM_%s\)" % (name, perm), text), name
    assert re.search(r"#define GCK_SELECT_LOOKUP\s+\(GCK_SELECT_HAS \| GCK_SELECT_CONDITIONAL\)", text)


def test_select_layout_matches_the_c_struct(tmp_path):
    """sizeof and every offsetof of gck_select, from a C program compiled against the header."""
    names = [n for n, _ in E.Select._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gck.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gck_select));\n'
                   + "".join(f'  printf(" %zu", offsetof(gck_select, {n}));\n' for n in names)
                   + '  printf(" %u %u %u %u", GCK_SELECT_NO, GCK_SELECT_HAS, GCK_SELECT_CONDITIONAL, GCK_SELECT_LOOKUP);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == ctypes.sizeof(E.Select)
    assert got[1:1 + len(names)] == [getattr(E.Select, n).offset for n in names]
    assert got[1 + len(names):] == [E.SELECT_NO, E.SELECT_HAS, E.SELECT_CONDITIONAL, E.SELECT_LOOKUP]
    assert sys.maxsize > 2 ** 32  # (a 64-bit layout: 48 bytes)
    assert ctypes.sizeof(E.Select) == 48
