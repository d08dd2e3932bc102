"""Cross filter requests by resource without a GPU (include/gck.h gck_filter_cross_cols_device):
libgck.so and the driver export the entry points, gck.h declares them with the argument lists of the
ABI — the cross device call's, with `sel` between now_us and d_out_packed, as the row form —, the
Python mirror agrees, gck_select_cols' layout included, the hook refuses what the entry points' rule
function refuses, the row form's declarations are as they were, and the ABI version stays."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

from gochugaru_amd import engine as E
from tests.test_device_cross_filter_abi import _HEAD, _SUBMIT, _SYNC, _TAIL, CROSS, CTYPES, _declarations, _declared
from tests.test_device_cross_filter_abi import DECLARED as ROWS_DECLARED
from tests.test_device_cross_filter_abi import FIELDS as ROWS_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SEL = ["const gck_select_cols* sel"]
DECLARED = {"gck_filter_cross_cols_device": _HEAD + _SEL + _TAIL + _SYNC,
            "gck_filter_submit_cross_cols_device": _HEAD + _SEL + _TAIL + _SUBMIT}
COLS_CTYPES = dict(CTYPES, **{"const gck_select_cols*": (ctypes.POINTER(E.SelectCols),)})

FIELDS = ["uint32_t mask", "uint32_t col_limit", "uint32_t* d_out_col_off", "uint32_t* d_out_col_n",
          "uint32_t* d_out_ids", "uint32_t* d_out_row", "uint8_t* d_out_perm", "size_t cap", "uint32_t* d_out_n"]


def test_libraries_export_the_symbols():
    lib = E.load_library()
    for name in list(DECLARED) + ["gck_test_select_cols"]:
        assert hasattr(lib, name), name
    drv = ctypes.CDLL(os.path.join(os.path.dirname(E.__file__), "libgck_driver.so"))
    assert hasattr(drv, "gckd_run_filter_cross_cols_device")
    assert hasattr(E._driver(), "gckd_run_filter_cross_cols_device")
    for name in ("filter_cross_cols_device", "submit_filter_cross_cols_device", "prepare_filter_cross_cols_device",
                 "filter_cross_cols_ids"):
        assert callable(getattr(E.Engine, name)), name
    assert issubclass(E.PreparedFilterCrossColsDevice, E._Prepared)
    from gochugaru_amd.client import Client
    assert callable(getattr(Client, "FilterCrossSubjectsDevice"))


def test_header_declares_the_argument_lists():
    text = _declarations()
    for name, want in DECLARED.items():
        assert _declared(text, name) == want, name
    # no existing call changed: the row form's and the cross device call's lists are as they were
    for name, want in list(ROWS_DECLARED.items()) + list(CROSS.items()):
        assert _declared(text, name) == want, name
    assert re.search(r"#define GCK_ABI_VERSION 13\b", text)  # additive: the ABI version stays
    assert E.load_library().gck_abi_version() == 13


def test_python_mirror_matches_the_declarations():
    for name, params in DECLARED.items():
        restype, argtypes = E._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            t, _ = p.rsplit(" ", 1)
            assert a in COLS_CTYPES[t], (name, p, a)
    loop, rows = E._driver().gckd_run_filter_cross_cols_device, E._driver().gckd_run_filter_cross_device
    assert loop.restype is ctypes.c_int and len(loop.argtypes) == 28 and list(loop.argtypes) == list(rows.argtypes)


def test_select_cols_fields_match_the_header():
    text = _declarations()
    m = re.search(r"typedef struct gck_select_cols \{(.*?)\} gck_select_cols;", text, flags=re.S)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == FIELDS
    assert [n for n, _ in E.SelectCols._fields_] == [f.rsplit(" ", 1)[1] for f in fields]
    # gck_select_rows has no spare field and is unchanged
    m = re.search(r"typedef struct gck_select_rows \{(.*?)\} gck_select_rows;", text, flags=re.S)
    assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == ROWS_FIELDS


def test_select_cols_layout_matches_the_c_struct(tmp_path):
    """sizeof and every offsetof of gck_select_cols, from a C program compiled against the header."""
    names = [n for n, _ in E.SelectCols._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gck.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gck_select_cols));\n'
                   + "".join(f'  printf(" %zu", offsetof(gck_select_cols, {n}));\n' for n in names)
                   + '  printf(" %zu %d", sizeof(gck_select_rows), GCK_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sys.maxsize > 2 ** 32  # (a 64-bit layout)
    assert got[0] == ctypes.sizeof(E.SelectCols) == 64
    assert got[1:1 + len(names)] == [getattr(E.SelectCols, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert got[-2:] == [64, 13]


def test_hook_rejects_what_the_rule_function_rejects():
    """gck_test_select_cols goes through the entry points' own rule function (select_cols_fault): a bad
    mask, and cap > 0 with all three record arrays NULL, are -1 with nothing written."""
    fn = E.load_library().gck_test_select_cols
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p]
    words = np.full(3, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)  # 3 x 2, all HAS (and garbage padding)
    src = np.arange(3, dtype=np.uint32)
    col_off, ids = np.full(4, 0xDEADBEEF, dtype=np.uint32), np.full(8, 0xDEADBEEF, dtype=np.uint32)
    n = ctypes.c_uint32(0x7777)

    def call(mask, cap, out_ids):
        return fn(words.ctypes.data, 3, 2, mask, 0, cap, src.ctypes.data, col_off.ctypes.data, None, out_ids, None,
                  None, ctypes.byref(n))

    for mask in (0, 1, 0xF, 0x10, 0x12):
        assert call(mask, 8, ids.ctypes.data) == -1, mask
    assert call(E.SELECT_LOOKUP, 8, None) == -1
    assert (col_off == 0xDEADBEEF).all() and (ids == 0xDEADBEEF).all() and n.value == 0x7777
    assert call(E.SELECT_LOOKUP, 8, ids.ctypes.data) == 0
    assert n.value == 6 and col_off[:3].tolist() == [0, 3, 6] and ids[:6].tolist() == [0, 1, 2, 0, 1, 2]
    assert call(E.SELECT_LOOKUP, 0, None) == 0  # cap == 0 needs no record array
