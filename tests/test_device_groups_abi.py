"""Group filter requests without a GPU (include/gck.h gck_filter_groups_device): libgck.so exports the
entry points and the test hooks, gck.h declares them with the argument lists of the ABI, the Python
mirror agrees, gck_select_groups' layout included, the hook refuses what the entry points' rule
function refuses — every item of the header's refusal list —, the cross filter forms' and the list
device call's declarations are as they were, and the ABI version stays."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

from gochugaru_amd import engine as E
from tests.test_device_cross_cols_abi import DECLARED as COLS_DECLARED
from tests.test_device_cross_cols_abi import FIELDS as COLS_FIELDS
from tests.test_device_cross_filter_abi import _SUBMIT, _SYNC, _TAIL, CROSS, CTYPES, _declarations, _declared
from tests.test_device_cross_filter_abi import DECLARED as ROWS_DECLARED
from tests.test_device_cross_filter_abi import FIELDS as ROWS_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "uint32_t vary",
         "const uint32_t* d_owners", "size_t n_owners", "const uint32_t* d_group_off", "const uint32_t* d_candidates",
         "size_t n_candidates", "const char* const* contexts", "const size_t* context_lens", "size_t n_contexts",
         "int64_t now_us"]
_SEL = ["const gck_select_groups* sel"]
DECLARED = {"gck_filter_groups_device": _HEAD + _SEL + _TAIL + _SYNC,
            "gck_filter_submit_groups_device": _HEAD + _SEL + _TAIL + _SUBMIT}
GROUPS_CTYPES = dict(CTYPES, **{"const gck_select_groups*": (ctypes.POINTER(E.SelectGroups),)})

FIELDS = ["uint32_t mask", "uint32_t group_limit", "uint32_t* d_out_row_off", "uint32_t* d_out_row_n",
          "uint32_t* d_out_ids", "uint32_t* d_out_pos", "uint8_t* d_out_perm", "size_t cap", "uint32_t* d_out_n"]


def test_libraries_export_the_symbols():
    lib = E.load_library()
    for name in list(DECLARED) + ["gck_test_select_groups", "gck_test_group_of", "gck_test_groups_rule"]:
        assert hasattr(lib, name), name
    for name in ("filter_groups_device", "submit_filter_groups_device", "filter_groups_ids"):
        assert callable(getattr(E.Engine, name)), name
    from gochugaru_amd.client import Client
    assert callable(getattr(Client, "FilterGroupsDevice")) and callable(getattr(Client, "FilterGroupSubjectsDevice"))


def test_header_declares_the_argument_lists():
    text = _declarations()
    for name, want in DECLARED.items():
        assert _declared(text, name) == want, name
    # no existing call changed: the cross filter forms', the cross device call's and the list filter's lists
    for name, want in list(ROWS_DECLARED.items()) + list(COLS_DECLARED.items()) + list(CROSS.items()):
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
            assert a in GROUPS_CTYPES[t], (name, p, a)


def test_select_groups_fields_match_the_header():
    text = _declarations()
    m = re.search(r"typedef struct gck_select_groups \{(.*?)\} gck_select_groups;", text, flags=re.S)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == FIELDS
    assert [n for n, _ in E.SelectGroups._fields_] == [f.rsplit(" ", 1)[1] for f in fields]
    # the cross filter forms' structs are unchanged
    for struct, want in (("gck_select_rows", ROWS_FIELDS), ("gck_select_cols", COLS_FIELDS)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S)
        assert [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == want, struct


def test_select_groups_layout_matches_the_c_struct(tmp_path):
    """sizeof and every offsetof of gck_select_groups, from a C program compiled against the header."""
    names = [n for n, _ in E.SelectGroups._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gck.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gck_select_groups));\n'
                   + "".join(f'  printf(" %zu", offsetof(gck_select_groups, {n}));\n' for n in names)
                   + '  printf(" %zu %zu %d", sizeof(gck_select_rows), sizeof(gck_select_cols), GCK_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sys.maxsize > 2 ** 32  # (a 64-bit layout)
    assert got[0] == ctypes.sizeof(E.SelectGroups) == 64
    assert got[1:1 + len(names)] == [getattr(E.SelectGroups, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert got[-3:] == [64, 64, 13]


def test_rule_function_refuses_the_refusal_list():
    """gck_test_groups_rule is the entry points' own rule function (groups_fault) over the same
    arguments; it reads no buffer but the header and the selection, so host memory stands in for the
    device pointers. One good request, then each item of gck.h's refusal list alone."""
    fn = E.load_library().gck_test_groups_rule
    fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    fn.argtypes = [ctypes.POINTER(E.Uniform), ctypes.c_uint32, P, ctypes.c_size_t, P, P, ctypes.c_size_t, ctypes.c_size_t,
                   ctypes.POINTER(E.SelectGroups), P, P, ctypes.c_size_t, P]
    buf = np.zeros(64, dtype=np.uint64)  # 8-byte aligned; + 4 is 4-byte aligned only, + 2 and + 1 neither
    at = buf.ctypes.data

    def hdr(context_slot=0, reserved=0):
        h = E.Uniform()
        h.context_slot, h.reserved = context_slot, reserved
        return h

    def sel(**kw):
        f = dict(mask=E.SELECT_LOOKUP, group_limit=0, d_out_row_off=at, d_out_row_n=at, d_out_ids=at, d_out_pos=at,
                 d_out_perm=at + 1, cap=8, d_out_n=at)
        f.update(kw)
        return E.SelectGroups(*[f[n] for n, _ in E.SelectGroups._fields_])

    def rule(h=None, vary=E.VARY_RESOURCE, owners=at, S=3, off=at, cands=at, n=40, n_contexts=0, s="good", packed=at,
             errs=at, err_cap=4, n_errs=at):
        s = sel() if s == "good" else s
        return fn(ctypes.byref(h or hdr()), vary, owners, S, off, cands, n, n_contexts,
                  ctypes.byref(s) if s is not None else None, packed, errs, err_cap, n_errs)

    assert rule() == 0
    assert rule(vary=E.VARY_SUBJECT) == 0
    assert rule(S=0, n=0, owners=None, off=None, cands=None) == 0       # the empty request
    assert rule(n=0, owners=None, off=None, cands=None) == 0            # n == 0 with S > 0: no input is read
    assert rule(s=sel(cap=0, d_out_ids=None, d_out_pos=None, d_out_perm=None)) == 0  # cap == 0 needs no record array
    assert rule(s=sel(d_out_row_n=None), errs=None, err_cap=0, n_errs=None) == 0
    assert rule(hdr(context_slot=2), n_contexts=2) == 0

    assert rule(s=None) == -1                                           # sel == NULL
    for mask in (0, 1, 3, 0xF, 0x10, 0x12):                             # a bad mask
        assert rule(s=sel(mask=mask)) == -1, mask
    assert rule(hdr(reserved=1)) == -1                                  # reserved in the header
    for vary in (0, 3, 4):                                              # a bad vary
        assert rule(vary=vary) == -1, vary
    assert rule(s=sel(d_out_row_off=None)) == -1                        # d_out_row_off, d_out_n or d_out_packed NULL
    assert rule(s=sel(d_out_n=None)) == -1
    assert rule(packed=None) == -1
    assert rule(s=sel(d_out_ids=None, d_out_pos=None, d_out_perm=None)) == -1  # cap > 0, all three record arrays NULL
    assert rule(n=2 ** 32) == -1 and rule(n=2 ** 32 - 1) == 0           # n >= 2^32 or S >= 2^32
    assert rule(S=2 ** 32) == -1 and rule(S=2 ** 32 - 1) == 0
    assert rule(S=0) == -1                                              # n > 0 with S == 0
    for null in ("owners", "off", "cands"):                             # a null input with n > 0
        assert rule(**{null: None}) == -1, null
    assert rule(packed=at + 4) == -1                                    # d_out_packed not 8-byte aligned
    for name in ("owners", "off", "cands", "errs", "n_errs"):           # any other device pointer not 4-byte aligned
        assert rule(**{name: at + 2}) == -1 and rule(**{name: at + 4}) == 0, name
    for name in ("d_out_row_off", "d_out_row_n", "d_out_ids", "d_out_pos", "d_out_n"):
        assert rule(s=sel(**{name: at + 1})) == -1 and rule(s=sel(**{name: at + 4})) == 0, name
    assert rule(hdr(context_slot=1)) == -1                              # a context slot beyond n_contexts
    assert rule(hdr(context_slot=3), n_contexts=2) == -1
    assert rule(errs=None) == -1                                        # err_cap > 0 without a list (the compact calls' rule)

