"""Recheck requests without a GPU (include/gck.h gck_recheck_list_device, gck_recheck_cross_device and
the plane-only calls): libgck.so exports the entry points and the test hooks, gck.h declares them with
the argument lists of the ABI — the list and cross device calls', with `d_prev_packed` and `sel`
between now_us and d_out_packed — the Python mirror agrees, the two structs' layouts (48 and 56 bytes)
included, the constants have their values, the rule hooks refuse what the entry points' rule functions
refuse — every item of the header's refusal list —, the list and cross device calls' declarations are
as they were, and the ABI version stays."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

from gochugaru_amd import engine as E
from tests.test_device_cross_filter_abi import _SUBMIT, _SYNC, _TAIL, CROSS, CTYPES, _declarations, _declared
from tests.test_device_cross_filter_abi import _HEAD as CROSS_HEAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIST_HEAD = ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "uint32_t fixed_id", "uint32_t vary",
             "const uint32_t* d_ids", "uint32_t first_id", "size_t n", "const char* const* contexts",
             "const size_t* context_lens", "size_t n_contexts", "int64_t now_us"]
_PREV = ["const uint64_t* d_prev_packed"]
_DSEL, _RSEL = ["const gck_select_changes* sel"], ["const gck_select_row_changes* sel"]
DECLARED = {
    "gck_recheck_list_device": LIST_HEAD + _PREV + _DSEL + _TAIL + _SYNC,
    "gck_recheck_submit_list_device": LIST_HEAD + _PREV + _DSEL + _TAIL + _SUBMIT,
    "gck_recheck_cross_device": CROSS_HEAD + _PREV + _RSEL + _TAIL + _SYNC,
    "gck_recheck_submit_cross_device": CROSS_HEAD + _PREV + _RSEL + _TAIL + _SUBMIT,
    "gck_diff_planes_device": ["gck_engine* e", "const uint64_t* d_old", "const uint64_t* d_new", "size_t n",
                               "const uint32_t* d_ids", "uint32_t first_id", "const gck_select_changes* sel", "void* stream"],
    "gck_diff_cross_planes_device": ["gck_engine* e", "const uint64_t* d_old", "const uint64_t* d_new", "size_t n_subjects",
                                     "size_t n_resources", "const uint32_t* d_resources",
                                     "const gck_select_row_changes* sel", "void* stream"],
}
LIST = {"gck_check_bulk_list_device": LIST_HEAD + _TAIL + _SYNC, "gck_check_submit_list_device": LIST_HEAD + _TAIL + _SUBMIT}
RECHECK_CTYPES = dict(CTYPES, **{"const gck_select_changes*": (ctypes.POINTER(E.SelectChanges),),
                                 "const gck_select_row_changes*": (ctypes.POINTER(E.SelectRowChanges),),
                                 "const uint64_t*": (ctypes.c_void_p,)})

FIELDS = {"gck_select_changes": ["uint32_t transitions", "uint32_t reserved", "uint32_t* d_out_ids", "uint32_t* d_out_pos",
                                 "uint8_t* d_out_trans", "size_t cap", "uint32_t* d_out_n"],
          "gck_select_row_changes": ["uint32_t transitions", "uint32_t reserved", "uint32_t* d_out_row_off",
                                     "uint32_t* d_out_ids", "uint32_t* d_out_col", "uint8_t* d_out_trans", "size_t cap",
                                     "uint32_t* d_out_n"]}
MIRROR = {"gck_select_changes": E.SelectChanges, "gck_select_row_changes": E.SelectRowChanges}
HOOKS = ["gck_test_change_plane", "gck_test_change_rows", "gck_test_changes_rule", "gck_test_row_changes_rule"]


def test_libraries_export_the_symbols():
    lib = E.load_library()
    for name in list(DECLARED) + HOOKS:
        assert hasattr(lib, name), name
    for name in ("diff_planes_device", "diff_cross_planes_device", "recheck_list_device", "recheck_cross_device",
                 "submit_recheck_list_device", "submit_recheck_cross_device", "recheck_ids", "recheck_cross_ids"):
        assert callable(getattr(E.Engine, name)), name
    from gochugaru_amd.client import Client
    for name in ("RecheckResourcesDevice", "RecheckSubjectsDevice", "RecheckCrossDevice"):
        assert callable(getattr(Client, name)), name


def test_header_declares_the_argument_lists():
    text = _declarations()
    for name, want in DECLARED.items():
        assert _declared(text, name) == want, name
    # no existing call changed: the list and cross device calls' lists
    for name, want in list(LIST.items()) + list(CROSS.items()):
        assert _declared(text, name) == want, name
    assert re.search(r"#define GCK_ABI_VERSION 13\b", text)  # additive: the ABI version stays
    assert E.load_library().gck_abi_version() == 13


def test_python_mirror_matches_the_declarations():
    for name, params in DECLARED.items():
        restype, argtypes = E._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, a in zip(params, argtypes):
            t, _ = p.rsplit(" ", 1)
            assert a in RECHECK_CTYPES[t], (name, p, a)


def test_struct_fields_match_the_header():
    text = _declarations()
    for struct, want in FIELDS.items():
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S)
        assert m, struct
        fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
        assert fields == want, struct
        assert [n for n, _ in MIRROR[struct]._fields_] == [f.rsplit(" ", 1)[1] for f in fields], struct


def test_struct_layouts_and_constants_match_the_c_header(tmp_path):
    """sizeof and every offsetof of the two structs and the three constants, from a C program compiled
    against the header."""
    src = tmp_path / "layout.c"
    body = ""
    for struct, cls in MIRROR.items():
        body += f'  printf("%zu", sizeof({struct}));\n'
        body += "".join(f'  printf(" %zu", offsetof({struct}, {n}));\n' for n, _ in cls._fields_)
        body += '  printf("\\n");\n'
    body += '  printf("%u %u %u %d\\n", GCK_CHANGE_GAINED, GCK_CHANGE_LOST, GCK_CHANGE_ANY, GCK_ABI_VERSION);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gck.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = [[int(x) for x in line.split()]
             for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert sys.maxsize > 2 ** 32  # (a 64-bit layout)
    assert lines[0][0] == ctypes.sizeof(E.SelectChanges) == 48
    assert lines[0][1:] == [getattr(E.SelectChanges, n).offset for n, _ in E.SelectChanges._fields_] == [0, 4, 8, 16, 24, 32, 40]
    assert lines[1][0] == ctypes.sizeof(E.SelectRowChanges) == 56
    assert lines[1][1:] == [getattr(E.SelectRowChanges, n).offset for n, _ in E.SelectRowChanges._fields_] \
        == [0, 4, 8, 16, 24, 32, 40, 48]
    assert lines[2] == [E.CHANGE_GAINED, E.CHANGE_LOST, E.CHANGE_ANY, 13] == [0x00CC, 0x3300, 0x7BDE, 13]


def test_constants_are_the_transition_sets():
    bit = lambda v, w: 1 << (4 * v + w)
    assert E.CHANGE_GAINED == sum(bit(v, w) for v in (0, 1) for w in (2, 3))
    assert E.CHANGE_LOST == sum(bit(v, w) for v in (2, 3) for w in (0, 1))
    assert E.CHANGE_ANY == sum(bit(v, w) for v in range(4) for w in range(4) if v != w)
    assert E.change_split(4 * E.PERM_NO + E.PERM_HAS) == (E.PERM_NO, E.PERM_HAS)
    old, new = E.change_split(np.array([4 * 3 + 0, 4 * 0 + 2], dtype=np.uint8))
    assert old.tolist() == [3, 0] and new.tolist() == [0, 2]


def _buffers():
    buf = np.zeros(256, dtype=np.uint64)  # 8-byte aligned; + 4 is 4-byte aligned only, + 2 and + 1 neither
    return buf, buf.ctypes.data


def test_dense_rule_refuses_the_refusal_list():
    """gck_test_changes_rule is the list form's rule function (changes_fault: both entry points and the
    plane-only call go through it) over the same arguments; it reads no buffer but the struct, so host
    memory stands in for the device pointers. One good request, then each refusal alone."""
    fn = E.load_library().gck_test_changes_rule
    fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    fn.argtypes = [ctypes.POINTER(E.SelectChanges), P, P, ctypes.c_size_t, ctypes.c_int]
    buf, at = _buffers()
    n, words = 100, 4
    prev, out, rec = at, at + 8 * words, at + 1024

    def sel(**kw):
        f = dict(transitions=E.CHANGE_ANY, reserved=0, d_out_ids=rec, d_out_pos=rec, d_out_trans=rec + 1, cap=8, d_out_n=rec)
        f.update(kw)
        return E.SelectChanges(*[f[k] for k, _ in E.SelectChanges._fields_])

    def rule(s="good", prev=prev, out=out, n=n, need=1):
        s = sel() if s == "good" else s
        return fn(ctypes.byref(s) if s is not None else None, prev, out, n, need)

    assert rule() == 0
    assert rule(prev=None) == 0                                          # a null previous plane: all zeros
    assert rule(s=sel(cap=0, d_out_ids=None, d_out_pos=None, d_out_trans=None)) == 0
    for tr in (E.CHANGE_GAINED, E.CHANGE_LOST, 1 << 1, 1 << 14):
        assert rule(s=sel(transitions=tr)) == 0, tr
    assert rule(n=0, prev=at, out=at) == 0                               # no words: nothing to overlap
    assert rule(out=None, n=0, need=0) == 0                              # a plane-only call without checks

    assert rule(s=None) == -1                                            # a null struct
    for tr in (0, 1, 1 << 5, 1 << 10, 1 << 15, 0x8000, 0x10000, E.CHANGE_ANY | 0x10000):  # bad transitions
        assert rule(s=sel(transitions=tr)) == -1, tr
    assert rule(s=sel(reserved=1)) == -1                                 # reserved != 0
    assert rule(s=sel(d_out_n=None)) == -1                               # a missing required pointer
    assert rule(out=None) == -1
    assert rule(s=sel(d_out_ids=None, d_out_pos=None, d_out_trans=None)) == -1  # cap > 0, every record array NULL
    assert rule(prev=prev + 4, out=out + 64) == -1 and rule(out=out + 4) == -1  # the planes: 8 bytes
    for name in ("d_out_ids", "d_out_pos", "d_out_n"):                   # everything else: 4 bytes
        assert rule(s=sel(**{name: rec + 2})) == -1 and rule(s=sel(**{name: rec + 4})) == 0, name
    # a d_prev_packed range that overlaps d_out_packed's: the same, either way round by one word, inside
    for p, o in ((at, at), (at, at + 8 * (words - 1)), (at + 8 * (words - 1), at), (at + 8, at)):
        assert rule(prev=p, out=o) == -1, (p - at, o - at)
    assert rule(prev=at, out=at + 8 * words) == 0 and rule(prev=at + 8 * words, out=at) == 0  # adjacent


def test_row_rule_refuses_the_refusal_list():
    """gck_test_row_changes_rule, likewise for the cross form (row_changes_fault)."""
    fn = E.load_library().gck_test_row_changes_rule
    fn.restype = ctypes.c_int
    P = ctypes.c_void_p
    fn.argtypes = [ctypes.POINTER(E.SelectRowChanges), P, P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    buf, at = _buffers()
    S, R, words = 5, 40, 10
    prev, out, rec = at, at + 8 * words, at + 1024

    def sel(**kw):
        f = dict(transitions=E.CHANGE_ANY, reserved=0, d_out_row_off=rec, d_out_ids=rec, d_out_col=rec, d_out_trans=rec + 1,
                 cap=8, d_out_n=rec)
        f.update(kw)
        return E.SelectRowChanges(*[f[k] for k, _ in E.SelectRowChanges._fields_])

    def rule(s="good", prev=prev, out=out, S=S, R=R, need=1):
        s = sel() if s == "good" else s
        return fn(ctypes.byref(s) if s is not None else None, prev, out, S, R, need)

    assert rule() == 0
    assert rule(prev=None) == 0
    assert rule(s=sel(cap=0, d_out_ids=None, d_out_col=None, d_out_trans=None)) == 0
    assert rule(S=0, prev=at, out=at) == 0 and rule(R=0, prev=at, out=at) == 0  # no words: nothing to overlap
    assert rule(out=None, S=0, need=0) == 0

    assert rule(s=None) == -1
    for tr in (0, 1, 1 << 5, 1 << 10, 1 << 15, 0x8000, 0x10000):
        assert rule(s=sel(transitions=tr)) == -1, tr
    assert rule(s=sel(reserved=7)) == -1
    assert rule(s=sel(d_out_row_off=None)) == -1
    assert rule(s=sel(d_out_n=None)) == -1
    assert rule(out=None) == -1
    assert rule(s=sel(d_out_ids=None, d_out_col=None, d_out_trans=None)) == -1
    assert rule(prev=prev + 4, out=out + 160) == -1 and rule(out=out + 4) == -1
    for name in ("d_out_row_off", "d_out_ids", "d_out_col", "d_out_n"):
        assert rule(s=sel(**{name: rec + 1})) == -1 and rule(s=sel(**{name: rec + 4})) == 0, name
    for p, o in ((at, at), (at, at + 8 * (words - 1)), (at + 8 * (words - 1), at), (at + 16, at)):
        assert rule(prev=p, out=o) == -1, (p - at, o - at)
    assert rule(prev=at, out=at + 8 * words) == 0 and rule(prev=at + 8 * words, out=at) == 0
