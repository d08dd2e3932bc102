"""List requests without a GPU (include/gck.h gck_check_bulk_list): the libraries export the new
entry points with the declared signatures, the constants of gck.h and engine.py agree, and the
request errors are reported on the host before anything else."""
import ctypes
import os
import re

import numpy as np
import pytest

from gochugaru_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gck_check_bulk_list", "gck_check_submit_list", "gck_list_stats", "gck_lookup_resources_among",
       "gck_lookup_subjects_among")
# C parameter types -> the ctypes the Python mirror must declare
CTYPES = {"gck_engine*": ctypes.c_void_p, "const gck_consistency*": ctypes.POINTER(E._Consistency),
          "const gck_uniform*": ctypes.POINTER(E.Uniform), "uint32_t": ctypes.c_uint32, "uint16_t": ctypes.c_uint16,
          "const uint32_t*": ctypes.c_void_p, "uint32_t*": ctypes.c_void_p, "uint8_t*": ctypes.c_void_p,
          "size_t": ctypes.c_size_t, "const char* const*": ctypes.POINTER(ctypes.c_char_p),
          "const size_t*": ctypes.POINTER(ctypes.c_size_t), "int64_t": ctypes.c_int64, "uint64_t*": None,
          "gck_item_error*": ctypes.c_void_p, "size_t*": ctypes.POINTER(ctypes.c_size_t),
          "gck_batch**": ctypes.POINTER(ctypes.c_void_p), "uint64_t": ctypes.c_uint64}


def _header_text():
    with open(os.path.join(ROOT, "include", "gck.h")) as f:
        return f.read()


@pytest.fixture()
def eng():
    e = E.Engine(device=0)
    yield e
    e.close()


def test_libraries_export_the_list_symbols():
    lib = E.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    path = os.path.join(os.path.dirname(E.__file__), "libgck_driver.so")
    assert hasattr(ctypes.CDLL(path), "gckd_run_list")
    for name in ("check_list", "submit_list", "prepare_list", "list_stats", "lookup_resources_among",
                 "lookup_subjects_among"):
        assert callable(getattr(E.Engine, name)), name


def test_constants_agree_with_the_header():
    text = _header_text()
    for name, value in (("GCK_VARY_RESOURCE", E.VARY_RESOURCE), ("GCK_VARY_SUBJECT", E.VARY_SUBJECT),
                        ("GCK_ID_ABSENT", E.ID_ABSENT), ("GCK_ID_WILDCARD", E.ID_WILDCARD)):
        m = re.search(r"#define %s (\w+)" % name, text)
        assert m and int(m.group(1).rstrip("uU"), 0) == value, name
    assert E.VARY_RESOURCE != E.VARY_SUBJECT and 0 not in (E.VARY_RESOURCE, E.VARY_SUBJECT)
    assert re.search(r"#define GCK_ABI_VERSION 13\b", text)  # additive: the ABI version stays


def test_declared_signatures_match_the_python_mirror():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint %s\((.*?)\);" % name, text, flags=re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        # "type name" / "type name[2]" -> type
        types = []
        for p in params:
            t, ident = p.rsplit(" ", 1)
            types.append(t + "*" if ident.endswith("]") else t)
        restype, argtypes = E._SIGS[name]
        assert restype is ctypes.c_int and len(argtypes) == len(types), (name, types)
        for t, a in zip(types, argtypes):
            assert t in CTYPES, (name, t)
            want = CTYPES[t]
            if want is None:  # uint64_t*: an output array (void pointer) or one revision (typed pointer)
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), (name, t, a)
            else:
                assert a is want or (want is ctypes.c_void_p and a is ctypes.c_void_p), (name, t, a)


def test_list_entry_points_report_request_errors_without_a_snapshot(eng):
    plain = (0, 0, 0, E.ELLIPSIS)
    ids = np.arange(4, dtype=np.uint32)
    words = np.zeros(4, dtype=np.uint64)
    errs = np.zeros(16, dtype=E.ITEM_ERROR_DTYPE)
    lib = eng._lib
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    n_errs = ctypes.c_size_t(0)
    rev = ctypes.c_uint64(0)

    def bulk(hdr, vary, p, first, n, out, n_ctx=0, err_cap=len(errs), err_p=errs.ctypes.data):
        return lib.gck_check_bulk_list(eng._h, ctypes.byref(cs), ctypes.byref(hdr), 0, vary, p, first, n, None, None,
                                       n_ctx, 0, out, err_p, err_cap, ctypes.byref(n_errs), ctypes.byref(rev))

    def submit(hdr, vary, p, first, n, out, n_ctx=0, err_cap=len(errs), err_p=errs.ctypes.data):
        h = ctypes.c_void_p()
        rc = lib.gck_check_submit_list(eng._h, ctypes.byref(cs), ctypes.byref(hdr), 0, vary, p, first, n, None, None,
                                       n_ctx, 0, out, err_p, err_cap, ctypes.byref(n_errs), ctypes.byref(h))
        assert h.value is None
        return rc

    ok = E.Uniform(*plain, 0, 0)
    p, w = ids.ctypes.data, words.ctypes.data
    R, S = E.VARY_RESOURCE, E.VARY_SUBJECT
    bad = E.GCK_E_INVALID_ARGUMENT
    for call in (bulk, submit):
        for vary in (0, 3, 4, 0xFFFFFFFF):                          # a side flag that is neither value
            assert call(ok, vary, p, 0, 4, w) == bad
        assert call(E.Uniform(*plain, 0, 7), R, p, 0, 4, w) == bad    # reserved != 0
        assert call(E.Uniform(*plain, 1, 0), R, p, 0, 4, w) == bad    # a context slot above n_contexts
        assert call(ok, R, None, 0xFFFFFFFF, 2, w) == bad             # first_id + n > 2^32
        assert call(ok, R, None, 2, 0xFFFFFFFF, w) == bad
        assert call(ok, S, None, 0, 4, w) == bad                      # a range varies the resource id
        assert call(ok, R, p, 0, 4, None) == bad                      # null outputs with n > 0
        assert call(ok, S, p, 0, 4, None) == bad
        assert call(ok, R, p, 0, 4, w, err_cap=4, err_p=None) == bad  # an error list without a buffer
    assert submit(ok, R, p, 0, 4, w) != bad and bulk(ok, R, None, 0xFFFFFFFC, 4, w) != bad  # (valid: fails later, below)
    # the Python methods raise the same
    with pytest.raises(E.GckError) as ei:
        eng.check_list(plain, 0, 5, ids)
    assert ei.value.code == bad
    with pytest.raises(E.GckError) as ei:
        eng.check_list((0, 0, 0, E.ELLIPSIS, 2), 0, R, ids, contexts=[{"a": 1}])
    assert ei.value.code == bad
    with pytest.raises(ValueError):
        eng.check_list(plain, 0, R)  # a range needs n
    # a valid request needs a snapshot like any check, an empty one included
    eng.load_schema("definition user {}")
    for args in ((ids,), (ids[:0],), (None, 0, 4), (None, 9, 0)):
        with pytest.raises(E.GckError) as ei:
            eng.check_list(plain, 0, R, *args)
        assert ei.value.code == E.GCK_E_STATE
    assert eng.list_stats() == (0, 0)
    out = (ctypes.c_uint64 * 2)()
    assert lib.gck_list_stats(eng._h, None) == bad and lib.gck_list_stats(eng._h, out) == 0


def test_lookups_among_report_request_errors_without_a_snapshot(eng):
    lib = eng._lib
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    n = ctypes.c_size_t(0)
    ids = np.arange(4, dtype=np.uint32)
    out_ids, out_perm = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    bad = E.GCK_E_INVALID_ARGUMENT
    res = lambda *tail: lib.gck_lookup_resources_among(eng._h, ctypes.byref(cs), 0, 0, 0, E.ELLIPSIS, *tail)
    sub = lambda *tail: lib.gck_lookup_subjects_among(eng._h, ctypes.byref(cs), 0, 0, 0, 0, E.ELLIPSIS, *tail)
    # a wildcard subject cannot be looked up (gck_lookup_resources' rule)
    assert res(E.ID_WILDCARD, ids.ctypes.data, 4, 1, out_ids.ctypes.data, out_perm.ctypes.data, 4, ctypes.byref(n)) == bad
    # null outputs
    assert res(0, ids.ctypes.data, 4, 1, out_ids.ctypes.data, out_perm.ctypes.data, 4, None) == bad
    assert res(0, ids.ctypes.data, 4, 1, None, out_perm.ctypes.data, 4, ctypes.byref(n)) == bad
    assert sub(ids.ctypes.data, 4, 1, out_ids.ctypes.data, None, 4, ctypes.byref(n)) == bad
    # the subjects need a candidate list
    assert sub(None, 4, 1, out_ids.ctypes.data, out_perm.ctypes.data, 4, ctypes.byref(n)) == bad
    # valid requests need a snapshot
    assert res(0, None, 0, 1, out_ids.ctypes.data, out_perm.ctypes.data, 4, ctypes.byref(n)) == E.GCK_E_STATE
    assert sub(ids.ctypes.data, 4, 1, out_ids.ctypes.data, out_perm.ctypes.data, 4, ctypes.byref(n)) == E.GCK_E_STATE
    # an empty candidate list asks nothing
    got, perms = eng.lookup_subjects_among(0, 0, 0, 0, np.zeros(0, dtype=np.uint32))
    assert len(got) == 0 and len(perms) == 0
