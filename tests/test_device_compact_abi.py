"""Compact requests over device buffers without a GPU (include/gck.h gck_check_bulk_uniform_device
...): libgck.so and the driver export the new entry points, gck.h declares them with the argument
lists of the ABI, the Python mirror agrees, and the ABI version stays."""
import ctypes
import os
import re

from gochugaru_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CALL = ["const char* const* contexts", "const size_t* context_lens", "size_t n_contexts", "int64_t now_us"]
_OUT = ["uint64_t* d_out_packed", "gck_item_error* d_out_errs", "size_t err_cap", "uint32_t* d_out_n_errs"]
_SYNC = ["void* stream", "uint64_t* out_revision"]
_SUBMIT = ["uint32_t flags", "void* stream", "gck_batch** out"]
_HEAD = {
    "uniform": ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "const uint32_t* d_pairs",
                "size_t n"],
    "shaped": ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* shapes", "size_t n_shapes",
               "const uint8_t* d_shape_of", "const uint32_t* d_pairs", "size_t n"],
    "list": ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "uint32_t fixed_id",
             "uint32_t vary", "const uint32_t* d_ids", "uint32_t first_id", "size_t n"],
}
DECLARED = {f"gck_check_bulk_{k}_device": h + _CALL + _OUT + _SYNC for k, h in _HEAD.items()}
DECLARED.update({f"gck_check_submit_{k}_device": h + _CALL + _OUT + _SUBMIT for k, h in _HEAD.items()})
DECLARED["gck_device_compact_stats"] = ["gck_engine* e", "uint64_t out[2]"]

# C parameter types -> what the ctypes mirror declares (device and host addresses alike: void pointers)
CTYPES = {"gck_engine*": (ctypes.c_void_p,), "const gck_consistency*": (ctypes.POINTER(E._Consistency),),
          "const gck_uniform*": (ctypes.POINTER(E.Uniform), ctypes.c_void_p), "uint32_t": (ctypes.c_uint32,),
          "const uint32_t*": (ctypes.c_void_p,), "const uint8_t*": (ctypes.c_void_p,), "uint32_t*": (ctypes.c_void_p,),
          "size_t": (ctypes.c_size_t,), "const char* const*": (ctypes.POINTER(ctypes.c_char_p),),
          "const size_t*": (ctypes.POINTER(ctypes.c_size_t),), "int64_t": (ctypes.c_int64,),
          "uint64_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), "gck_item_error*": (ctypes.c_void_p,),
          "void*": (ctypes.c_void_p,), "gck_batch**": (ctypes.POINTER(ctypes.c_void_p),)}


def _declarations():
    with open(os.path.join(ROOT, "include", "gck.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_libraries_export_the_device_compact_symbols():
    lib = E.load_library()
    for name in DECLARED:
        assert hasattr(lib, name), name
    drv = ctypes.CDLL(os.path.join(os.path.dirname(E.__file__), "libgck_driver.so"))
    for name in ("gckd_run_uniform_device", "gckd_run_list_device"):
        assert hasattr(drv, name), name
    for name in ("check_uniform_device", "check_shaped_device", "check_list_device", "submit_uniform_device",
                 "submit_shaped_device", "submit_list_device", "prepare_uniform_device", "prepare_list_device",
                 "device_compact_stats"):
        assert callable(getattr(E.Engine, name)), name


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
            t, ident = p.rsplit(" ", 1)
            t = t + "*" if ident.endswith("]") else t
            assert a in CTYPES[t], (name, p, a)
