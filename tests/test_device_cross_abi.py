"""Cross requests over device buffers without a GPU (include/gck.h gck_check_bulk_cross_device): the
libraries export the entry points, gck.h declares them with the ABI's argument lists, the Python
mirror agrees, the ABI version stays, the device tiling rule equals its restatement, and
cross_id_block lays the two lists out as the joins read an id block."""
import ctypes
import os
import re

import pytest
import torch

from gochugaru_amd import engine as E
from gochugaru_amd.client import Client

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = ["gck_engine* e", "const gck_consistency* cs", "const gck_uniform* hdr", "const uint32_t* d_subjects",
         "size_t n_subjects", "const uint32_t* d_resources", "size_t n_resources", "const char* const* contexts",
         "const size_t* context_lens", "size_t n_contexts", "int64_t now_us", "uint64_t* d_out_packed",
         "gck_item_error* d_out_errs", "size_t err_cap", "uint32_t* d_out_n_errs"]
DECLARED = {
    "gck_check_bulk_cross_device": _HEAD + ["void* stream", "uint64_t* out_revision"],
    "gck_check_submit_cross_device": _HEAD + ["uint32_t flags", "void* stream", "gck_batch** out"],
    "gck_cross_tile_device": ["size_t n_subjects", "size_t n_resources", "size_t max_batch", "uint32_t* rows"],
}
CTYPES = {"gck_engine*": (ctypes.c_void_p,), "const gck_consistency*": (ctypes.POINTER(E._Consistency),),
          "const gck_uniform*": (ctypes.POINTER(E.Uniform),), "uint32_t": (ctypes.c_uint32,),
          "const uint32_t*": (ctypes.c_void_p,), "uint32_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)),
          "size_t": (ctypes.c_size_t,), "const char* const*": (ctypes.POINTER(ctypes.c_char_p),),
          "const size_t*": (ctypes.POINTER(ctypes.c_size_t),), "int64_t": (ctypes.c_int64,),
          "uint64_t*": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)), "gck_item_error*": (ctypes.c_void_p,),
          "void*": (ctypes.c_void_p,), "gck_batch**": (ctypes.POINTER(ctypes.c_void_p),)}
CROSS_IDS = 2048


def _declarations():
    with open(os.path.join(ROOT, "include", "gck.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_libraries_export_the_cross_device_symbols():
    lib = E.load_library()
    for name in DECLARED:
        assert hasattr(lib, name), name
    drv = ctypes.CDLL(os.path.join(os.path.dirname(E.__file__), "libgck_driver.so"))
    assert hasattr(drv, "gckd_run_cross_device")
    for name in ("check_cross_device", "submit_cross_device", "prepare_cross_device", "check_cross_ids"):
        assert callable(getattr(E.Engine, name)), name
    assert callable(E.cross_tile_device) and callable(E.cross_id_block)
    assert callable(Client.CheckCrossDevice)


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
            assert a in CTYPES[p.rsplit(" ", 1)[0]], (name, p, a)


def _rule(S, R, mb):
    """The device tiling rule restated: full-width tiles, the host rule's thin condition."""
    if R == 0 or R >= CROSS_IDS:
        return 0
    row = 32 * ((R + 31) // 32)
    if row > mb:
        return 0
    rows = min(S, mb // row, CROSS_IDS - R)
    if rows == 0:
        return 0
    if S * R > rows * R and rows * R < mb // 4:
        return 0
    return rows


SIZES = [0, 1, 31, 32, 33, 65, 2015, 2016, 2047, 2048, 3000]


@pytest.mark.parametrize("max_batch", [32, 64, 256, 65536])
def test_tiling_rule_matches_its_restatement(max_batch):
    lib = E.load_library()
    for S in SIZES:
        for R in SIZES:
            rows = ctypes.c_uint32(77)
            ok = lib.gck_cross_tile_device(S, R, max_batch, ctypes.byref(rows))
            want = _rule(S, R, max_batch)
            assert (ok, rows.value) == (1 if want else 0, want), (S, R, max_batch)
            assert E.cross_tile_device(S, R, max_batch) == want
            if want:  # what the engine relies on: the padded tile fits a batch, its ids fit the block
                assert want * 32 * ((R + 31) // 32) <= max_batch and E.cross_sub_off(R) + want <= CROSS_IDS + 3
    assert lib.gck_cross_tile_device(5, 5, 65536, None) == 1  # (rows may be NULL)


def test_tiling_rule_spot_values():
    assert E.cross_tile_device(256, 256, 65536) == 256
    assert E.cross_tile_device(32, 2016, 65536) == 32       # 32 x 2,016: one tile, the id block full
    assert E.cross_tile_device(10, 100, 256) == 2           # five bands, the last one ragged
    assert E.cross_tile_device(1, 3000, 65536) == 0         # wider than the id block: expanded
    assert E.cross_tile_device(60, 3, 64) == 0              # thin: thirty 2 x 3 tiles
    assert E.cross_tile_device(1, 500, 64) == 0             # a row's 512 padded checks exceed max_batch
    # the host rule is untouched
    assert E.cross_tile(10, 100, 256) == (4, 64) and E.cross_tile(1, 500, 64) == (1, 64)


@pytest.mark.parametrize("S,R", [(1, 1), (3, 4), (5, 31), (2, 33), (7, 65), (32, 2016), (0, 5), (4, 0)])
def test_cross_id_block_layout(S, R):
    sub = torch.arange(1000, 1000 + S, dtype=torch.int32)
    res = torch.arange(1, 1 + R, dtype=torch.int32)
    block, sv, rv = E.cross_id_block(sub, res)
    off = E.cross_sub_off(R)
    assert off == (R + 3) // 4 * 4 and block.numel() == off + S and block.dtype == torch.int32
    assert torch.equal(rv, res) and torch.equal(sv, sub)
    assert not block[R:off].any()
    # the views lie in the block, the subjects at word cross_sub_off(R): the layout read in place
    # (an empty view has no address)
    if R:
        assert rv.data_ptr() == block.data_ptr()
    if S:
        assert sv.data_ptr() == block.data_ptr() + 4 * off
