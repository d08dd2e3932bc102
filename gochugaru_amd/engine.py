"""ctypes binding of ``libgck.so`` (the C ABI in ``include/gck.h``).

This is the host-side plumbing a Python caller uses; a Go caller binds the same symbols with
cgo. The shared library is built in-tree by ``__graft_entry__.build()``
(``make -C gochugaru_amd/csrc``). There is deliberately **no fallback**: if the library or a
HIP device is missing, the calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time
import weakref
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

# GCK_LIBRARY: an instrumented build of the same sources (make TIMING=1 -> libgck_timing.so)
_LIB_PATH = os.environ.get("GCK_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgck.so")

# ---- constants mirrored from include/gck.h ------------------------------------------------
GCK_OK = 0
GCK_E_INVALID_ARGUMENT = -1
GCK_E_SCHEMA = -2
GCK_E_NOT_FOUND = -3
GCK_E_DEVICE = -4
GCK_E_CAPACITY = -5
GCK_E_STATE = -6
GCK_E_REVISION = -7
GCK_E_NO_DEVICE = -8
GCK_E_REVISION_GONE = -9

PERM_UNSPECIFIED, PERM_NO, PERM_HAS, PERM_CONDITIONAL = 0, 1, 2, 3

ITEM_OK = 0
ITEM_ERR_MAX_DEPTH = 1
ITEM_ERR_UNKNOWN_PERMISSION = 2
ITEM_ERR_UNKNOWN_TYPE = 3
ITEM_ERR_UNKNOWN_SUBJECT_RELATION = 4
ITEM_ERR_WILDCARD_SUBJECT = 5
ITEM_ERR_CAVEAT_EVAL = 6

ELLIPSIS = 0xFFFF
ID_WILDCARD = 0xFFFFFFFF
ID_ABSENT = 0xFFFFFFFE
TYPE_INVALID = 0xFFFF
REL_INVALID = 0xFFFE  # an id no schema relation has (never equal to ELLIPSIS)

CONSISTENCY_MIN_LATENCY, CONSISTENCY_FULL, CONSISTENCY_AT_LEAST, CONSISTENCY_SNAPSHOT = 0, 1, 2, 3
CAVEAT_FALSE, CAVEAT_TRUE, CAVEAT_PARTIAL = 0, 1, 2
INTERN_CREATE = 1
MEM_DEVICE = 1
FLAG_PROFILE = 1
FLAG_NO_BUNDLE = 2
FLAG_NO_MHASH = 4
FLAG_NO_GIANT = 8
FLAG_NO_BIDIR = 16
FLAG_NO_CLOSURE = 32
FLAG_LAZY_CAVEATS = 64
FLAG_NO_SLOTS = 128
FLAG_NO_LABELS = 256
FLAG_RESIDENT = 512
FLAG_BIG_MHASH = 1024
SUBMIT_DEVICE = 1
SUBMIT_ENGINE_STREAM = 2

ITEM_DTYPE = np.dtype([
    ("resource_type", "<u2"), ("permission", "<u2"), ("resource_id", "<u4"),
    ("subject_type", "<u2"), ("subject_relation", "<u2"), ("subject_id", "<u4"),
    ("context_slot", "<u4"),
])
assert ITEM_DTYPE.itemsize == 20

TUPLE_DTYPE = np.dtype({
    "names": ["resource_type", "relation", "resource_id", "subject_type", "subject_relation",
              "subject_id", "caveat", "expires_at_us"],
    "formats": ["<u2", "<u2", "<u4", "<u2", "<u2", "<u4", "<u4", "<i8"],
    "offsets": [0, 2, 4, 8, 10, 12, 16, 24],
    "itemsize": 32,
})

UPDATE_CREATE, UPDATE_DELETE, UPDATE_TOUCH = 1, 2, 3  # rel.UpdateType (rel/relationship.go:267-274)
UPDATE_DTYPE = np.dtype({"names": ["op", "reserved", "tuple"], "formats": ["<u4", "<u4", TUPLE_DTYPE],
                         "offsets": [0, 4, 8], "itemsize": 40})

ITEM_ERROR_MESSAGES = {
    ITEM_ERR_MAX_DEPTH: "max depth exceeded: this usually indicates a recursive or too deep data dependency",
    ITEM_ERR_UNKNOWN_PERMISSION: "relation/permission not found",
    ITEM_ERR_UNKNOWN_TYPE: "object definition not found",
    ITEM_ERR_UNKNOWN_SUBJECT_RELATION: "subject relation not found",
    ITEM_ERR_WILDCARD_SUBJECT: "cannot perform check on wildcard subject",
    ITEM_ERR_CAVEAT_EVAL: "evaluation error for caveat",
}


class GckError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"gck error {code}: {message}")
        self.code = code
        self.message = message


class _Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_depth", C.c_uint32), ("max_batch", C.c_uint32),
                ("flags", C.c_uint32), ("visited_capacity", C.c_uint64),
                ("frontier_capacity", C.c_uint64), ("segment_capacity", C.c_uint64),
                ("query_capacity", C.c_uint64), ("bundle_checks", C.c_uint32),
                ("bundle_frontier", C.c_uint32), ("bundle_visited", C.c_uint32),
                ("bundle_waves_per_cu", C.c_uint32), ("bundle_budget", C.c_uint32),
                ("giant_frontier", C.c_uint32), ("giant_visited", C.c_uint32),
                ("giant_slots", C.c_uint32), ("bidir_both", C.c_uint32),
                ("workspaces", C.c_uint32)]


class _Consistency(C.Structure):
    _fields_ = [("requirement", C.c_int32), ("reserved", C.c_uint32), ("revision", C.c_uint64)]


class _Stats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("levels", C.c_uint64), ("entries_expanded", C.c_uint64),
                ("row_lookups", C.c_uint64), ("membership_probes", C.c_uint64),
                ("edges_enumerated", C.c_uint64), ("ext_edges", C.c_uint64),
                ("queries", C.c_uint64), ("joins", C.c_uint64), ("retries", C.c_uint64),
                ("kernel_ms", C.c_double), ("expand_ms", C.c_double), ("edges_ms", C.c_double),
                ("resolve_ms", C.c_double), ("expand_launches", C.c_uint64),
                ("edges_launches", C.c_uint64), ("bundle_ms", C.c_double),
                ("bundle_launches", C.c_uint64), ("deferred", C.c_uint64),
                ("giant_ms", C.c_double), ("deferred_wide", C.c_uint64),
                ("bidir_checks", C.c_uint64), ("bundles", C.c_uint64), ("closure_checks", C.c_uint64),
                ("caveat_evals", C.c_uint64), ("caveat_passes", C.c_uint64), ("slot_checks", C.c_uint64),
                ("label_checks", C.c_uint64), ("aql_batches", C.c_uint64), ("resident_batches", C.c_uint64)]


class Uniform(C.Structure):
    """gck_uniform (include/gck.h): the shared shape of a uniform request's checks."""
    _fields_ = [("resource_type", C.c_uint16), ("permission", C.c_uint16), ("subject_type", C.c_uint16),
                ("subject_relation", C.c_uint16), ("context_slot", C.c_uint32), ("reserved", C.c_uint32)]


def _header(h) -> Uniform:
    """A uniform request's header from (resource_type, permission, subject_type, subject_relation
    [, context_slot])."""
    return Uniform(*h[:4], h[4] if len(h) > 4 else 0, 0)


# gck_item_error: (index, GCK_ITEM_*) of a uniform request's errored checks
ITEM_ERROR_DTYPE = np.dtype([("index", "<u4"), ("code", "<i4")])


def unpack_results(words: np.ndarray, n: int) -> np.ndarray:
    """The Permissionship of each of n checks from a uniform request's packed words (2 bits per
    check, 32 per little-endian u64 word: include/gck.h gck_check_bulk_uniform)."""
    b = np.ascontiguousarray(words, dtype="<u8").view(np.uint8)
    four = np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)
    return four[:n].astype(np.uint8)


class Select(C.Structure):
    """gck_select (include/gck.h): which Permissionships survive a filter request, and the device
    arrays the survivors go to."""
    _fields_ = [("mask", C.c_uint32), ("reserved", C.c_uint32), ("d_out_ids", C.c_void_p), ("d_out_pos", C.c_void_p),
                ("d_out_perm", C.c_void_p), ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


class SelectRows(C.Structure):
    """gck_select_rows (include/gck.h): which Permissionships survive a cross filter request, how many
    each subject keeps, and the device arrays of the CSR they go to."""
    _fields_ = [("mask", C.c_uint32), ("row_limit", C.c_uint32), ("d_out_row_off", C.c_void_p),
                ("d_out_row_n", C.c_void_p), ("d_out_ids", C.c_void_p), ("d_out_col", C.c_void_p),
                ("d_out_perm", C.c_void_p), ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


class SelectCols(C.Structure):
    """gck_select_cols (include/gck.h): which Permissionships survive a cross filter request by
    resource, how many each resource keeps, and the device arrays of the CSR they go to."""
    _fields_ = [("mask", C.c_uint32), ("col_limit", C.c_uint32), ("d_out_col_off", C.c_void_p),
                ("d_out_col_n", C.c_void_p), ("d_out_ids", C.c_void_p), ("d_out_row", C.c_void_p),
                ("d_out_perm", C.c_void_p), ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


class SelectGroups(C.Structure):
    """gck_select_groups (include/gck.h): which Permissionships survive a group filter request, how
    many each group keeps, and the device arrays of the CSR they go to."""
    _fields_ = [("mask", C.c_uint32), ("group_limit", C.c_uint32), ("d_out_row_off", C.c_void_p),
                ("d_out_row_n", C.c_void_p), ("d_out_ids", C.c_void_p), ("d_out_pos", C.c_void_p),
                ("d_out_perm", C.c_void_p), ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


class SelectChanges(C.Structure):
    """gck_select_changes (include/gck.h): which transitions a recheck request over a dense plane
    reports, and the device arrays the change records go to."""
    _fields_ = [("transitions", C.c_uint32), ("reserved", C.c_uint32), ("d_out_ids", C.c_void_p),
                ("d_out_pos", C.c_void_p), ("d_out_trans", C.c_void_p), ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


class SelectRowChanges(C.Structure):
    """gck_select_row_changes (include/gck.h): which transitions a recheck cross request reports, and
    the device arrays of the CSR by subject the change records go to."""
    _fields_ = [("transitions", C.c_uint32), ("reserved", C.c_uint32), ("d_out_row_off", C.c_void_p),
                ("d_out_ids", C.c_void_p), ("d_out_col", C.c_void_p), ("d_out_trans", C.c_void_p),
                ("cap", C.c_size_t), ("d_out_n", C.c_void_p)]


SELECT_NO = 1 << PERM_NO                       # GCK_SELECT_NO
SELECT_HAS = 1 << PERM_HAS                     # GCK_SELECT_HAS
SELECT_CONDITIONAL = 1 << PERM_CONDITIONAL     # GCK_SELECT_CONDITIONAL
SELECT_LOOKUP = SELECT_HAS | SELECT_CONDITIONAL  # GCK_SELECT_LOOKUP: LookupResources' rule

# A transition (old value v, new value w) of PERM_* is bit 4 * v + w of a `transitions` word, and a
# change record's transition byte is that bit index.
CHANGE_GAINED = 0x00CC  # GCK_CHANGE_GAINED: {UNSPECIFIED, NO} -> {HAS, CONDITIONAL}
CHANGE_LOST = 0x3300    # GCK_CHANGE_LOST: {HAS, CONDITIONAL} -> {UNSPECIFIED, NO}
CHANGE_ANY = 0x7BDE     # GCK_CHANGE_ANY: every pair of different values


def change_split(trans):
    """A change record's transition byte (an int, or an array of them) as (old, new) PERM_* values."""
    return trans >> 2, trans & 3


CROSS_IDS = 2048  # GCK_CROSS_IDS
VARY_RESOURCE = 1  # GCK_VARY_RESOURCE: a list request's ids are resource ids (the fixed id is the subject's)
VARY_SUBJECT = 2   # GCK_VARY_SUBJECT: ... subject ids (the fixed id is the resource's)


def unpack_cross(words: np.ndarray, S: int, R: int) -> np.ndarray:
    """The Permissionship of every (subject, resource) of a cross request (gck_check_bulk_cross) as
    uint8[S, R], from its row-padded plane: S rows of ceil(R / 32) words, padding ignored."""
    stride = (R + 31) // 32
    b = np.ascontiguousarray(words, dtype="<u8").reshape(-1)[:S * stride].view(np.uint8).reshape(S, stride * 8)
    four = np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(S, stride * 32)
    return np.ascontiguousarray(four[:, :R]).astype(np.uint8)


def cross_tile(S: int, R: int, max_batch: int = 65536) -> Optional[Tuple[int, int]]:
    """gck_cross_tile: the (rows, cols) tile an in-place cross request of S subjects by R resources
    is cut into on an engine of that max_batch, or None when the request is expanded to items."""
    rows, cols = C.c_uint32(0), C.c_uint32(0)
    ok = load_library().gck_cross_tile(S, R, max_batch, C.byref(rows), C.byref(cols))
    return (rows.value, cols.value) if ok else None


def cross_tile_device(S: int, R: int, max_batch: int = 65536) -> int:
    """gck_cross_tile_device: the subjects of a full-width tile (rows x all R resources) a cross
    request over device buffers is cut into in place, or 0 when the request is expanded to items."""
    rows = C.c_uint32(0)
    ok = load_library().gck_cross_tile_device(S, R, max_batch, C.byref(rows))
    return rows.value if ok else 0


def cross_sub_off(R: int) -> int:
    """The word at which a cross id block's subject ids begin: R rounded up to a multiple of four."""
    return (R + 3) & ~3


def cross_id_block(subjects, resources):
    """One tensor in the block layout a cross device request of one tile is read from in place — the
    R resource ids, padding (0) to a multiple of four words, then the S subject ids — and the two
    views into it: (block, subjects_view, resources_view). The views are what check_cross_device /
    submit_cross_device take as d_subjects / d_resources. Tensors of any device, int32 or uint32."""
    import torch
    resources = resources.reshape(-1)
    subjects = subjects.reshape(-1).to(device=resources.device, dtype=resources.dtype)
    R, S, off = resources.numel(), subjects.numel(), cross_sub_off(resources.numel())
    block = torch.zeros(off + S, dtype=resources.dtype, device=resources.device)
    block[:R] = resources
    block[off:] = subjects
    return block, block[off:off + S], block[:R]


MAX_SHAPES = 64  # GCK_MAX_SHAPES
_SHAPE_FIELDS = ("resource_type", "permission", "subject_type", "subject_relation", "context_slot")


def _shape_table(shapes):
    """A ctypes array of gck_uniform from (resource_type, permission, subject_type,
    subject_relation[, context_slot[, reserved]]) tuples (or Uniform structures)."""
    rows = [h if isinstance(h, Uniform) else
            Uniform(*[int(x) for x in h[:4]], int(h[4]) if len(h) > 4 else 0, int(h[5]) if len(h) > 5 else 0)
            for h in shapes]
    return (Uniform * max(1, len(rows)))(*rows), len(rows)


def shape_request(items: np.ndarray):
    """A request's items as a shaped request (gck_check_bulk_shaped): (shapes, shape_of, pairs) —
    the distinct (resource type, permission, subject type, subject relation, context slot) tuples
    in first-seen order, each check's index into them (u8) and its (resource id, subject id) pair
    ((n, 2) u32). None when the items hold more than MAX_SHAPES shapes."""
    items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
    n = len(items)
    pairs = np.empty((n, 2), dtype=np.uint32)
    pairs[:, 0] = items["resource_id"]
    pairs[:, 1] = items["subject_id"]
    key = np.zeros(n, dtype=[(f, "<u4") for f in _SHAPE_FIELDS])
    for f in _SHAPE_FIELDS:
        key[f] = items[f]
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    if len(uniq) > MAX_SHAPES:
        return None
    order = np.argsort(first, kind="stable")      # sorted-unique position -> first-seen rank
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    shapes = [tuple(int(x) for x in uniq[j]) for j in order]
    shape_of = rank[inv.reshape(-1)].astype(np.uint8)
    return shapes, shape_of, pairs


# symbol -> (restype, argtypes); the ABI test checks this list against include/gck.h
_P = C.c_void_p

# gck_transport (include/gck.h): a caller's exchange between the ranks of a partitioned engine
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, _P, _P, C.POINTER(C.c_uint64), _P, C.POINTER(C.c_uint64), _P)
ALLREDUCE_MAX_U8_FN = C.CFUNCTYPE(C.c_int, _P, _P, C.c_uint64, _P)


class Transport(C.Structure):
    _fields_ = [("ctx", _P), ("alltoallv", ALLTOALLV_FN), ("allreduce_max_u8", ALLREDUCE_MAX_U8_FN)]


_SIGS = {
    "gck_abi_version": (C.c_int, []),
    "gck_last_error": (C.c_char_p, []),
    "gck_create": (C.c_int, [C.POINTER(_Config), C.POINTER(_P)]),
    "gck_destroy": (None, [_P]),
    "gck_load_schema": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "gck_type_id": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint16)]),
    "gck_relation_id": (C.c_int, [_P, C.c_uint16, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint16)]),
    "gck_type_count": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "gck_relation_count": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "gck_intern": (C.c_int, [_P, C.c_uint16, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                             C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]),
    "gck_object_count": (C.c_int, [_P, C.c_uint16, C.POINTER(C.c_uint32)]),
    "gck_reserve_objects": (C.c_int, [_P, C.c_uint16, C.c_uint32]),
    "gck_object_name": (C.c_int, [_P, C.c_uint16, C.c_uint32, C.c_char_p, C.c_size_t,
                                  C.POINTER(C.c_size_t)]),
    "gck_add_caveat_instance": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                          C.POINTER(C.c_uint32)]),
    "gck_evaluate_caveat": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p,
                                      C.c_size_t, C.POINTER(C.c_uint8)]),
    "gck_begin_snapshot": (C.c_int, [_P, C.c_uint64]),
    "gck_add_tuples": (C.c_int, [_P, _P, C.c_size_t]),
    "gck_add_tuples_text": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "gck_load_csr": (C.c_int, [_P, C.c_uint16, C.c_uint16, C.c_uint16, C.c_uint32, _P, _P,
                               C.c_uint64, C.c_uint32]),
    "gck_commit_snapshot": (C.c_int, [_P]),
    "gck_save_snapshot": (C.c_int, [_P, C.c_char_p]),
    "gck_load_snapshot_file": (C.c_int, [_P, C.c_char_p]),
    "gck_revision": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_set_head_revision": (C.c_int, [_P, C.c_uint64]),
    "gck_tuple_count": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_device_bytes": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_apply_updates": (C.c_int, [_P, C.c_uint64, _P, C.c_size_t]),
    "gck_apply_updates_text": (C.c_int, [_P, C.c_uint64, C.c_char_p, C.c_size_t]),
    "gck_watch_stage": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_uint64)]),
    "gck_watch_apply_staged": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "gck_watch_discard": (C.c_int, [_P, C.c_uint64]),
    "gck_check_bulk": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, C.c_int64, _P, _P]),
    "gck_check_bulk_device": (C.c_int, [_P, _P, C.c_size_t, C.c_int64, _P, _P, _P]),
    "gck_check_bulk_ctx": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, C.POINTER(C.c_char_p),
                                     C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P]),
    "gck_check_bulk_device_ctx": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                            C.c_size_t, C.c_int64, _P, _P, _P]),
    "gck_check_submit": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, C.POINTER(C.c_char_p),
                                   C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P, C.c_uint32, _P,
                                   C.POINTER(_P)]),
    "gck_set_profile": (C.c_int, [_P, C.c_uint32]),
    "gck_check_wait": (C.c_int, [_P, _P]),
    "gck_check_bulk_at": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, C.POINTER(C.c_char_p),
                                    C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P, C.POINTER(C.c_uint64)]),
    "gck_check_wait_at": (C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_uniform": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t,
                                         C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P,
                                         C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "gck_check_submit_uniform": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t,
                                           C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P,
                                           _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_P)]),
    "gck_check_bulk_shaped": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, _P, _P, C.c_size_t,
                                        C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P,
                                        C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "gck_check_submit_shaped": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, _P, _P, C.c_size_t,
                                          C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P,
                                          _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_P)]),
    "gck_shaped_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_cross": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                       C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                       _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "gck_check_submit_cross": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                         C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                         C.c_int64, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(_P)]),
    "gck_cross_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_cross_tile": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gck_check_bulk_list": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, C.c_uint32, _P,
                                      C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                      C.c_int64, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "gck_check_submit_list": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, C.c_uint32, _P,
                                        C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                        C.c_size_t, C.c_int64, _P, _P, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(_P)]),
    "gck_list_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_uniform_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t,
                                                C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                                _P, _P, C.c_size_t, _P, _P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_shaped_device": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, _P, _P, C.c_size_t,
                                               C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                               _P, _P, C.c_size_t, _P, _P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, C.c_uint32,
                                             _P, C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                             C.c_size_t, C.c_int64, _P, _P, C.c_size_t, _P, _P,
                                             C.POINTER(C.c_uint64)]),
    "gck_check_submit_uniform_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t,
                                                  C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                                  _P, _P, C.c_size_t, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "gck_check_submit_shaped_device": (C.c_int, [_P, C.POINTER(_Consistency), _P, C.c_size_t, _P, _P, C.c_size_t,
                                                 C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                                 _P, _P, C.c_size_t, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "gck_check_submit_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32,
                                               C.c_uint32, _P, C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p),
                                               C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P, _P, C.c_size_t, _P,
                                               C.c_uint32, _P, C.POINTER(_P)]),
    "gck_device_compact_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "gck_check_bulk_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                              C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                              C.c_int64, _P, _P, C.c_size_t, _P, _P, C.POINTER(C.c_uint64)]),
    "gck_check_submit_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                                C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                C.c_int64, _P, _P, C.c_size_t, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "gck_cross_tile_device": (C.c_int, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32)]),
    "gck_filter_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, C.c_uint32, _P,
                                         C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                         C.c_size_t, C.c_int64, C.POINTER(Select), _P, _P, C.c_size_t, _P, _P,
                                         C.POINTER(C.c_uint64)]),
    "gck_filter_submit_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32,
                                                C.c_uint32, _P, C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p),
                                                C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, C.POINTER(Select), _P,
                                                _P, C.c_size_t, _P, C.c_uint32, _P, C.POINTER(_P)]),
    "gck_filter_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                          C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                          C.c_int64, C.POINTER(SelectRows), _P, _P, C.c_size_t, _P, _P,
                                          C.POINTER(C.c_uint64)]),
    "gck_filter_submit_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                                 C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                 C.c_int64, C.POINTER(SelectRows), _P, _P, C.c_size_t, _P, C.c_uint32,
                                                 _P, C.POINTER(_P)]),
    "gck_filter_cross_cols_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                               C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                               C.c_int64, C.POINTER(SelectCols), _P, _P, C.c_size_t, _P, _P,
                                               C.POINTER(C.c_uint64)]),
    "gck_filter_submit_cross_cols_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t,
                                                      _P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                                      C.c_size_t, C.c_int64, C.POINTER(SelectCols), _P, _P, C.c_size_t,
                                                      _P, C.c_uint32, _P, C.POINTER(_P)]),
    "gck_filter_groups_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, _P, C.c_size_t,
                                           _P, _P, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                           C.c_size_t, C.c_int64, C.POINTER(SelectGroups), _P, _P, C.c_size_t, _P, _P,
                                           C.POINTER(C.c_uint64)]),
    "gck_filter_submit_groups_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, _P,
                                                  C.c_size_t, _P, _P, C.c_size_t, C.POINTER(C.c_char_p),
                                                  C.POINTER(C.c_size_t), C.c_size_t, C.c_int64,
                                                  C.POINTER(SelectGroups), _P, _P, C.c_size_t, _P, C.c_uint32, _P,
                                                  C.POINTER(_P)]),
    "gck_diff_planes_device": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_uint32, C.POINTER(SelectChanges), _P]),
    "gck_diff_cross_planes_device": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, C.POINTER(SelectRowChanges), _P]),
    "gck_recheck_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32, C.c_uint32, _P,
                                          C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                          C.c_size_t, C.c_int64, _P, C.POINTER(SelectChanges), _P, _P, C.c_size_t, _P,
                                          _P, C.POINTER(C.c_uint64)]),
    "gck_recheck_submit_list_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), C.c_uint32,
                                                 C.c_uint32, _P, C.c_uint32, C.c_size_t, C.POINTER(C.c_char_p),
                                                 C.POINTER(C.c_size_t), C.c_size_t, C.c_int64, _P,
                                                 C.POINTER(SelectChanges), _P, _P, C.c_size_t, _P, C.c_uint32, _P,
                                                 C.POINTER(_P)]),
    "gck_recheck_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                           C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                           C.c_int64, _P, C.POINTER(SelectRowChanges), _P, _P, C.c_size_t, _P, _P,
                                           C.POINTER(C.c_uint64)]),
    "gck_recheck_submit_cross_device": (C.c_int, [_P, C.POINTER(_Consistency), C.POINTER(Uniform), _P, C.c_size_t, _P,
                                                  C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t,
                                                  C.c_int64, _P, C.POINTER(SelectRowChanges), _P, _P, C.c_size_t, _P,
                                                  C.c_uint32, _P, C.POINTER(_P)]),
    "gck_lookup_resources_among": (C.c_int, [_P, C.POINTER(_Consistency), C.c_uint16, C.c_uint16, C.c_uint16,
                                             C.c_uint16, C.c_uint32, _P, C.c_size_t, C.c_int64, _P, _P, C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "gck_lookup_subjects_among": (C.c_int, [_P, C.POINTER(_Consistency), C.c_uint16, C.c_uint32, C.c_uint16,
                                            C.c_uint16, C.c_uint16, _P, C.c_size_t, C.c_int64, _P, _P, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "gck_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "gck_host_free": (C.c_int, [_P, _P]),
    "gck_last_stats": (C.c_int, [_P, C.POINTER(_Stats)]),
    "gck_lookup_resources": (C.c_int, [_P, C.POINTER(_Consistency), C.c_uint16, C.c_uint16, C.c_uint16,
                                       C.c_uint16, C.c_uint32, C.c_int64, _P, _P, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "gck_lookup_subjects": (C.c_int, [_P, C.POINTER(_Consistency), C.c_uint16, C.c_uint32, C.c_uint16,
                                      C.c_uint16, C.c_uint16, C.c_int64, _P, _P, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "gck_set_partition": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "gck_partition_owner": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "gck_partition_owner_name": (C.c_uint32, [C.c_uint16, C.c_char_p, C.c_size_t, C.c_uint32]),
    "gck_part_intern_with": (C.c_int, [_P, C.POINTER(Transport), _P, _P, _P, C.c_size_t, C.c_uint32, _P]),
    "gck_part_add_tuples_text_with": (C.c_int, [_P, C.POINTER(Transport), C.c_char_p, C.c_size_t]),
    "gck_interned_names": (C.c_int, [_P, C.c_uint16, C.POINTER(C.c_uint32)]),
    "gck_part_check_with": (C.c_int, [_P, C.POINTER(Transport), _P, C.c_size_t, C.c_int64, _P, _P, _P]),
    "gck_part_unique_id": (C.c_int, [_P]),
    "gck_part_init": (C.c_int, [_P, _P]),
    "gck_part_check": (C.c_int, [_P, _P, C.c_size_t, C.c_int64, _P, _P, _P]),
    "gck_reset_stats": (C.c_int, [_P]),
}

_lib = None


_DRIVER = None


def _cpulist(text: str) -> List[int]:
    out = []
    for tok in text.strip().split(","):
        if tok:
            a, _, b = tok.partition("-")
            out.extend(range(int(a), int(b or a) + 1))
    return out


def device_numa_node(device: int = 0) -> Tuple[int, str]:
    """The NUMA node of the GPU's PCIe root (sysfs), and its PCI address; -1 when unknown."""
    import torch
    p = torch.cuda.get_device_properties(device)
    bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
    try:
        with open(f"/sys/bus/pci/devices/{bdf}/numa_node") as f:
            return int(f.read().strip()), bdf
    except (OSError, ValueError):
        return -1, bdf


def pin_to_device_node(device: int = 0) -> dict:
    """Runs the calling process on the CPUs of the GPU's NUMA node (those of them it may use).

    A host batch's items are read by the GPU across PCIe right after the submitting thread wrote
    them: from a thread on the other socket every line is snooped out of a remote cache, and
    the copy engines and kernels read host memory ~10 % slower (tools/pcie_probe: zero-copy reads
    36 vs 40 GB/s, DMA 28-32 vs 41 GB/s). Pinned buffers already come from the GPU's node
    (hipHostMalloc follows the device). Returns what was done, for the bench line."""
    node, bdf = device_numa_node(device)
    allowed = sorted(os.sched_getaffinity(0))
    info = {"gpu_bdf": bdf, "gpu_numa_node": node, "cpus_allowed": len(allowed), "pinned": False}
    if node < 0:
        return info
    try:
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            local = set(_cpulist(f.read()))
    except OSError:
        return info
    use = [c for c in allowed if c in local]
    if use and len(use) < len(allowed):
        os.sched_setaffinity(0, use)
        info.update(pinned=True, cpus_used=len(use))
    elif use:
        info.update(cpus_used=len(use))
    return info


def _driver():
    """libgck_driver.so (csrc/driver.cpp): the compiled submit/wait loop bench.py times through."""
    global _DRIVER
    if _DRIVER is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgck_driver.so")
        if not os.path.exists(path):
            raise OSError(f"{path} is missing: build it with `make -C gochugaru_amd/csrc`")
        d = C.CDLL(path)
        d.gckd_run.restype = C.c_int
        d.gckd_run.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64,
                               C.POINTER(C.c_double)]
        d.gckd_run_host.restype = C.c_int
        d.gckd_run_host.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_uint32, C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_uniform.restype = C.c_int
        d.gckd_run_uniform.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                       C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_shaped.restype = C.c_int
        d.gckd_run_shaped.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_cross.restype = C.c_int
        d.gckd_run_cross.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_list.restype = C.c_int
        d.gckd_run_list.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_uniform_device.restype = C.c_int
        d.gckd_run_uniform_device.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_list_device.restype = C.c_int
        d.gckd_run_list_device.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64,
                                           C.POINTER(C.c_double)]
        d.gckd_run_cross_device.restype = C.c_int
        d.gckd_run_cross_device.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64,
                                            C.POINTER(C.c_double)]
        d.gckd_run_filter_device.restype = C.c_int
        d.gckd_run_filter_device.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_filter_cross_device.restype = C.c_int
        d.gckd_run_filter_cross_device.argtypes = [C.c_void_p, C.c_void_p, _P, C.c_void_p, C.c_size_t, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                   C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                   C.c_int64, C.POINTER(C.c_double)]
        d.gckd_run_filter_cross_cols_device.restype = C.c_int
        d.gckd_run_filter_cross_cols_device.argtypes = list(d.gckd_run_filter_cross_device.argtypes)  # (its twin)
        d.gckd_set_trace.restype = None
        d.gckd_set_trace.argtypes = [C.c_void_p, C.c_size_t]
        _DRIVER = d
    return _DRIVER


def load_library(path: str = _LIB_PATH):
    """Load libgck.so (raises if it has not been built — there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(
            f"libgck.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (make -C gochugaru_amd/csrc); the check engine has no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME
    # libamdhip64.so.7) and loads it by file name. If libgck were loaded first, the process
    # would end up with two HIP runtimes and torch could not see the GPU. Loading torch first
    # makes libgck's NEEDED libamdhip64.so.7 resolve to the already-loaded runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int):
    if rc != GCK_OK:
        msg = _lib.gck_last_error().decode("utf-8", "replace")
        raise GckError(rc, msg)


class Stats(dict):
    pass


class Engine:
    """One engine = one device-resident snapshot on one GPU (``gck_engine``)."""

    def __init__(self, device: int = 0, max_depth: int = 50, max_batch: int = 65536,
                 visited_capacity: int = 0, frontier_capacity: int = 0,
                 segment_capacity: int = 0, query_capacity: int = 0, profile: bool = False,
                 wide_only: bool = False, bundle_checks: int = 0, bundle_frontier: int = 0,
                 bundle_visited: int = 0, bundle_waves_per_cu: int = 0,
                 membership_hash: bool = True, bundle_budget: int = 0, giant_frontier: int = 0,
                 giant_visited: int = 0, giant_slots: int = 0, giant_stage: bool = True,
                 bidir: bool = True, bidir_both: int = 0, workspaces: int = 0, closure: bool = True,
                 lazy_caveats: bool = False, slots: bool = True, labels: bool = True, resident: bool = False,
                 big_membership_hash: bool = False):
        lib = load_library()
        flags = ((FLAG_PROFILE if profile else 0) | (FLAG_NO_BUNDLE if wide_only else 0)
                 | (0 if membership_hash else FLAG_NO_MHASH) | (0 if giant_stage else FLAG_NO_GIANT)
                 | (0 if bidir else FLAG_NO_BIDIR) | (0 if closure else FLAG_NO_CLOSURE)
                 | (FLAG_LAZY_CAVEATS if lazy_caveats else 0) | (0 if slots else FLAG_NO_SLOTS)
                 | (0 if labels else FLAG_NO_LABELS) | (FLAG_RESIDENT if resident else 0)
                 | (FLAG_BIG_MHASH if big_membership_hash else 0))
        cfg = _Config(device, max_depth, max_batch, flags, visited_capacity, frontier_capacity,
                      segment_capacity, query_capacity, bundle_checks, bundle_frontier,
                      bundle_visited, bundle_waves_per_cu, bundle_budget, giant_frontier,
                      giant_visited, giant_slots, bidir_both, workspaces)
        h = _P()
        _check(lib.gck_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._lib = lib
        self.device = device    # the HIP device the engine lives on (filter_ids allocates there)
        self._pins = 0         # live host_array() buffers (each keeps the engine handle alive)
        self._closing = False
        self._staged = {}       # ticket -> the staged Watch batch's array (kept alive until applied)
        self._type_ids = {}
        self._rel_ids = {}
        self.part_rank, self.part_world = 0, 1

    def close(self):
        """Destroys the engine — once the last host_array() buffer is gone, since gck_destroy
        frees the pinned memory those arrays view."""
        self._closing = True
        if self._h and self._pins == 0:
            self._lib.gck_destroy(self._h)
            self._h = None

    def _unpin(self, p):
        self._pins -= 1
        if self._h:
            self._lib.gck_host_free(self._h, p)
            if self._closing and self._pins == 0:
                self._lib.gck_destroy(self._h)
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- schema --------------------------------------------------------------------------
    def load_schema(self, text: str):
        b = text.encode()
        _check(self._lib.gck_load_schema(self._h, b, len(b)))
        self._type_ids.clear()
        self._rel_ids.clear()

    def type_id(self, name: str) -> int:
        """Type id, or TYPE_INVALID if the type is not defined."""
        t = self._type_ids.get(name)
        if t is None:
            out = C.c_uint16()
            b = name.encode()
            rc = self._lib.gck_type_id(self._h, b, len(b), C.byref(out))
            if rc == GCK_E_NOT_FOUND:
                return TYPE_INVALID
            _check(rc)
            t = self._type_ids[name] = out.value
        return t

    def relation_id(self, type_id: int, name: str) -> int:
        """Global relation id, or REL_INVALID if not defined on the type."""
        key = (type_id, name)
        r = self._rel_ids.get(key)
        if r is None:
            if type_id == TYPE_INVALID:
                return REL_INVALID
            out = C.c_uint16()
            b = name.encode()
            rc = self._lib.gck_relation_id(self._h, type_id, b, len(b), C.byref(out))
            if rc == GCK_E_NOT_FOUND:
                return REL_INVALID
            _check(rc)
            r = self._rel_ids[key] = out.value
        return r

    def counts(self) -> Tuple[int, int]:
        t, r = C.c_uint32(), C.c_uint32()
        _check(self._lib.gck_type_count(self._h, C.byref(t)))
        _check(self._lib.gck_relation_count(self._h, C.byref(r)))
        return t.value, r.value

    # ---- interning -----------------------------------------------------------------------
    def intern(self, type_id: int, ids: Sequence[str], create: bool = False) -> np.ndarray:
        n = len(ids)
        out = np.empty(n, dtype=np.uint32)
        if n == 0:
            return out
        enc = [s.encode() for s in ids]
        arr = (C.c_char_p * n)(*enc)
        lens = (C.c_uint32 * n)(*[len(b) for b in enc])
        _check(self._lib.gck_intern(self._h, type_id, arr, lens, n,
                                    INTERN_CREATE if create else 0,
                                    out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def object_count(self, type_id: int) -> int:
        out = C.c_uint32()
        _check(self._lib.gck_object_count(self._h, type_id, C.byref(out)))
        return out.value

    def reserve_objects(self, type_id: int, n: int):
        _check(self._lib.gck_reserve_objects(self._h, type_id, n))

    def object_name(self, type_id: int, oid: int) -> str:
        buf = C.create_string_buffer(1100)
        ln = C.c_size_t()
        _check(self._lib.gck_object_name(self._h, type_id, oid, buf, len(buf), C.byref(ln)))
        return buf.value.decode()

    def add_caveat_instance(self, name: str, context_json: str = "") -> int:
        out = C.c_uint32()
        nb, jb = name.encode(), context_json.encode()
        _check(self._lib.gck_add_caveat_instance(self._h, nb, len(nb), jb, len(jb), C.byref(out)))
        return out.value

    def evaluate_caveat(self, name: str, stored=None, context=None) -> int:
        """The host CEL evaluator: CAVEAT_FALSE / CAVEAT_TRUE / CAVEAT_PARTIAL."""
        out = C.c_uint8()
        nb = name.encode()
        sb = _context_json(stored).encode()
        cb = _context_json(context).encode()
        _check(self._lib.gck_evaluate_caveat(self._h, nb, len(nb), sb, len(sb), cb, len(cb), C.byref(out)))
        return out.value

    # ---- snapshot ------------------------------------------------------------------------
    def begin_snapshot(self, revision: int):
        _check(self._lib.gck_begin_snapshot(self._h, revision))

    def add_tuples_text(self, text: str):
        b = text.encode()
        _check(self._lib.gck_add_tuples_text(self._h, b, len(b)))

    def add_tuples(self, tuples: np.ndarray):
        tuples = np.ascontiguousarray(tuples, dtype=TUPLE_DTYPE)
        _check(self._lib.gck_add_tuples(self._h, tuples.ctypes.data, len(tuples)))

    def load_csr(self, relation: int, subject_type: int, subject_relation: int, n_rows: int,
                 offsets, neighbours, n_edges: int, device: bool = False):
        """Bulk ingest of one prebuilt CSR. Host numpy arrays (uint32) or, with device=True,
        raw device pointers (ints) on the engine's GPU."""
        if device:
            po, pn = int(offsets), int(neighbours)
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
            neighbours = np.ascontiguousarray(neighbours, dtype=np.uint32)
            po, pn = offsets.ctypes.data, neighbours.ctypes.data
        _check(self._lib.gck_load_csr(self._h, relation, subject_type, subject_relation, n_rows,
                                      po, pn, n_edges, MEM_DEVICE if device else 0))

    def commit_snapshot(self):
        _check(self._lib.gck_commit_snapshot(self._h))

    def save_snapshot(self, path: str):
        """Writes the committed snapshot to `path` (the on-disk snapshot cache, gck_save_snapshot)."""
        _check(self._lib.gck_save_snapshot(self._h, os.fsencode(path)))

    def load_snapshot_file(self, path: str):
        """Replaces the committed snapshot with one saved under the same schema text."""
        _check(self._lib.gck_load_snapshot_file(self._h, os.fsencode(path)))

    def load_snapshot_text(self, revision: int, text: str):
        self.begin_snapshot(revision)
        self.add_tuples_text(text)
        self.commit_snapshot()

    @property
    def revision(self) -> int:
        out = C.c_uint64()
        _check(self._lib.gck_revision(self._h, C.byref(out)))
        return out.value

    def set_head_revision(self, revision: int):
        """The source's head revision for consistency.Full() (ReadSchema's ReadAt token,
        client/client.go:416-422, or a Watch checkpoint)."""
        _check(self._lib.gck_set_head_revision(self._h, revision))

    @property
    def tuple_count(self) -> int:
        out = C.c_uint64()
        _check(self._lib.gck_tuple_count(self._h, C.byref(out)))
        return out.value

    @property
    def device_bytes(self) -> int:
        out = C.c_uint64()
        _check(self._lib.gck_device_bytes(self._h, C.byref(out)))
        return out.value

    # ---- Watch updates (Client.UpdatesSinceRevision, client/client.go:370-413) -------------
    def apply_updates(self, revision: int, updates: np.ndarray):
        """One batch of interned updates (UPDATE_DTYPE records, stream order) -> `revision`."""
        updates = np.ascontiguousarray(updates, dtype=UPDATE_DTYPE)
        _check(self._lib.gck_apply_updates(self._h, revision, updates.ctypes.data if len(updates) else None,
                                           len(updates)))

    def stage_updates(self, updates: np.ndarray) -> int:
        """Stages a batch (gck_watch_stage): the engine's thread validates and groups it while the
        caller applies the previous one. Returns the ticket for `apply_staged`; the array is held
        until then."""
        updates = np.ascontiguousarray(updates, dtype=UPDATE_DTYPE)
        t = C.c_uint64(0)
        _check(self._lib.gck_watch_stage(self._h, updates.ctypes.data if len(updates) else None, len(updates),
                                         C.byref(t)))
        self._staged[t.value] = updates
        return t.value

    def apply_staged(self, revision: int, ticket: int):
        """Applies a staged batch -> `revision` (gck_watch_apply_staged; the errors of apply_updates)."""
        try:
            _check(self._lib.gck_watch_apply_staged(self._h, revision, ticket))
        finally:
            self._staged.pop(ticket, None)

    def discard_staged(self, ticket: int):
        try:
            _check(self._lib.gck_watch_discard(self._h, ticket))
        finally:
            self._staged.pop(ticket, None)

    def apply_updates_text(self, revision: int, text: str):
        """One batch as text: "<CREATE|TOUCH|DELETE> <rel.Relationship.String>" per line."""
        b = text.encode()
        _check(self._lib.gck_apply_updates_text(self._h, revision, b, len(b)))

    # ---- checks --------------------------------------------------------------------------
    def check_bulk(self, items: np.ndarray, requirement: int = CONSISTENCY_MIN_LATENCY,
                   revision: int = 0, now_us: int = 0,
                   contexts: Optional[Sequence] = None) -> Tuple[np.ndarray, np.ndarray]:
        """`contexts`: check-time caveat contexts (dicts or JSON text); an item's context_slot
        k selects contexts[k-1] (make_request builds both)."""
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = len(items)
        perm = np.zeros(n, dtype=np.uint8)
        err = np.zeros(n, dtype=np.int32)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        _check(self._lib.gck_check_bulk_ctx(self._h, C.byref(cs), items.ctypes.data if n else None, n,
                                            ctx_arr, ctx_lens, n_ctx, now_us,
                                            perm.ctypes.data if n else None,
                                            err.ctypes.data if n else None))
        return perm, err

    def check_bulk_at(self, items: np.ndarray, requirement: int = CONSISTENCY_MIN_LATENCY,
                      revision: int = 0, now_us: int = 0,
                      contexts: Optional[Sequence] = None) -> Tuple[np.ndarray, np.ndarray, int]:
        """check_bulk plus the revision the batch was evaluated at (gck_check_bulk_at): the
        response's CheckedAt."""
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = len(items)
        perm = np.zeros(n, dtype=np.uint8)
        err = np.zeros(n, dtype=np.int32)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_at(self._h, C.byref(cs), items.ctypes.data if n else None, n, ctx_arr,
                                           ctx_lens, n_ctx, now_us, perm.ctypes.data if n else None,
                                           err.ctypes.data if n else None, C.byref(rev)))
        return perm, err, rev.value

    def check_uniform(self, header, pairs: np.ndarray, requirement: int = CONSISTENCY_MIN_LATENCY,
                      revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None,
                      out_packed: Optional[np.ndarray] = None, out_errs: Optional[np.ndarray] = None):
        """A uniform request (gck_check_bulk_uniform): `header` = (resource_type, permission,
        subject_type, subject_relation, context_slot), `pairs` = (n, 2) u32 (resource id, subject
        id). Returns (packed words, errors as ITEM_ERROR_DTYPE records, evaluated revision);
        unpack_results(words, n) gives the Permissionships. Pinned output arrays (host_array) are
        written in place by the kernels."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        hdr = _header(header)
        return self._check_compact(self._lib.gck_check_bulk_uniform, (C.byref(hdr),), pairs, requirement, revision,
                                   now_us, contexts, out_packed, out_errs)

    def _check_compact(self, fn, head, pairs, requirement, revision, now_us, contexts, out_packed, out_errs):
        """check_uniform / check_shaped after their own arguments: `head` is what the call names
        before the pairs (the header; or the table, its length and the index bytes)."""
        n = len(pairs)
        words = out_packed if out_packed is not None else np.zeros((n + 31) // 32, dtype=np.uint64)
        errs = out_errs if out_errs is not None else np.zeros(n, dtype=ITEM_ERROR_DTYPE)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        n_errs = C.c_size_t(0)
        rev = C.c_uint64(0)
        _check(fn(self._h, C.byref(cs), *head, pairs.ctypes.data if n else None, n, ctx_arr, ctx_lens, n_ctx, now_us,
                  words.ctypes.data if n else None, errs.ctypes.data if len(errs) else None, len(errs),
                  C.byref(n_errs), C.byref(rev)))
        return words, errs[:min(n_errs.value, len(errs))].copy(), rev.value

    def submit_uniform(self, header, pairs: np.ndarray, out_packed: np.ndarray, out_errs: np.ndarray,
                       requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                       contexts: Optional[Sequence] = None) -> "UniformBatch":
        """gck_check_submit_uniform: the results land in out_packed / out_errs at wait()."""
        hdr = _header(header)
        return self._submit_compact(self._lib.gck_check_submit_uniform, (C.byref(hdr),),
                                    UniformBatch(self, hdr, pairs, out_packed, out_errs), requirement, revision,
                                    now_us, contexts)

    def _submit_compact(self, fn, head, b, requirement, revision, now_us, contexts):
        """submit_uniform / submit_shaped after their own arguments (`head` as _check_compact's): `b`
        is the batch to return, holding the arrays the call reads and writes."""
        n = len(b._pairs)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        _check(fn(self._h, C.byref(cs), *head, b._pairs.ctypes.data if n else None, n, ctx_arr, ctx_lens, n_ctx,
                  now_us, b.packed.ctypes.data if n else None, b.errs.ctypes.data if len(b.errs) else None,
                  len(b.errs), C.byref(b._n_errs), C.byref(b._h)))
        return b

    def prepare_uniform(self, headers, pairs, ns, packed, errs, err_cap: int, depth: int,
                        now_us: int = 0) -> "PreparedUniform":
        """The compiled submit/wait loop over uniform requests (libgck_driver.so gckd_run_uniform),
        its arguments marshalled ahead: request k = headers[k] (gck_uniform fields) and host pointers
        pairs[k] (ns[k] pairs), packed[k], errs[k] (err_cap records), `depth` in flight."""
        return PreparedUniform(self, headers, pairs, ns, packed, errs, err_cap, depth, now_us)

    def run_uniform_batches(self, header, pairs, packed, errs, err_cap: int, n: int, depth: int,
                            now_us: int = 0) -> float:
        """prepare_uniform(...).run() for requests of one header and n checks each; returns the loop's
        wall time in seconds."""
        k = len(pairs)
        return self.prepare_uniform([header] * k, pairs, [n] * k, packed, errs, err_cap, depth, now_us).run()

    def check_shaped(self, shapes, shape_of: np.ndarray, pairs: np.ndarray,
                     requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                     contexts: Optional[Sequence] = None, out_packed: Optional[np.ndarray] = None,
                     out_errs: Optional[np.ndarray] = None):
        """A shaped request (gck_check_bulk_shaped): `shapes` = up to MAX_SHAPES headers as
        check_uniform takes one, `shape_of` = n u8 indices into them, `pairs` = (n, 2) u32. Returns
        what check_uniform returns. Pinned arrays (host_array) are read and written in place."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        shape_of = np.ascontiguousarray(shape_of, dtype=np.uint8).reshape(-1)
        n = len(pairs)
        if len(shape_of) != n:
            raise ValueError("shape_of and pairs differ in length")
        table, n_shapes = _shape_table(shapes)
        head = (C.addressof(table), n_shapes, shape_of.ctypes.data if n else None)
        return self._check_compact(self._lib.gck_check_bulk_shaped, head, pairs, requirement, revision, now_us,
                                   contexts, out_packed, out_errs)

    def submit_shaped(self, shapes, shape_of: np.ndarray, pairs: np.ndarray, out_packed: np.ndarray,
                      out_errs: np.ndarray, requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                      now_us: int = 0, contexts: Optional[Sequence] = None) -> "ShapedBatch":
        """gck_check_submit_shaped: the results land in out_packed / out_errs at wait(). `shape_of`
        (u8) and `pairs` (u32) are used as they are (contiguous arrays) and kept until the wait."""
        n = len(pairs)
        if shape_of.dtype != np.uint8 or pairs.dtype != np.uint32 or len(shape_of) != n:
            raise ValueError("submit_shaped takes u8 shape_of and u32 pairs of one length")
        table, n_shapes = _shape_table(shapes)
        head = (C.addressof(table), n_shapes, shape_of.ctypes.data if n else None)
        return self._submit_compact(self._lib.gck_check_submit_shaped, head,
                                    ShapedBatch(self, (table, shape_of), pairs, out_packed, out_errs), requirement,
                                    revision, now_us, contexts)

    def prepare_shaped(self, shapes, shape_of, pairs, ns, packed, errs, err_cap: int, depth: int,
                       now_us: int = 0) -> "PreparedShaped":
        """The compiled submit/wait loop over shaped requests (libgck_driver.so gckd_run_shaped):
        request k = the table shapes[k] (a list of headers) and host pointers shape_of[k], pairs[k]
        (ns[k] checks), packed[k], errs[k] (err_cap records), `depth` in flight."""
        return PreparedShaped(self, shapes, shape_of, pairs, ns, packed, errs, err_cap, depth, now_us)

    def shaped_stats(self) -> Tuple[int, int]:
        """gck_shaped_stats: shaped requests (chunks) the join read in place, and those expanded to
        items on the host, since the engine was created."""
        out = (C.c_uint64 * 2)()
        _check(self._lib.gck_shaped_stats(self._h, out))
        return int(out[0]), int(out[1])

    def check_cross(self, header, subjects: np.ndarray, resources: np.ndarray,
                    requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                    contexts: Optional[Sequence] = None, out_packed: Optional[np.ndarray] = None,
                    out_errs: Optional[np.ndarray] = None):
        """A cross request (gck_check_bulk_cross): every subject id of `subjects` against every
        resource id of `resources` under one `header` (as check_uniform's). Returns (words, errors,
        evaluated revision): words = the row-padded plane, len(subjects) rows of ceil(R / 32) u64
        (unpack_cross gives uint8[S, R]); an error's index is s * R + r."""
        subjects = np.ascontiguousarray(subjects, dtype=np.uint32).reshape(-1)
        resources = np.ascontiguousarray(resources, dtype=np.uint32).reshape(-1)
        S, R = len(subjects), len(resources)
        hdr = header if isinstance(header, Uniform) else _header(header)
        n_words = S * ((R + 31) // 32)
        words = out_packed if out_packed is not None else np.zeros(n_words, dtype=np.uint64)
        errs = out_errs if out_errs is not None else np.zeros(min(S * R, 1 << 20), dtype=ITEM_ERROR_DTYPE)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        n_errs = C.c_size_t(0)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_cross(self._h, C.byref(cs), C.byref(hdr), subjects.ctypes.data if S else None, S,
                                              resources.ctypes.data if R else None, R, ctx_arr, ctx_lens, n_ctx, now_us,
                                              words.ctypes.data if n_words else None,
                                              errs.ctypes.data if len(errs) else None, len(errs), C.byref(n_errs),
                                              C.byref(rev)))
        return words, errs[:min(n_errs.value, len(errs))].copy(), rev.value

    def submit_cross(self, header, subjects: np.ndarray, resources: np.ndarray, out_packed: np.ndarray,
                     out_errs: np.ndarray, requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                     now_us: int = 0, contexts: Optional[Sequence] = None) -> "CrossBatch":
        """gck_check_submit_cross (one tile: cross_tile(S, R, max_batch) == (S, R)): the results land
        in out_packed / out_errs at wait(). The id lists are copied by the call."""
        subjects = np.ascontiguousarray(subjects, dtype=np.uint32).reshape(-1)
        resources = np.ascontiguousarray(resources, dtype=np.uint32).reshape(-1)
        S, R = len(subjects), len(resources)
        hdr = header if isinstance(header, Uniform) else _header(header)
        b = CrossBatch(self, hdr, None, out_packed, out_errs)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        _check(self._lib.gck_check_submit_cross(self._h, C.byref(cs), C.byref(hdr), subjects.ctypes.data if S else None,
                                                S, resources.ctypes.data if R else None, R, ctx_arr, ctx_lens, n_ctx,
                                                now_us, out_packed.ctypes.data if S * R else None,
                                                out_errs.ctypes.data if len(out_errs) else None, len(out_errs),
                                                C.byref(b._n_errs), C.byref(b._h)))
        return b

    def prepare_cross(self, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap: int,
                      depth: int, now_us: int = 0) -> "PreparedCross":
        """The compiled submit/wait loop over cross requests (libgck_driver.so gckd_run_cross):
        request k = headers[k] and host pointers subjects[k] (n_subjects[k] ids), resources[k]
        (n_resources[k] ids), packed[k], errs[k] (err_cap records), `depth` in flight."""
        return PreparedCross(self, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap, depth,
                             now_us)

    def cross_stats(self) -> Tuple[int, int]:
        """gck_cross_stats: cross tiles whose join read the id lists in place, and chunks expanded to
        items on the host, since the engine was created."""
        out = (C.c_uint64 * 2)()
        _check(self._lib.gck_cross_stats(self._h, out))
        return int(out[0]), int(out[1])

    @staticmethod
    def _list_ids(ids, first_id, n):
        """A list request's varying ids as the C ABI takes them: (array or None, first_id, n)."""
        if ids is None:
            if n is None:
                raise ValueError("a range needs n")
            return None, int(first_id), int(n)
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        return ids, 0, len(ids) if n is None else int(n)

    def check_list(self, header, fixed_id: int, vary: int, ids: Optional[np.ndarray] = None, first_id: int = 0,
                   n: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                   now_us: int = 0, contexts: Optional[Sequence] = None, out_packed: Optional[np.ndarray] = None,
                   out_errs: Optional[np.ndarray] = None):
        """A list request (gck_check_bulk_list): one fixed id against n ids of the other side under
        one `header` (as check_uniform's). `vary` = VARY_RESOURCE (fixed_id is the subject id) or
        VARY_SUBJECT (fixed_id is the resource id); the varying ids are `ids` (u32, 4 B per check) or,
        with ids=None, the range first_id .. first_id + n - 1. Returns (words, errors, evaluated
        revision) as check_uniform does: unpack_results(words, n) gives the Permissionships."""
        ids, first_id, n = self._list_ids(ids, first_id, n)
        hdr = header if isinstance(header, Uniform) else _header(header)
        words = out_packed if out_packed is not None else np.zeros((n + 31) // 32, dtype=np.uint64)
        errs = out_errs if out_errs is not None else np.zeros(min(n, 1 << 20), dtype=ITEM_ERROR_DTYPE)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        n_errs = C.c_size_t(0)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_list(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary,
                                             ids.ctypes.data if ids is not None and len(ids) else None, first_id, n,
                                             ctx_arr, ctx_lens, n_ctx, now_us, words.ctypes.data if len(words) else None,
                                             errs.ctypes.data if len(errs) else None, len(errs), C.byref(n_errs),
                                             C.byref(rev)))
        return words, errs[:min(n_errs.value, len(errs))].copy(), rev.value

    def submit_list(self, header, fixed_id: int, vary: int, out_packed: np.ndarray, out_errs: np.ndarray,
                    ids: Optional[np.ndarray] = None, first_id: int = 0, n: Optional[int] = None,
                    requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                    contexts: Optional[Sequence] = None) -> "ListBatch":
        """gck_check_submit_list (one chunk: n <= max_batch): the results land in out_packed /
        out_errs at wait(). A pinned id list (host_array) is read in place until then."""
        ids, first_id, n = self._list_ids(ids, first_id, n)
        hdr = header if isinstance(header, Uniform) else _header(header)
        b = ListBatch(self, hdr, ids, out_packed, out_errs)
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        _check(self._lib.gck_check_submit_list(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary,
                                               ids.ctypes.data if ids is not None and len(ids) else None, first_id, n,
                                               ctx_arr, ctx_lens, n_ctx, now_us,
                                               out_packed.ctypes.data if n else None,
                                               out_errs.ctypes.data if len(out_errs) else None, len(out_errs),
                                               C.byref(b._n_errs), C.byref(b._h)))
        return b

    def prepare_list(self, headers, fixed, vary: int, ids, first, ns, packed, errs, err_cap: int, depth: int,
                     now_us: int = 0) -> "PreparedList":
        """The compiled submit/wait loop over list requests (libgck_driver.so gckd_run_list): request
        k = headers[k], the fixed id fixed[k], and ns[k] varying ids — the host pointer ids[k], or
        with ids[k] == 0 the range from first[k] — with host pointers packed[k], errs[k] (err_cap
        records); every request varies the side `vary`; `depth` in flight."""
        return PreparedList(self, headers, fixed, vary, ids, first, ns, packed, errs, err_cap, depth, now_us)

    def list_stats(self) -> Tuple[int, int]:
        """gck_list_stats: list chunks whose join read the ids in place (or computed a range), and
        chunks expanded to items on the host, since the engine was created."""
        out = (C.c_uint64 * 2)()
        _check(self._lib.gck_list_stats(self._h, out))
        return int(out[0]), int(out[1])

    # ---- compact requests over device buffers (gck_check_bulk_uniform_device ...) ------------
    # Device buffers are integer addresses on the engine's device (torch: tensor.data_ptr()):
    # d_pairs (n, 2) u32, d_shape_of u8, d_ids u32, d_out_packed ceil(n / 32) u64, d_out_errs err_cap
    # ITEM_ERROR_DTYPE records, d_out_n_errs one u32 (0 / None: no count). `stream` as
    # check_bulk_device's. The synchronous forms return the evaluated revision.
    def _device_tail(self, requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap, d_out_n_errs):
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        return cs, (ctx_arr, ctx_lens, n_ctx, now_us, d_out_packed or None, d_out_errs or None, err_cap,
                    d_out_n_errs or None)

    def check_uniform_device(self, header, d_pairs: int, n: int, d_out_packed: int, d_out_errs: int = 0,
                             err_cap: int = 0, d_out_n_errs: int = 0, stream: Optional[int] = None,
                             requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                             contexts: Optional[Sequence] = None) -> int:
        """gck_check_bulk_uniform_device: check_uniform over device buffers; results on the device."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_uniform_device(self._h, C.byref(cs), C.byref(hdr), d_pairs or None, n, *tail,
                                                       stream, C.byref(rev)))
        return rev.value

    def check_shaped_device(self, shapes, d_shape_of: int, d_pairs: int, n: int, d_out_packed: int,
                            d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                            stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                            revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_check_bulk_shaped_device: check_shaped over device buffers (the table is host memory)."""
        table, n_shapes = _shape_table(shapes)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_shaped_device(self._h, C.byref(cs), C.addressof(table), n_shapes,
                                                      d_shape_of or None, d_pairs or None, n, *tail, stream,
                                                      C.byref(rev)))
        return rev.value

    def check_list_device(self, header, fixed_id: int, vary: int, n: int, d_out_packed: int, d_ids: int = 0,
                          first_id: int = 0, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                          stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                          revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_check_bulk_list_device: check_list over a device id list, or (d_ids = 0) the range
        first_id .. first_id + n - 1."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary, d_ids or None,
                                                    first_id, n, *tail, stream, C.byref(rev)))
        return rev.value

    def submit_uniform_device(self, header, d_pairs: int, n: int, d_out_packed: int, d_out_errs: int = 0,
                              err_cap: int = 0, d_out_n_errs: int = 0, stream: Optional[int] = None,
                              engine_stream: bool = False, requirement: int = CONSISTENCY_MIN_LATENCY,
                              revision: int = 0, now_us: int = 0,
                              contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_check_submit_uniform_device (n <= max_batch): on `stream`, or with engine_stream on the
        stream of the workspace the batch holds; wait() completes it and returns its revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_check_submit_uniform_device(self._h, C.byref(cs), C.byref(hdr), d_pairs or None, n, *tail,
                                                         SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                         C.byref(b._h)))
        return b

    def submit_shaped_device(self, shapes, d_shape_of: int, d_pairs: int, n: int, d_out_packed: int,
                             d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                             stream: Optional[int] = None, engine_stream: bool = False,
                             requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                             contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_check_submit_shaped_device: as submit_uniform_device."""
        table, n_shapes = _shape_table(shapes)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        b = DeviceCompactBatch(self, table)
        _check(self._lib.gck_check_submit_shaped_device(self._h, C.byref(cs), C.addressof(table), n_shapes,
                                                        d_shape_of or None, d_pairs or None, n, *tail,
                                                        SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                        C.byref(b._h)))
        return b

    def submit_list_device(self, header, fixed_id: int, vary: int, n: int, d_out_packed: int, d_ids: int = 0,
                           first_id: int = 0, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                           stream: Optional[int] = None, engine_stream: bool = False,
                           requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                           contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_check_submit_list_device: as submit_uniform_device."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_check_submit_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary, d_ids or None,
                                                      first_id, n, *tail, SUBMIT_ENGINE_STREAM if engine_stream else 0,
                                                      stream, C.byref(b._h)))
        return b

    def prepare_uniform_device(self, headers, pairs, ns, packed, errs, err_cap: int, depth: int, n_errs=None,
                               streams=None, engine_streams: bool = True,
                               now_us: int = 0) -> "PreparedUniformDevice":
        """The compiled submit/wait loop over uniform device requests (libgck_driver.so
        gckd_run_uniform_device): as prepare_uniform with device pointers; n_errs[k] is request k's
        device count word (None: none), batch k on streams[k % depth] or the engine's streams."""
        return PreparedUniformDevice(self, headers, pairs, ns, packed, errs, err_cap, depth, n_errs, streams,
                                     engine_streams, now_us)

    def prepare_list_device(self, headers, fixed, vary: int, ids, first, ns, packed, errs, err_cap: int, depth: int,
                            n_errs=None, streams=None, engine_streams: bool = True,
                            now_us: int = 0) -> "PreparedListDevice":
        """The compiled loop over list device requests (gckd_run_list_device): as prepare_list with
        device pointers (ids[k] == 0: the range from first[k])."""
        return PreparedListDevice(self, headers, fixed, vary, ids, first, ns, packed, errs, err_cap, depth, n_errs,
                                  streams, engine_streams, now_us)

    # ---- cross requests over device buffers (gck_check_bulk_cross_device): d_subjects (S) and
    # d_resources (R) u32 id lists, d_out_packed the row-padded plane of S * ceil(R / 32) u64. The
    # lists are read where they are (never copied): unchanged until the call or the wait returns.
    def check_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                           d_out_packed: int, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                           stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                           revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_check_bulk_cross_device: check_cross over two device id lists; the plane and the error
        records (index = s * R + r) on the device. Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        rev = C.c_uint64(0)
        _check(self._lib.gck_check_bulk_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                     n_subjects, d_resources or None, n_resources, *tail, stream,
                                                     C.byref(rev)))
        return rev.value

    def submit_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                            d_out_packed: int, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                            stream: Optional[int] = None, engine_stream: bool = False,
                            requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                            contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_check_submit_cross_device (one device tile: cross_tile_device(S, R, max_batch) == S): as
        submit_uniform_device."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_check_submit_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                       n_subjects, d_resources or None, n_resources, *tail,
                                                       SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                       C.byref(b._h)))
        return b

    def prepare_cross_device(self, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap: int,
                             depth: int, n_errs=None, streams=None, engine_streams: bool = True,
                             now_us: int = 0) -> "PreparedCrossDevice":
        """The compiled loop over cross device requests (gckd_run_cross_device): as prepare_cross with
        device pointers; n_errs[k] is request k's device count word (None: none)."""
        return PreparedCrossDevice(self, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap,
                                   depth, n_errs, streams, engine_streams, now_us)

    def check_cross_ids(self, header, subjects, resources, requirement: int = CONSISTENCY_MIN_LATENCY,
                        revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None):
        """The permission plane of `subjects` x `resources` — device int32 / uint32 tensors of ids —
        as an int64 [S, ceil(R / 32)] device tensor (2 bits per check, unpack_cross's layout). Runs
        check_cross_device on the current stream, reads back only the error count — the call's only
        copy to the host — and raises GckError, with the lookups' message, when it is not 0."""
        import torch
        for name, t in (("subjects", subjects), ("resources", resources)):
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, f"check_cross_ids: {name} must be a device int32 / uint32 tensor")
        if subjects.device != resources.device:
            raise GckError(GCK_E_INVALID_ARGUMENT, "check_cross_ids: the two lists are on different devices")
        subjects, resources = subjects.contiguous().reshape(-1), resources.contiguous().reshape(-1)
        S, R, dev = subjects.numel(), resources.numel(), subjects.device
        with torch.cuda.device(dev):
            plane = torch.empty((S, (R + 31) // 32), dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            err = torch.empty(2, dtype=torch.int32, device=dev)  # the first error record
            self.check_cross_device(header, subjects.data_ptr() if S * R else 0, S, resources.data_ptr() if S * R else 0,
                                    R, plane.data_ptr() if S * R else 0, d_out_errs=err.data_ptr(), err_cap=1,
                                    d_out_n_errs=count.data_ptr(),
                                    stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                    revision=revision, now_us=now_us, contexts=contexts)
            if int(count.item()) & 0xFFFFFFFF:
                code = int(err[1].item())
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               ITEM_ERROR_MESSAGES[ITEM_ERR_MAX_DEPTH] if code == ITEM_ERR_MAX_DEPTH
                               else f"lookup failed: per-item error {code}")
        return plane

    # ---- filter requests (gck_filter_list_device): the list device request, its survivors compacted
    # on the device. d_out_n: one u32 (required); d_out_ids / d_out_pos (u32) and d_out_perm (u8): `cap`
    # entries each, 0: not wanted; d_out_packed may be 0 (the plane stays in the engine).
    def filter_list_device(self, header, fixed_id: int, vary: int, n: int, d_out_n: int, cap: int, d_out_ids: int = 0,
                           d_out_pos: int = 0, d_out_perm: int = 0, select: int = SELECT_LOOKUP, d_out_packed: int = 0,
                           d_ids: int = 0, first_id: int = 0, d_out_errs: int = 0, err_cap: int = 0,
                           d_out_n_errs: int = 0, stream: Optional[int] = None,
                           requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                           contexts: Optional[Sequence] = None) -> int:
        """gck_filter_list_device: check_list_device, then the checks whose Permissionship `select`
        (SELECT_*) names, in request order: their ids, positions and Permissionships into the device
        arrays, their number into *d_out_n. A per-item error does not fail the call (it is counted in
        *d_out_n_errs and never survives). Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = Select(select, 0, d_out_ids or None, d_out_pos or None, d_out_perm or None, cap, d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_filter_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary, d_ids or None,
                                                first_id, n, *tail[:4], C.byref(sel), *tail[4:], stream,
                                                C.byref(rev)))
        return rev.value

    def submit_filter_list_device(self, header, fixed_id: int, vary: int, n: int, d_out_n: int, cap: int,
                                  d_out_ids: int = 0, d_out_pos: int = 0, d_out_perm: int = 0,
                                  select: int = SELECT_LOOKUP, d_out_packed: int = 0, d_ids: int = 0, first_id: int = 0,
                                  d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                                  stream: Optional[int] = None, engine_stream: bool = False,
                                  requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                                  contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_filter_submit_list_device: as submit_list_device, with filter_list_device's outputs."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = Select(select, 0, d_out_ids or None, d_out_pos or None, d_out_perm or None, cap, d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_filter_submit_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary,
                                                       d_ids or None, first_id, n, *tail[:4], C.byref(sel), *tail[4:],
                                                       SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                       C.byref(b._h)))
        return b

    def prepare_filter_device(self, headers, fixed, vary: int, ids, first, ns, out_n, cap: int, depth: int,
                              out_ids=None, out_pos=None, out_perm=None, select: int = SELECT_LOOKUP, packed=None,
                              errs=None, err_cap: int = 0, n_errs=None, streams=None, engine_streams: bool = True,
                              now_us: int = 0) -> "PreparedFilterDevice":
        """The compiled loop over filter requests (gckd_run_filter_device): as prepare_list_device, with
        request k's survivors into out_ids[k] / out_pos[k] / out_perm[k] (`cap` entries; None: not
        wanted) and their number into out_n[k], all under the one `select`; packed may be None."""
        return PreparedFilterDevice(self, headers, fixed, vary, ids, first, ns, select, out_ids, out_pos, out_perm,
                                    cap, out_n, packed, errs, err_cap, depth, n_errs, streams, engine_streams, now_us)

    def filter_ids(self, header, fixed_id: int, vary: int, ids=None, first_id: int = 0, n: Optional[int] = None,
                   select: int = SELECT_LOOKUP, want_pos: bool = False, want_perm: bool = False,
                   requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                   contexts: Optional[Sequence] = None):
        """The survivors of a filter request as torch tensors: `ids` is a device int32 / uint32 tensor
        of varying ids (None: the range first_id .. first_id + n - 1 on the engine's device). Runs
        filter_list_device on the current stream with outputs allocated on the tensor's device, reads
        the two count words — the call's only copy to the host — and returns the surviving ids (in
        the tensor's dtype), then their positions (int64-indexable int32) and Permissionships (uint8)
        when asked for, each sliced to the survivor count. A per-item error raises GckError with the
        lookups' message."""
        import torch
        if ids is not None:
            if ids.dtype not in (torch.int32, torch.uint32) or not ids.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, "filter_ids: ids must be a device int32 / uint32 tensor")
            ids = ids.contiguous().reshape(-1)
            n, dev, dtype = ids.numel(), ids.device, ids.dtype
        else:
            if n is None:
                raise GckError(GCK_E_INVALID_ARGUMENT, "filter_ids: a range needs n")
            dev, dtype = torch.device("cuda", self.device), torch.int32
        with torch.cuda.device(dev):
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [survivors, errors]
            out_ids = torch.empty(n, dtype=dtype, device=dev)
            out_pos = torch.empty(n, dtype=torch.int32, device=dev) if want_pos else None
            out_perm = torch.empty(n, dtype=torch.uint8, device=dev) if want_perm else None
            err = torch.empty(2, dtype=torch.int32, device=dev)  # the first error record
            self.filter_list_device(header, fixed_id, vary, n, counts.data_ptr(), n, d_out_ids=out_ids.data_ptr(),
                                    d_out_pos=out_pos.data_ptr() if want_pos else 0,
                                    d_out_perm=out_perm.data_ptr() if want_perm else 0, select=select,
                                    d_ids=ids.data_ptr() if ids is not None and n else 0, first_id=first_id,
                                    d_out_errs=err.data_ptr(), err_cap=1, d_out_n_errs=counts.data_ptr() + 4,
                                    stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                    revision=revision, now_us=now_us, contexts=contexts)
            total, n_errs = (int(x) & 0xFFFFFFFF for x in counts.tolist())
            if n_errs:
                code = int(err[1].item())
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               ITEM_ERROR_MESSAGES[ITEM_ERR_MAX_DEPTH] if code == ITEM_ERR_MAX_DEPTH
                               else f"lookup failed: per-item error {code}")
        out = (out_ids[:total],)
        if want_pos:
            out += (out_pos[:total],)
        if want_perm:
            out += (out_perm[:total],)
        return out[0] if len(out) == 1 else out

    # ---- cross filter requests (gck_filter_cross_device): the cross device request, each subject's
    # survivors compacted on the device into a CSR. d_out_row_off: S + 1 u32 (required); d_out_n: one
    # u32 (required); d_out_row_n: S u32, 0: not wanted; d_out_ids / d_out_col (u32) and d_out_perm (u8):
    # `cap` entries each, 0: not wanted; d_out_packed is required.
    def filter_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                            d_out_row_off: int, d_out_n: int, cap: int, d_out_packed: int, d_out_ids: int = 0,
                            d_out_col: int = 0, d_out_perm: int = 0, d_out_row_n: int = 0, select: int = SELECT_LOOKUP,
                            row_limit: int = 0, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                            stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                            revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_filter_cross_device: check_cross_device, then for each subject the resources whose
        Permissionship `select` (SELECT_*) names, in list order and at most `row_limit` of them (0: all):
        row offsets, ids, columns and Permissionships into the device arrays, their number into
        *d_out_n. A per-item error does not fail the call. Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectRows(select, row_limit, d_out_row_off or None, d_out_row_n or None, d_out_ids or None,
                         d_out_col or None, d_out_perm or None, cap, d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_filter_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None, n_subjects,
                                                 d_resources or None, n_resources, *tail[:4], C.byref(sel), *tail[4:],
                                                 stream, C.byref(rev)))
        return rev.value

    def submit_filter_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                                   d_out_row_off: int, d_out_n: int, cap: int, d_out_packed: int, d_out_ids: int = 0,
                                   d_out_col: int = 0, d_out_perm: int = 0, d_out_row_n: int = 0,
                                   select: int = SELECT_LOOKUP, row_limit: int = 0, d_out_errs: int = 0,
                                   err_cap: int = 0, d_out_n_errs: int = 0, stream: Optional[int] = None,
                                   engine_stream: bool = False, requirement: int = CONSISTENCY_MIN_LATENCY,
                                   revision: int = 0, now_us: int = 0,
                                   contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_filter_submit_cross_device (one device tile): as submit_cross_device, with
        filter_cross_device's outputs."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectRows(select, row_limit, d_out_row_off or None, d_out_row_n or None, d_out_ids or None,
                         d_out_col or None, d_out_perm or None, cap, d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_filter_submit_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                        n_subjects, d_resources or None, n_resources, *tail[:4],
                                                        C.byref(sel), *tail[4:],
                                                        SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                        C.byref(b._h)))
        return b

    def prepare_filter_cross_device(self, headers, subjects, n_subjects, resources, n_resources, row_off, out_n,
                                    cap: int, packed, depth: int, out_ids=None, out_col=None, out_perm=None,
                                    row_n=None, select: int = SELECT_LOOKUP, row_limit: int = 0, errs=None,
                                    err_cap: int = 0, n_errs=None, streams=None, engine_streams: bool = True,
                                    now_us: int = 0) -> "PreparedFilterCrossDevice":
        """The compiled loop over cross filter requests (gckd_run_filter_cross_device): as
        prepare_cross_device, with request k's CSR into row_off[k] / out_ids[k] / out_col[k] / out_perm[k]
        (`cap` entries; None: not wanted), its rows' survivor counts into row_n[k] and the total into
        out_n[k], all under the one `select` and `row_limit`."""
        return PreparedFilterCrossDevice(self, headers, subjects, n_subjects, resources, n_resources, select, row_limit,
                                         row_off, row_n, out_ids, out_col, out_perm, cap, out_n, packed, errs, err_cap,
                                         depth, n_errs, streams, engine_streams, now_us)

    def filter_cross_ids(self, header, subjects, resources, select: int = SELECT_LOOKUP, row_limit: int = 0,
                         want_col: bool = False, want_perm: bool = False,
                         requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                         contexts: Optional[Sequence] = None):
        """For each of `subjects` the `resources` it may see — device int32 / uint32 tensors of ids — as
        a CSR of torch tensors: (row_off, ids), row_off an int32 [S + 1] tensor and ids (in the
        resources' dtype) the kept survivors of row s at row_off[s] .. row_off[s + 1]; then their
        columns (int32) and Permissionships (uint8) when asked for. `row_limit`: at most so many per
        subject, the first in list order (0: all). Runs filter_cross_device on the current stream with
        outputs allocated on the tensors' device (cap = S * (row_limit or R)) and reads the two count
        words — the call's only copy to the host. A per-item error raises GckError with the lookups'
        message."""
        import torch
        for name, t in (("subjects", subjects), ("resources", resources)):
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, f"filter_cross_ids: {name} must be a device int32 / uint32 tensor")
        if subjects.device != resources.device:
            raise GckError(GCK_E_INVALID_ARGUMENT, "filter_cross_ids: the two lists are on different devices")
        subjects, resources = subjects.contiguous().reshape(-1), resources.contiguous().reshape(-1)
        S, R, dev = subjects.numel(), resources.numel(), subjects.device
        cap = S * (min(row_limit, R) if row_limit else R)
        with torch.cuda.device(dev):
            plane = torch.empty(max(1, S * ((R + 31) // 32)), dtype=torch.int64, device=dev)  # (required, also when empty)
            row_off = torch.empty(S + 1, dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [kept survivors, errors]
            out_ids = torch.empty(cap, dtype=resources.dtype, device=dev)
            out_col = torch.empty(cap, dtype=torch.int32, device=dev) if want_col else None
            out_perm = torch.empty(cap, dtype=torch.uint8, device=dev) if want_perm else None
            err = torch.empty(2, dtype=torch.int32, device=dev)  # the first error record
            self.filter_cross_device(header, subjects.data_ptr() if S * R else 0, S,
                                     resources.data_ptr() if S * R else 0, R, row_off.data_ptr(), counts.data_ptr(),
                                     cap, plane.data_ptr(), d_out_ids=out_ids.data_ptr() if cap else 0,
                                     d_out_col=out_col.data_ptr() if want_col and cap else 0,
                                     d_out_perm=out_perm.data_ptr() if want_perm and cap else 0, select=select,
                                     row_limit=row_limit, d_out_errs=err.data_ptr(), err_cap=1,
                                     d_out_n_errs=counts.data_ptr() + 4,
                                     stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                     revision=revision, now_us=now_us, contexts=contexts)
            total, n_errs = (int(x) & 0xFFFFFFFF for x in counts.tolist())
            if n_errs:
                code = int(err[1].item())
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               ITEM_ERROR_MESSAGES[ITEM_ERR_MAX_DEPTH] if code == ITEM_ERR_MAX_DEPTH
                               else f"lookup failed: per-item error {code}")
        out = (row_off, out_ids[:total])
        if want_col:
            out += (out_col[:total],)
        if want_perm:
            out += (out_perm[:total],)
        return out

    # ---- cross filter requests by resource (gck_filter_cross_cols_device): the mirror — each resource's
    # surviving subjects as a CSR. d_out_col_off: R + 1 u32 (required); d_out_n: one u32 (required);
    # d_out_col_n: R u32, 0: not wanted; d_out_ids / d_out_row (u32) and d_out_perm (u8): `cap` entries
    # each, 0: not wanted; d_out_packed is required.
    def filter_cross_cols_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                                 d_out_col_off: int, d_out_n: int, cap: int, d_out_packed: int, d_out_ids: int = 0,
                                 d_out_row: int = 0, d_out_perm: int = 0, d_out_col_n: int = 0,
                                 select: int = SELECT_LOOKUP, col_limit: int = 0, d_out_errs: int = 0, err_cap: int = 0,
                                 d_out_n_errs: int = 0, stream: Optional[int] = None,
                                 requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                                 contexts: Optional[Sequence] = None) -> int:
        """gck_filter_cross_cols_device: check_cross_device, then for each resource the subjects whose
        Permissionship `select` (SELECT_*) names, in the subject list's order and at most `col_limit` of
        them (0: all): column offsets, ids, rows and Permissionships into the device arrays, their number
        into *d_out_n. A per-item error does not fail the call. Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectCols(select, col_limit, d_out_col_off or None, d_out_col_n or None, d_out_ids or None,
                         d_out_row or None, d_out_perm or None, cap, d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_filter_cross_cols_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                      n_subjects, d_resources or None, n_resources, *tail[:4],
                                                      C.byref(sel), *tail[4:], stream, C.byref(rev)))
        return rev.value

    def submit_filter_cross_cols_device(self, header, d_subjects: int, n_subjects: int, d_resources: int,
                                        n_resources: int, d_out_col_off: int, d_out_n: int, cap: int, d_out_packed: int,
                                        d_out_ids: int = 0, d_out_row: int = 0, d_out_perm: int = 0,
                                        d_out_col_n: int = 0, select: int = SELECT_LOOKUP, col_limit: int = 0,
                                        d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                                        stream: Optional[int] = None, engine_stream: bool = False,
                                        requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                                        contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_filter_submit_cross_cols_device (one device tile): as submit_cross_device, with
        filter_cross_cols_device's outputs."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectCols(select, col_limit, d_out_col_off or None, d_out_col_n or None, d_out_ids or None,
                         d_out_row or None, d_out_perm or None, cap, d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_filter_submit_cross_cols_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                             n_subjects, d_resources or None, n_resources, *tail[:4],
                                                             C.byref(sel), *tail[4:],
                                                             SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                             C.byref(b._h)))
        return b

    def prepare_filter_cross_cols_device(self, headers, subjects, n_subjects, resources, n_resources, col_off, out_n,
                                         cap: int, packed, depth: int, out_ids=None, out_row=None, out_perm=None,
                                         col_n=None, select: int = SELECT_LOOKUP, col_limit: int = 0, errs=None,
                                         err_cap: int = 0, n_errs=None, streams=None, engine_streams: bool = True,
                                         now_us: int = 0) -> "PreparedFilterCrossColsDevice":
        """The compiled loop over cross filter requests by resource (gckd_run_filter_cross_cols_device): as
        prepare_filter_cross_device, with request k's CSR into col_off[k] / out_ids[k] / out_row[k] /
        out_perm[k] (`cap` entries; None: not wanted), its columns' survivor counts into col_n[k] and the
        total into out_n[k], all under the one `select` and `col_limit`."""
        return PreparedFilterCrossColsDevice(self, headers, subjects, n_subjects, resources, n_resources, select,
                                             col_limit, col_off, col_n, out_ids, out_row, out_perm, cap, out_n, packed,
                                             errs, err_cap, depth, n_errs, streams, engine_streams, now_us)

    def filter_cross_cols_ids(self, header, subjects, resources, select: int = SELECT_LOOKUP, col_limit: int = 0,
                              want_row: bool = False, want_perm: bool = False,
                              requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                              contexts: Optional[Sequence] = None):
        """For each of `resources` the `subjects` that may see it — device int32 / uint32 tensors of ids —
        as a CSR of torch tensors: (col_off, ids), col_off an int32 [R + 1] tensor and ids (in the
        subjects' dtype) the kept survivors of resource r at col_off[r] .. col_off[r + 1], in the subject
        list's order; then their rows (int32) and Permissionships (uint8) when asked for. `col_limit`:
        at most so many per resource (0: all). Runs filter_cross_cols_device on the current stream with
        outputs allocated on the tensors' device (cap = R * (col_limit or S)) and reads the two count
        words — the call's only copy to the host. A per-item error raises GckError with the lookups'
        message."""
        import torch
        for name, t in (("subjects", subjects), ("resources", resources)):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               f"filter_cross_cols_ids: {name} must be a device int32 / uint32 tensor")
        if subjects.device != resources.device:
            raise GckError(GCK_E_INVALID_ARGUMENT, "filter_cross_cols_ids: the two lists are on different devices")
        subjects, resources = subjects.contiguous().reshape(-1), resources.contiguous().reshape(-1)
        S, R, dev = subjects.numel(), resources.numel(), subjects.device
        cap = R * (min(col_limit, S) if col_limit else S)
        with torch.cuda.device(dev):
            plane = torch.empty(max(1, S * ((R + 31) // 32)), dtype=torch.int64, device=dev)  # (required, also when empty)
            col_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [kept survivors, errors]
            out_ids = torch.empty(cap, dtype=subjects.dtype, device=dev)
            out_row = torch.empty(cap, dtype=torch.int32, device=dev) if want_row else None
            out_perm = torch.empty(cap, dtype=torch.uint8, device=dev) if want_perm else None
            err = torch.empty(2, dtype=torch.int32, device=dev)  # the first error record
            self.filter_cross_cols_device(header, subjects.data_ptr() if S * R else 0, S,
                                          resources.data_ptr() if S * R else 0, R, col_off.data_ptr(),
                                          counts.data_ptr(), cap, plane.data_ptr(),
                                          d_out_ids=out_ids.data_ptr() if cap else 0,
                                          d_out_row=out_row.data_ptr() if want_row and cap else 0,
                                          d_out_perm=out_perm.data_ptr() if want_perm and cap else 0, select=select,
                                          col_limit=col_limit, d_out_errs=err.data_ptr(), err_cap=1,
                                          d_out_n_errs=counts.data_ptr() + 4,
                                          stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                          revision=revision, now_us=now_us, contexts=contexts)
            total, n_errs = (int(x) & 0xFFFFFFFF for x in counts.tolist())
            if n_errs:
                code = int(err[1].item())
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               ITEM_ERROR_MESSAGES[ITEM_ERR_MAX_DEPTH] if code == ITEM_ERR_MAX_DEPTH
                               else f"lookup failed: per-item error {code}")
        out = (col_off, out_ids[:total])
        if want_row:
            out += (out_row[:total],)
        if want_perm:
            out += (out_perm[:total],)
        return out

    # ---- group filter requests (gck_filter_groups_device): a candidate list per owner, each owner's
    # survivors as a CSR. d_owners: S u32; d_group_off: S + 1 u32; d_candidates: n u32. d_out_row_off:
    # S + 1 u32 (required); d_out_n: one u32 (required); d_out_row_n: S u32, 0: not wanted; d_out_ids /
    # d_out_pos (u32) and d_out_perm (u8): `cap` entries each, 0: not wanted; d_out_packed (ceil(n / 32)
    # u64) is required.
    def filter_groups_device(self, header, d_owners: int, n_owners: int, d_group_off: int, d_candidates: int,
                             n_candidates: int, d_out_row_off: int, d_out_n: int, cap: int, d_out_packed: int,
                             d_out_ids: int = 0, d_out_pos: int = 0, d_out_perm: int = 0, d_out_row_n: int = 0,
                             vary: int = VARY_RESOURCE, select: int = SELECT_LOOKUP, group_limit: int = 0,
                             d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                             stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                             revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_filter_groups_device: check k is candidate k against the owner of the group it lies in
        (VARY_RESOURCE: owners are subject ids, candidates resource ids; VARY_SUBJECT: the mirror); then
        for each group the candidates whose Permissionship `select` (SELECT_*) names, in the group's
        order and at most `group_limit` of them (0: all): group offsets, ids, positions and
        Permissionships into the device arrays, their number into *d_out_n. A per-item error does not
        fail the call; malformed offsets do (GckError, InvalidArgument). Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectGroups(select, group_limit, d_out_row_off or None, d_out_row_n or None, d_out_ids or None,
                           d_out_pos or None, d_out_perm or None, cap, d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_filter_groups_device(self._h, C.byref(cs), C.byref(hdr), vary, d_owners or None, n_owners,
                                                  d_group_off or None, d_candidates or None, n_candidates, *tail[:4],
                                                  C.byref(sel), *tail[4:], stream, C.byref(rev)))
        return rev.value

    def submit_filter_groups_device(self, header, d_owners: int, n_owners: int, d_group_off: int, d_candidates: int,
                                    n_candidates: int, d_out_row_off: int, d_out_n: int, cap: int, d_out_packed: int,
                                    d_out_ids: int = 0, d_out_pos: int = 0, d_out_perm: int = 0, d_out_row_n: int = 0,
                                    vary: int = VARY_RESOURCE, select: int = SELECT_LOOKUP, group_limit: int = 0,
                                    d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                                    stream: Optional[int] = None, engine_stream: bool = False,
                                    requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                                    contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_filter_submit_groups_device (n_candidates <= max_batch): as submit_uniform_device, with
        filter_groups_device's outputs; malformed offsets fail the wait."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectGroups(select, group_limit, d_out_row_off or None, d_out_row_n or None, d_out_ids or None,
                           d_out_pos or None, d_out_perm or None, cap, d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_filter_submit_groups_device(self._h, C.byref(cs), C.byref(hdr), vary, d_owners or None,
                                                         n_owners, d_group_off or None, d_candidates or None,
                                                         n_candidates, *tail[:4], C.byref(sel), *tail[4:],
                                                         SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                         C.byref(b._h)))
        return b

    def filter_groups_ids(self, header, owners, offsets, candidates, vary: int = VARY_RESOURCE,
                          select: int = SELECT_LOOKUP, group_limit: int = 0, want_pos: bool = False,
                          want_perm: bool = False, requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                          now_us: int = 0, contexts: Optional[Sequence] = None):
        """For each of `owners` those of its own candidates that it may see (VARY_SUBJECT: that may see
        it) — device int32 / uint32 tensors: S owners, S + 1 offsets into the flat `candidates` — as a CSR
        of torch tensors: (row_off, ids), row_off an int32 [S + 1] tensor and ids (in the candidates'
        dtype) the kept survivors of owner s at row_off[s] .. row_off[s + 1], in its candidates' order;
        then their positions in `candidates` (int32) and Permissionships (uint8) when asked for.
        `group_limit`: at most so many per owner (0: all). Runs filter_groups_device on the current stream
        with outputs allocated on the tensors' device (cap = n, or S * group_limit when that is smaller)
        and reads the two count words — the call's only copy to the host. A per-item error raises
        GckError with the lookups' message."""
        import torch
        for name, t in (("owners", owners), ("offsets", offsets), ("candidates", candidates)):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, f"filter_groups_ids: {name} must be a device int32 / uint32 tensor")
        if owners.device != candidates.device or offsets.device != candidates.device:
            raise GckError(GCK_E_INVALID_ARGUMENT, "filter_groups_ids: the tensors are on different devices")
        owners, offsets, candidates = (t.contiguous().reshape(-1) for t in (owners, offsets, candidates))
        S, n, dev = owners.numel(), candidates.numel(), candidates.device
        if offsets.numel() != S + 1:
            raise GckError(GCK_E_INVALID_ARGUMENT, f"filter_groups_ids: {offsets.numel()} offsets for {S} owners")
        cap = min(n, S * group_limit) if group_limit else n
        with torch.cuda.device(dev):
            plane = torch.empty(max(1, (n + 31) // 32), dtype=torch.int64, device=dev)  # (required, also when empty)
            row_off = torch.empty(S + 1, dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [kept survivors, errors]
            out_ids = torch.empty(cap, dtype=candidates.dtype, device=dev)
            out_pos = torch.empty(cap, dtype=torch.int32, device=dev) if want_pos else None
            out_perm = torch.empty(cap, dtype=torch.uint8, device=dev) if want_perm else None
            err = torch.empty(2, dtype=torch.int32, device=dev)  # the first error record
            self.filter_groups_device(header, owners.data_ptr() if n else 0, S, offsets.data_ptr() if n else 0,
                                      candidates.data_ptr() if n else 0, n, row_off.data_ptr(), counts.data_ptr(), cap,
                                      plane.data_ptr(), d_out_ids=out_ids.data_ptr() if cap else 0,
                                      d_out_pos=out_pos.data_ptr() if want_pos and cap else 0,
                                      d_out_perm=out_perm.data_ptr() if want_perm and cap else 0, vary=vary,
                                      select=select, group_limit=group_limit, d_out_errs=err.data_ptr(), err_cap=1,
                                      d_out_n_errs=counts.data_ptr() + 4,
                                      stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                      revision=revision, now_us=now_us, contexts=contexts)
            total, n_errs = (int(x) & 0xFFFFFFFF for x in counts.tolist())
            if n_errs:
                code = int(err[1].item())
                raise GckError(GCK_E_INVALID_ARGUMENT,
                               ITEM_ERROR_MESSAGES[ITEM_ERR_MAX_DEPTH] if code == ITEM_ERR_MAX_DEPTH
                               else f"lookup failed: per-item error {code}")
        out = (row_off, out_ids[:total])
        if want_pos:
            out += (out_pos[:total],)
        if want_perm:
            out += (out_perm[:total],)
        return out

    # ---- recheck requests (gck_recheck_list_device, gck_recheck_cross_device): a list or cross device
    # request evaluated again and compared on the device with the caller's previous plane. d_prev_packed:
    # that plane (0: all zeros); d_out_packed: the new one (required; the next call's previous plane);
    # d_out_n: one u32 (required); the record arrays (u32, u32, u8 transition bytes): `cap` entries each,
    # 0: not wanted. `transitions`: CHANGE_*.
    def diff_planes_device(self, d_old: int, d_new: int, n: int, d_out_n: int, cap: int, d_ids: int = 0,
                           first_id: int = 0, d_out_ids: int = 0, d_out_pos: int = 0, d_out_trans: int = 0,
                           transitions: int = CHANGE_ANY, stream: Optional[int] = None) -> None:
        """gck_diff_planes_device: the changes between two dense planes of n checks the caller holds
        (d_old = 0: all zeros), in ascending position; synchronous on `stream`."""
        sel = SelectChanges(transitions, 0, d_out_ids or None, d_out_pos or None, d_out_trans or None, cap,
                            d_out_n or None)
        _check(self._lib.gck_diff_planes_device(self._h, d_old or None, d_new or None, n, d_ids or None, first_id,
                                                C.byref(sel), stream))

    def diff_cross_planes_device(self, d_old: int, d_new: int, n_subjects: int, n_resources: int, d_resources: int,
                                 d_out_row_off: int, d_out_n: int, cap: int, d_out_ids: int = 0, d_out_col: int = 0,
                                 d_out_trans: int = 0, transitions: int = CHANGE_ANY,
                                 stream: Optional[int] = None) -> None:
        """gck_diff_cross_planes_device: the changes between two cross planes of S x R checks, as a CSR
        by subject; synchronous on `stream`."""
        sel = SelectRowChanges(transitions, 0, d_out_row_off or None, d_out_ids or None, d_out_col or None,
                               d_out_trans or None, cap, d_out_n or None)
        _check(self._lib.gck_diff_cross_planes_device(self._h, d_old or None, d_new or None, n_subjects, n_resources,
                                                      d_resources or None, C.byref(sel), stream))

    def recheck_list_device(self, header, fixed_id: int, vary: int, n: int, d_prev_packed: int, d_out_packed: int,
                            d_out_n: int, cap: int, d_out_ids: int = 0, d_out_pos: int = 0, d_out_trans: int = 0,
                            transitions: int = CHANGE_ANY, d_ids: int = 0, first_id: int = 0, d_out_errs: int = 0,
                            err_cap: int = 0, d_out_n_errs: int = 0, stream: Optional[int] = None,
                            requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                            contexts: Optional[Sequence] = None) -> int:
        """gck_recheck_list_device: check_list_device into d_out_packed, then the checks whose value
        differs from d_prev_packed's by a selected transition: ids, positions and transition bytes into
        the device arrays, their number into *d_out_n. Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectChanges(transitions, 0, d_out_ids or None, d_out_pos or None, d_out_trans or None, cap,
                            d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_recheck_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary, d_ids or None,
                                                 first_id, n, *tail[:4], d_prev_packed or None, C.byref(sel), *tail[4:],
                                                 stream, C.byref(rev)))
        return rev.value

    def submit_recheck_list_device(self, header, fixed_id: int, vary: int, n: int, d_prev_packed: int,
                                   d_out_packed: int, d_out_n: int, cap: int, d_out_ids: int = 0, d_out_pos: int = 0,
                                   d_out_trans: int = 0, transitions: int = CHANGE_ANY, d_ids: int = 0,
                                   first_id: int = 0, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                                   stream: Optional[int] = None, engine_stream: bool = False,
                                   requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                                   contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_recheck_submit_list_device: as submit_list_device, with recheck_list_device's outputs."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectChanges(transitions, 0, d_out_ids or None, d_out_pos or None, d_out_trans or None, cap,
                            d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_recheck_submit_list_device(self._h, C.byref(cs), C.byref(hdr), fixed_id, vary,
                                                        d_ids or None, first_id, n, *tail[:4], d_prev_packed or None,
                                                        C.byref(sel), *tail[4:],
                                                        SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                        C.byref(b._h)))
        return b

    def recheck_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int, n_resources: int,
                             d_prev_packed: int, d_out_packed: int, d_out_row_off: int, d_out_n: int, cap: int,
                             d_out_ids: int = 0, d_out_col: int = 0, d_out_trans: int = 0,
                             transitions: int = CHANGE_ANY, d_out_errs: int = 0, err_cap: int = 0, d_out_n_errs: int = 0,
                             stream: Optional[int] = None, requirement: int = CONSISTENCY_MIN_LATENCY,
                             revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None) -> int:
        """gck_recheck_cross_device: check_cross_device into d_out_packed, then each subject's checks
        whose value differs from d_prev_packed's by a selected transition, as a CSR: row offsets, resource
        ids, columns and transition bytes, their number into *d_out_n. Returns the evaluated revision."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectRowChanges(transitions, 0, d_out_row_off or None, d_out_ids or None, d_out_col or None,
                               d_out_trans or None, cap, d_out_n or None)
        rev = C.c_uint64(0)
        _check(self._lib.gck_recheck_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None, n_subjects,
                                                  d_resources or None, n_resources, *tail[:4], d_prev_packed or None,
                                                  C.byref(sel), *tail[4:], stream, C.byref(rev)))
        return rev.value

    def submit_recheck_cross_device(self, header, d_subjects: int, n_subjects: int, d_resources: int,
                                    n_resources: int, d_prev_packed: int, d_out_packed: int, d_out_row_off: int,
                                    d_out_n: int, cap: int, d_out_ids: int = 0, d_out_col: int = 0,
                                    d_out_trans: int = 0, transitions: int = CHANGE_ANY, d_out_errs: int = 0,
                                    err_cap: int = 0, d_out_n_errs: int = 0, stream: Optional[int] = None,
                                    engine_stream: bool = False, requirement: int = CONSISTENCY_MIN_LATENCY,
                                    revision: int = 0, now_us: int = 0,
                                    contexts: Optional[Sequence] = None) -> "DeviceCompactBatch":
        """gck_recheck_submit_cross_device (one device tile): as submit_cross_device, with
        recheck_cross_device's outputs."""
        hdr = header if isinstance(header, Uniform) else _header(header)
        cs, tail = self._device_tail(requirement, revision, now_us, contexts, d_out_packed, d_out_errs, err_cap,
                                     d_out_n_errs)
        sel = SelectRowChanges(transitions, 0, d_out_row_off or None, d_out_ids or None, d_out_col or None,
                               d_out_trans or None, cap, d_out_n or None)
        b = DeviceCompactBatch(self, hdr)
        _check(self._lib.gck_recheck_submit_cross_device(self._h, C.byref(cs), C.byref(hdr), d_subjects or None,
                                                         n_subjects, d_resources or None, n_resources, *tail[:4],
                                                         d_prev_packed or None, C.byref(sel), *tail[4:],
                                                         SUBMIT_ENGINE_STREAM if engine_stream else 0, stream,
                                                         C.byref(b._h)))
        return b

    @staticmethod
    def _prev_plane(name, prev, words, dev):
        import torch
        if prev is None:
            return 0
        if prev.dtype != torch.int64 or prev.device != dev or prev.numel() != words or not prev.is_contiguous():
            raise GckError(GCK_E_INVALID_ARGUMENT, f"{name}: prev must be the contiguous int64 plane of {words} words "
                                                   "an earlier call of the same request returned")
        return prev.data_ptr() if words else 0

    def recheck_ids(self, header, fixed_id: int, vary: int, ids=None, first_id: int = 0, n: Optional[int] = None,
                    prev=None, transitions: int = CHANGE_ANY, requirement: int = CONSISTENCY_MIN_LATENCY,
                    revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None):
        """A list request evaluated now and compared with `prev`, the plane an earlier call of the same
        request returned (None: all zeros, so CHANGE_GAINED yields the initial grant set). `ids` is a
        device int32 / uint32 tensor of varying ids (None: the range first_id .. first_id + n - 1).
        Returns (plane, revision, ids, pos, trans): the new plane (int64 [ceil(n / 32)], the next call's
        `prev`), the evaluated revision, and the changed checks in ascending position — their ids (in
        the tensor's dtype), positions (int32) and transition bytes (uint8; change_split). Runs
        recheck_list_device on the current stream and reads back the two count words, the call's only
        copy to the host. A per-item error is no failure here: the check reads 0 in the plane, and 0
        is a legal end of a transition."""
        import torch
        if ids is not None:
            if ids.dtype not in (torch.int32, torch.uint32) or not ids.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, "recheck_ids: ids must be a device int32 / uint32 tensor")
            ids = ids.contiguous().reshape(-1)
            n, dev, dtype = ids.numel(), ids.device, ids.dtype
        else:
            if n is None:
                raise GckError(GCK_E_INVALID_ARGUMENT, "recheck_ids: a range needs n")
            dev, dtype = torch.device("cuda", self.device), torch.int32
        words = (n + 31) // 32
        d_prev = self._prev_plane("recheck_ids", prev, words, dev)
        with torch.cuda.device(dev):
            plane = torch.empty(max(1, words), dtype=torch.int64, device=dev)  # (required, also when empty)
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [changes, errors]
            out_ids = torch.empty(n, dtype=dtype, device=dev)
            out_pos = torch.empty(n, dtype=torch.int32, device=dev)
            out_trans = torch.empty(n, dtype=torch.uint8, device=dev)
            rev = self.recheck_list_device(header, fixed_id, vary, n, d_prev, plane.data_ptr(), counts.data_ptr(), n,
                                           d_out_ids=out_ids.data_ptr() if n else 0,
                                           d_out_pos=out_pos.data_ptr() if n else 0,
                                           d_out_trans=out_trans.data_ptr() if n else 0, transitions=transitions,
                                           d_ids=ids.data_ptr() if ids is not None and n else 0, first_id=first_id,
                                           d_out_n_errs=counts.data_ptr() + 4,
                                           stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                           revision=revision, now_us=now_us, contexts=contexts)
            total = int(counts[0].item()) & 0xFFFFFFFF
        return plane[:words], rev, out_ids[:total], out_pos[:total], out_trans[:total]

    def recheck_cross_ids(self, header, subjects, resources, prev=None, transitions: int = CHANGE_ANY,
                          requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                          contexts: Optional[Sequence] = None):
        """A cross request evaluated now and compared with `prev`, the plane an earlier call of the same
        request returned (None: all zeros). Returns (plane, revision, row_off, ids, col, trans): the new
        plane (int64 [S, ceil(R / 32)], check_cross_ids' layout and the next call's `prev`), the
        evaluated revision, and the changes as a CSR by subject — row_off an int32 [S + 1] tensor, and
        at row_off[s] .. row_off[s + 1] subject s's changed resources in list order: their ids (in the
        resources' dtype), columns (int32) and transition bytes (uint8; change_split). Runs
        recheck_cross_device on the current stream and reads back the two count words. A per-item error
        is no failure here: the check reads 0 in the plane."""
        import torch
        for name, t in (("subjects", subjects), ("resources", resources)):
            if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda:
                raise GckError(GCK_E_INVALID_ARGUMENT, f"recheck_cross_ids: {name} must be a device int32 / uint32 tensor")
        if subjects.device != resources.device:
            raise GckError(GCK_E_INVALID_ARGUMENT, "recheck_cross_ids: the two lists are on different devices")
        subjects, resources = subjects.contiguous().reshape(-1), resources.contiguous().reshape(-1)
        S, R, dev = subjects.numel(), resources.numel(), subjects.device
        stride = (R + 31) // 32
        d_prev = self._prev_plane("recheck_cross_ids", prev, S * stride, dev)
        cap = S * R
        with torch.cuda.device(dev):
            plane = torch.empty(max(1, S * stride), dtype=torch.int64, device=dev)  # (required, also when empty)
            row_off = torch.empty(S + 1, dtype=torch.int32, device=dev)
            counts = torch.empty(2, dtype=torch.int32, device=dev)  # [changes, errors]
            out_ids = torch.empty(cap, dtype=resources.dtype, device=dev)
            out_col = torch.empty(cap, dtype=torch.int32, device=dev)
            out_trans = torch.empty(cap, dtype=torch.uint8, device=dev)
            rev = self.recheck_cross_device(header, subjects.data_ptr() if cap else 0, S,
                                            resources.data_ptr() if cap else 0, R, d_prev, plane.data_ptr(),
                                            row_off.data_ptr(), counts.data_ptr(), cap,
                                            d_out_ids=out_ids.data_ptr() if cap else 0,
                                            d_out_col=out_col.data_ptr() if cap else 0,
                                            d_out_trans=out_trans.data_ptr() if cap else 0, transitions=transitions,
                                            d_out_n_errs=counts.data_ptr() + 4,
                                            stream=torch.cuda.current_stream(dev).cuda_stream, requirement=requirement,
                                            revision=revision, now_us=now_us, contexts=contexts)
            total = int(counts[0].item()) & 0xFFFFFFFF
        return plane[:S * stride].reshape(S, stride), rev, row_off, out_ids[:total], out_col[:total], out_trans[:total]

    def device_compact_stats(self) -> Tuple[int, int]:
        """gck_device_compact_stats: chunks of device requests whose join read and wrote the caller's
        device buffers in place, and chunks expanded to items on the device."""
        out = (C.c_uint64 * 2)()
        _check(self._lib.gck_device_compact_stats(self._h, out))
        return int(out[0]), int(out[1])

    def check_bulk_device(self, d_items: int, n: int, d_perm: int, d_err: int,
                          stream: Optional[int] = None, now_us: int = 0,
                          contexts: Optional[Sequence] = None):
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        _check(self._lib.gck_check_bulk_device_ctx(self._h, d_items, n, ctx_arr, ctx_lens, n_ctx, now_us,
                                                   d_perm, d_err, stream))

    def submit(self, items, n: Optional[int] = None, out_perm=None, out_err=None, requirement: int = CONSISTENCY_MIN_LATENCY,
               revision: int = 0, now_us: int = 0, contexts: Optional[Sequence] = None, device: bool = False,
               stream: Optional[int] = None, engine_stream: bool = False) -> "Batch":
        """Starts one batch (n <= max_batch) without waiting (gck_check_submit); Batch.wait()
        completes it. Host batches: `items` is an ITEM_DTYPE array and the results are returned by
        wait(). Device batches (device=True): `items`, `out_perm`, `out_err` are device pointers
        ordered on `stream`."""
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        h = _P()
        if device:
            flags = SUBMIT_DEVICE | (SUBMIT_ENGINE_STREAM if engine_stream else 0)
            _check(self._lib.gck_check_submit(self._h, C.byref(cs), items, n, ctx_arr, ctx_lens, n_ctx, now_us,
                                              out_perm, out_err, flags, stream, C.byref(h)))
            return Batch(self, h, None, None, None)
        items = np.ascontiguousarray(items, dtype=ITEM_DTYPE)
        n = len(items)
        perm = np.zeros(n, dtype=np.uint8)
        err = np.zeros(n, dtype=np.int32)
        _check(self._lib.gck_check_submit(self._h, C.byref(cs), items.ctypes.data if n else None, n, ctx_arr,
                                          ctx_lens, n_ctx, now_us, perm.ctypes.data if n else None,
                                          err.ctypes.data if n else None, 0, None, C.byref(h)))
        return Batch(self, h, perm, err, items)

    def host_array(self, n: int, dtype) -> np.ndarray:
        """A numpy array in pinned host memory (gck_host_alloc): host batches over such arrays
        are copied by DMA directly. The memory is returned (gck_host_free) when the array and
        every view of it are gone; the engine itself stays alive until then, even past close().
        A batch submitted over it reads the items by DMA until its wait (include/gck.h)."""
        if not self._h or self._closing:
            raise GckError(GCK_E_STATE, "engine closed")
        dtype = np.dtype(dtype)
        p = _P()
        _check(self._lib.gck_host_alloc(self._h, max(1, n * dtype.itemsize), C.byref(p)))
        buf = (C.c_char * max(1, n * dtype.itemsize)).from_address(p.value)
        self._pins += 1
        weakref.finalize(buf, self._unpin, p.value)  # numpy views keep `buf` alive
        return np.frombuffer(buf, dtype=dtype, count=n)

    def submit_into(self, items: np.ndarray, perm: np.ndarray, err: np.ndarray,
                    requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0, now_us: int = 0,
                    contexts: Optional[Sequence] = None) -> "Batch":
        """A host batch writing its results into caller-provided arrays (pinned ones from
        host_array() skip the engine's staging copies). Items in a host_array() buffer are read by
        DMA while the batch runs: leave them unchanged until wait() returns (include/gck.h
        gck_check_submit); other host items are staged before this returns."""
        cs = _Consistency(requirement, 0, revision)
        ctx_arr, ctx_lens, n_ctx = _context_arrays(contexts)
        h = _P()
        n = len(items)
        _check(self._lib.gck_check_submit(self._h, C.byref(cs), items.ctypes.data if n else None, n, ctx_arr,
                                          ctx_lens, n_ctx, now_us, perm.ctypes.data if n else None,
                                          err.ctypes.data if n else None, 0, None, C.byref(h)))
        return Batch(self, h, perm, err, items)

    def set_profile(self, on: bool):
        """GCK_FLAG_PROFILE for the batches submitted from now on (gck_set_profile)."""
        _check(self._lib.gck_set_profile(self._h, 1 if on else 0))

    def prepare_batches(self, items, perms, errs, n: int, depth: int, streams=None, engine_streams: bool = False,
                        now_us: int = 0, host: bool = False) -> "PreparedRun":
        """The arguments of one compiled submit/wait loop (libgck_driver.so), marshalled ahead, so
        that a timed region holds the C loop alone. host=True: items / perms / errs are host
        pointers (gck_host_alloc memory for DMA in place), batches on the engine's streams."""
        return PreparedRun(self, items, perms, errs, n, depth, streams, engine_streams, now_us, host)

    def run_device_batches(self, items, perms, errs, n: int, depth: int, streams, engine_streams: bool = False,
                           now_us: int = 0) -> float:
        """Checks len(items) device batches of n items each (device pointers items[k], perms[k],
        errs[k]) with up to `depth` in flight, batch k on streams[k % depth] (engine_streams: on
        the engine's workspace streams, GCK_SUBMIT_ENGINE_STREAM), through the compiled
        submit/wait loop of libgck_driver.so (the loop a cgo caller runs; no Python per batch).
        Returns the loop's wall time in seconds."""
        drv = _driver()
        k = len(items)
        arr = lambda xs: (C.c_uint64 * max(1, len(xs)))(*[int(x) for x in xs])
        cs = _Consistency(CONSISTENCY_MIN_LATENCY, 0, 0)
        secs = C.c_double(0.0)
        submit = C.cast(self._lib.gck_check_submit, C.c_void_p)
        wait = C.cast(self._lib.gck_check_wait, C.c_void_p)
        _check(drv.gckd_run(submit, wait, self._h, C.byref(cs), k, arr(items), arr(perms), arr(errs), n, depth,
                            arr(streams), SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us, C.byref(secs)))
        return secs.value

    # ---- lookups (Client.LookupResources / LookupSubjects, client/client.go:508-599) --------
    def _lookup(self, fn, args, requirement, revision):
        cs = _Consistency(requirement, 0, revision)
        n = C.c_size_t(0)
        cap = 1024
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            perms = np.zeros(cap, dtype=np.uint8)
            rc = fn(self._h, C.byref(cs), *args, ids.ctypes.data, perms.ctypes.data, cap, C.byref(n))
            if rc == GCK_E_CAPACITY and n.value > cap:
                cap = n.value  # the engine kept the result: the retry copies it out
                continue
            _check(rc)
            return ids[: n.value], perms[: n.value]

    def lookup_resources(self, resource_type: int, permission: int, subject_type: int, subject_relation: int,
                         subject_id: int, requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                         now_us: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Ids (ascending) of the resource_type objects the subject has `permission` on, and
        their permissionship (PERM_HAS / PERM_CONDITIONAL)."""
        # an explicit evaluation time, so that a capacity retry is served from the engine's cache
        now_us = now_us or time.time_ns() // 1000
        return self._lookup(self._lib.gck_lookup_resources,
                            (resource_type, permission, subject_type, subject_relation, subject_id, now_us),
                            requirement, revision)

    def lookup_subjects(self, resource_type: int, resource_id: int, permission: int, subject_type: int,
                        subject_relation: int = ELLIPSIS, requirement: int = CONSISTENCY_MIN_LATENCY,
                        revision: int = 0, now_us: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Ids (ascending) of the subject_type subjects that have `permission` on the resource;
        a wildcard grant is one id, ID_WILDCARD (last), instead of every subject of the type."""
        now_us = now_us or time.time_ns() // 1000
        return self._lookup(self._lib.gck_lookup_subjects,
                            (resource_type, resource_id, permission, subject_type, subject_relation, now_us),
                            requirement, revision)

    def lookup_resources_among(self, resource_type: int, permission: int, subject_type: int, subject_relation: int,
                               subject_id: int, candidates: Optional[np.ndarray] = None,
                               requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                               now_us: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """gck_lookup_resources_among: of the candidate resource ids, those the subject has
        `permission` on — in the candidates' order, repeats included — and their permissionship.
        candidates=None: every object of the type (lookup_resources' answer)."""
        now_us = now_us or time.time_ns() // 1000
        cand = None if candidates is None else np.ascontiguousarray(candidates, dtype=np.uint32).reshape(-1)
        if cand is not None and len(cand) == 0:  # (nothing to ask: a null list would mean the whole type)
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
        return self._lookup(self._lib.gck_lookup_resources_among,
                            (resource_type, permission, subject_type, subject_relation, subject_id,
                             None if cand is None else cand.ctypes.data, 0 if cand is None else len(cand), now_us),
                            requirement, revision)

    def lookup_subjects_among(self, resource_type: int, resource_id: int, permission: int, subject_type: int,
                              candidates: np.ndarray, subject_relation: int = ELLIPSIS,
                              requirement: int = CONSISTENCY_MIN_LATENCY, revision: int = 0,
                              now_us: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """gck_lookup_subjects_among: of the candidate subject ids, those that have `permission` on
        the resource, in the candidates' order; a wildcard grant makes every candidate match (no
        ID_WILDCARD entry)."""
        now_us = now_us or time.time_ns() // 1000
        cand = np.ascontiguousarray(candidates, dtype=np.uint32).reshape(-1)
        if len(cand) == 0:
            return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
        return self._lookup(self._lib.gck_lookup_subjects_among,
                            (resource_type, resource_id, permission, subject_type, subject_relation,
                             cand.ctypes.data, len(cand), now_us), requirement, revision)

    # ---- partitioned graphs (gck_part_*; driven by gochugaru_amd.partition) -----------------
    def set_partition(self, rank: int, world: int):
        _check(self._lib.gck_set_partition(self._h, rank, world))
        self.part_rank, self.part_world = rank, world

    @staticmethod
    def part_unique_id() -> bytes:
        """gck_part_unique_id: the RCCL communicator id rank 0 hands to every rank."""
        buf = (C.c_uint8 * PART_UNIQUE_ID_BYTES)()
        _check(load_library().gck_part_unique_id(buf))
        return bytes(buf)

    def part_init(self, unique_id: bytes):
        """gck_part_init: join the RCCL communicator of the partition (every rank, same id)."""
        assert len(unique_id) == PART_UNIQUE_ID_BYTES
        buf = (C.c_uint8 * PART_UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._lib.gck_part_init(self._h, buf))

    def part_intern(self, transport: "Transport", type_ids, names, create: bool = False) -> np.ndarray:
        """gck_part_intern_with (collective): the ids every rank agrees on for (type, name) pairs,
        each interned by its owner rank (hash of the name)."""
        n = len(names)
        raw = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
        types = np.ascontiguousarray(type_ids, dtype=np.uint16)
        lens = np.array([len(b) for b in raw], dtype=np.uint32)
        bufs = [C.create_string_buffer(b, len(b) + 1) for b in raw]
        ptrs = (C.c_char_p * max(1, n))(*[C.cast(b, C.c_char_p) for b in bufs])
        out = np.zeros(n, dtype=np.uint32)
        _check(self._lib.gck_part_intern_with(self._h, C.byref(transport), types.ctypes.data if n else None,
                                              C.cast(ptrs, C.c_void_p) if n else None,
                                              lens.ctypes.data if n else None, n, INTERN_CREATE if create else 0,
                                              out.ctypes.data if n else None))
        return out

    def interned_names(self, type_id: int) -> int:
        """Names the interner holds for a type (gck_interned_names)."""
        v = C.c_uint32(0)
        _check(self._lib.gck_interned_names(self._h, type_id, C.byref(v)))
        return v.value

    def part_add_tuples_text(self, transport: "Transport", text: str):
        """gck_part_add_tuples_text_with (collective): the export stream's text, the same on every
        rank; each keeps and interns what it owns."""
        b = text.encode()
        _check(self._lib.gck_part_add_tuples_text_with(self._h, C.byref(transport), b, len(b)))

    def part_load_snapshot_text(self, transport: "Transport", revision: int, text: str):
        self.begin_snapshot(revision)
        self.part_add_tuples_text(transport, text)
        self.commit_snapshot()

    def part_make_items(self, transport: "Transport", rels: Iterable) -> np.ndarray:
        """make_items on a partitioned engine (collective): the names resolved by their owners,
        so that every rank builds the same items."""
        rels = list(rels)
        items = np.zeros(len(rels), dtype=ITEM_DTYPE)
        types, names, where = [], [], []
        for i, r in enumerate(rels):
            rt = self.type_id(r.ResourceType)
            st = self.type_id(r.SubjectType)
            items[i]["resource_type"] = rt
            items[i]["permission"] = self.relation_id(rt, r.ResourceRelation)
            items[i]["subject_type"] = st
            items[i]["subject_relation"] = (ELLIPSIS if r.SubjectRelation in ("", "...")
                                            else self.relation_id(st, r.SubjectRelation))
            items[i]["resource_id"] = ID_ABSENT
            items[i]["subject_id"] = ID_WILDCARD if (st == TYPE_INVALID and r.SubjectID == "*") else ID_ABSENT
            if rt != TYPE_INVALID:
                types.append(rt), names.append(r.ResourceID), where.append((i, "resource_id"))
            if st != TYPE_INVALID:
                types.append(st), names.append(r.SubjectID), where.append((i, "subject_id"))
        ids = self.part_intern(transport, types, names, create=False)
        for (i, f), v in zip(where, ids):
            items[i][f] = v
        return items

    def part_check(self, d_items: int, n: int, d_perm: int, d_err: int, now_us: int = 0,
                   stream: Optional[int] = None):
        """gck_part_check: the whole partitioned check, exchanged over RCCL inside libgck."""
        _check(self._lib.gck_part_check(self._h, d_items, n, now_us, d_perm, d_err, stream))

    def part_check_with(self, transport: "Transport", d_items: int, n: int, d_perm: int, d_err: int, now_us: int = 0,
                        stream: Optional[int] = None):
        """gck_part_check_with: the partitioned check over the caller's transport (a
        gochugaru_amd.partition transport: gck_transport's callbacks)."""
        _check(self._lib.gck_part_check_with(self._h, C.byref(transport), d_items, n, now_us, d_perm, d_err, stream))

    def stats(self) -> Stats:
        s = _Stats()
        _check(self._lib.gck_last_stats(self._h, C.byref(s)))
        return Stats({k: getattr(s, k) for k, _ in _Stats._fields_})

    def reset_stats(self):
        _check(self._lib.gck_reset_stats(self._h))

    # ---- string-level convenience --------------------------------------------------------
    def make_request(self, rels: Iterable) -> Tuple[np.ndarray, List[str]]:
        """Items plus their check-time caveat contexts, as Client.Check builds them
        (client/client.go:244-258: Context = MustV1ProtoCaveat().GetContext(), i.e. the
        relationship's caveat context when it names a caveat). Identical contexts share a slot."""
        rels = list(rels)
        items = self.make_items(rels)
        contexts: List[str] = []
        slots = {}
        for i, r in enumerate(rels):
            ctx = r.MustV1ProtoCaveatContext() if hasattr(r, "MustV1ProtoCaveatContext") else None
            if ctx is None:
                continue
            js = _context_json(ctx)
            k = slots.get(js)
            if k is None:
                contexts.append(js)
                k = slots[js] = len(contexts)
            items[i]["context_slot"] = k
        return items, contexts

    def make_items(self, rels: Iterable) -> np.ndarray:
        """rel.Relationship-like items -> interned gck_item array (unknown names map to
        invalid ids so the device reports the per-item error; unknown ids map to ABSENT)."""
        rels = list(rels)
        items = np.zeros(len(rels), dtype=ITEM_DTYPE)
        by_type = {}
        for i, r in enumerate(rels):
            rt = self.type_id(r.ResourceType)
            st = self.type_id(r.SubjectType)
            items[i]["resource_type"] = rt
            items[i]["permission"] = self.relation_id(rt, r.ResourceRelation)
            items[i]["subject_type"] = st
            items[i]["subject_relation"] = (ELLIPSIS if r.SubjectRelation in ("", "...")
                                            else self.relation_id(st, r.SubjectRelation))
            if rt != TYPE_INVALID:
                by_type.setdefault(rt, ([], []))[0].append(i)
            if st != TYPE_INVALID:
                by_type.setdefault(st, ([], []))[1].append(i)
        for t, (ri, si) in by_type.items():
            if ri:
                items["resource_id"][ri] = self.intern(t, [rels[i].ResourceID for i in ri])
            if si:
                items["subject_id"][si] = self.intern(t, [rels[i].SubjectID for i in si])
        for i, r in enumerate(rels):
            if items[i]["resource_type"] == TYPE_INVALID:
                items[i]["resource_id"] = ID_ABSENT
            if items[i]["subject_type"] == TYPE_INVALID:
                items[i]["subject_id"] = ID_WILDCARD if r.SubjectID == "*" else ID_ABSENT
        return items


class _Prepared:
    """What the compiled submit/wait loops of libgck_driver.so share: `k` batches through `loop`
    (a gckd_run* function) and the engine's `submit` entry point, `depth` in flight; the
    subclass's self._args are the loop's own arguments, marshalled ahead."""

    def __init__(self, engine, loop: str, submit: str, k: int, depth: int):
        self._e, self._k, self._depth = engine, k, depth
        self._cs = _Consistency(CONSISTENCY_MIN_LATENCY, 0, 0)
        self._drv = _driver()
        self._loop = getattr(self._drv, loop)
        self._submit = C.cast(getattr(engine._lib, submit), C.c_void_p)
        self._wait = C.cast(engine._lib.gck_check_wait, C.c_void_p)
        self._secs = C.c_double(0.0)
        self.n_errs = (C.c_size_t * max(1, k))()  # per request (the compact loops)
        self._args = ()

    @staticmethod
    def _arr(xs):
        return (C.c_uint64 * max(1, len(xs)))(*[int(x) for x in xs])

    def run(self) -> float:
        """Runs the loop; returns its wall time in seconds (first submit to last wait)."""
        _check(self._loop(self._submit, self._wait, self._e._h, C.byref(self._cs), self._k, *self._args,
                          C.byref(self._secs)))
        return self._secs.value


class PreparedRun(_Prepared):
    """A compiled submit/wait loop with its argument arrays built (Engine.prepare_batches)."""

    def __init__(self, engine, items, perms, errs, n, depth, streams, engine_streams, now_us, host):
        super().__init__(engine, "gckd_run_host" if host else "gckd_run", "gck_check_submit", len(items), depth)
        arr = self._arr
        self._args = (arr(items), arr(perms), arr(errs), n, depth)
        if not host:
            self._args += (arr(streams or [0]), SUBMIT_ENGINE_STREAM if engine_streams else 0)
        self._args += (now_us,)


class PreparedUniform(_Prepared):
    """A compiled submit/wait loop over uniform requests with its argument arrays built
    (Engine.prepare_uniform)."""

    def __init__(self, engine, headers, pairs, ns, packed, errs, err_cap, depth, now_us):
        super().__init__(engine, "gckd_run_uniform", "gck_check_submit_uniform", len(pairs), depth)
        arr = self._arr
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(pairs), arr(ns), arr(packed), arr(errs), err_cap, self.n_errs, depth, now_us)


class PreparedShaped(_Prepared):
    """A compiled submit/wait loop over shaped requests with its argument arrays built
    (Engine.prepare_shaped)."""

    def __init__(self, engine, shapes, shape_of, pairs, ns, packed, errs, err_cap, depth, now_us):
        super().__init__(engine, "gckd_run_shaped", "gck_check_submit_shaped", len(pairs), depth)
        arr = self._arr
        self._tables = [_shape_table(t) for t in shapes]  # (kept alive: the loop reads their addresses)
        self._args = (arr([C.addressof(t) for t, _ in self._tables]), arr([m for _, m in self._tables]),
                      arr(shape_of), arr(pairs), arr(ns), arr(packed), arr(errs), err_cap, self.n_errs, depth, now_us)


class PreparedCross(_Prepared):
    """A compiled submit/wait loop over cross requests with its argument arrays built
    (Engine.prepare_cross)."""

    def __init__(self, engine, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap, depth,
                 now_us):
        super().__init__(engine, "gckd_run_cross", "gck_check_submit_cross", len(subjects), depth)
        arr = self._arr
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(subjects), arr(n_subjects), arr(resources), arr(n_resources), arr(packed), arr(errs),
                      err_cap, self.n_errs, depth, now_us)


class PreparedList(_Prepared):
    """A compiled submit/wait loop over list requests with its argument arrays built
    (Engine.prepare_list)."""

    def __init__(self, engine, headers, fixed, vary, ids, first, ns, packed, errs, err_cap, depth, now_us):
        super().__init__(engine, "gckd_run_list", "gck_check_submit_list", len(ns), depth)
        arr = self._arr
        u32 = lambda xs: (C.c_uint32 * max(1, len(xs)))(*[int(x) for x in xs])
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, u32(fixed), vary, arr(ids), u32(first), arr(ns), arr(packed), arr(errs), err_cap, self.n_errs,
                      depth, now_us)


class PreparedUniformDevice(_Prepared):
    """A compiled submit/wait loop over uniform device requests (Engine.prepare_uniform_device)."""

    def __init__(self, engine, headers, pairs, ns, packed, errs, err_cap, depth, n_errs, streams, engine_streams,
                 now_us):
        super().__init__(engine, "gckd_run_uniform_device", "gck_check_submit_uniform_device", len(pairs), depth)
        arr = self._arr
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(pairs), arr(ns), arr(packed), arr(errs), err_cap, arr(n_errs or [0] * len(pairs)), depth,
                      arr(streams or [0]), SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class PreparedListDevice(_Prepared):
    """A compiled submit/wait loop over list device requests (Engine.prepare_list_device)."""

    def __init__(self, engine, headers, fixed, vary, ids, first, ns, packed, errs, err_cap, depth, n_errs, streams,
                 engine_streams, now_us):
        super().__init__(engine, "gckd_run_list_device", "gck_check_submit_list_device", len(ns), depth)
        arr = self._arr
        u32 = lambda xs: (C.c_uint32 * max(1, len(xs)))(*[int(x) for x in xs])
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, u32(fixed), vary, arr(ids), u32(first), arr(ns), arr(packed), arr(errs), err_cap,
                      arr(n_errs or [0] * len(ns)), depth, arr(streams or [0]),
                      SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class PreparedCrossDevice(_Prepared):
    """A compiled submit/wait loop over cross device requests (Engine.prepare_cross_device)."""

    def __init__(self, engine, headers, subjects, n_subjects, resources, n_resources, packed, errs, err_cap, depth,
                 n_errs, streams, engine_streams, now_us):
        super().__init__(engine, "gckd_run_cross_device", "gck_check_submit_cross_device", len(subjects), depth)
        arr = self._arr
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(subjects), arr(n_subjects), arr(resources), arr(n_resources), arr(packed),
                      arr(errs or [0] * len(subjects)), err_cap, arr(n_errs or [0] * len(subjects)), depth,
                      arr(streams or [0]), SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class PreparedFilterDevice(_Prepared):
    """A compiled submit/wait loop over filter requests (Engine.prepare_filter_device)."""

    def __init__(self, engine, headers, fixed, vary, ids, first, ns, select, out_ids, out_pos, out_perm, cap, out_n,
                 packed, errs, err_cap, depth, n_errs, streams, engine_streams, now_us):
        super().__init__(engine, "gckd_run_filter_device", "gck_filter_submit_list_device", len(ns), depth)
        arr = self._arr
        u32 = lambda xs: (C.c_uint32 * max(1, len(xs)))(*[int(x) for x in xs])
        opt = lambda xs: arr(xs or [0] * len(ns))
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, u32(fixed), vary, arr(ids), u32(first), arr(ns), select, opt(out_ids), opt(out_pos),
                      opt(out_perm), cap, arr(out_n), opt(packed), opt(errs), err_cap, opt(n_errs), depth,
                      arr(streams or [0]), SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class PreparedFilterCrossDevice(_Prepared):
    """A compiled submit/wait loop over cross filter requests (Engine.prepare_filter_cross_device)."""

    def __init__(self, engine, headers, subjects, n_subjects, resources, n_resources, select, row_limit, row_off,
                 row_n, out_ids, out_col, out_perm, cap, out_n, packed, errs, err_cap, depth, n_errs, streams,
                 engine_streams, now_us):
        super().__init__(engine, "gckd_run_filter_cross_device", "gck_filter_submit_cross_device", len(subjects), depth)
        arr = self._arr
        opt = lambda xs: arr(xs or [0] * len(subjects))
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(subjects), arr(n_subjects), arr(resources), arr(n_resources), select, row_limit,
                      arr(row_off), opt(row_n), opt(out_ids), opt(out_col), opt(out_perm), cap, arr(out_n), arr(packed),
                      opt(errs), err_cap, opt(n_errs), depth, arr(streams or [0]),
                      SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class PreparedFilterCrossColsDevice(_Prepared):
    """A compiled submit/wait loop over cross filter requests by resource
    (Engine.prepare_filter_cross_cols_device)."""

    def __init__(self, engine, headers, subjects, n_subjects, resources, n_resources, select, col_limit, col_off,
                 col_n, out_ids, out_row, out_perm, cap, out_n, packed, errs, err_cap, depth, n_errs, streams,
                 engine_streams, now_us):
        super().__init__(engine, "gckd_run_filter_cross_cols_device", "gck_filter_submit_cross_cols_device",
                         len(subjects), depth)
        arr = self._arr
        opt = lambda xs: arr(xs or [0] * len(subjects))
        hdrs = (Uniform * max(1, len(headers)))(*[_header(h) for h in headers])
        self._args = (hdrs, arr(subjects), arr(n_subjects), arr(resources), arr(n_resources), select, col_limit,
                      arr(col_off), opt(col_n), opt(out_ids), opt(out_row), opt(out_perm), cap, arr(out_n), arr(packed),
                      opt(errs), err_cap, opt(n_errs), depth, arr(streams or [0]),
                      SUBMIT_ENGINE_STREAM if engine_streams else 0, now_us)


class DeviceCompactBatch:
    """A submitted compact request over device buffers (gck_check_submit_uniform_device ...): wait()
    completes it exactly once and returns the evaluated revision; the results are in the caller's
    device buffers. It keeps the header or shape table alive until the wait."""

    def __init__(self, engine, head):
        self._engine, self._head = engine, head
        self._h = _P()
        self.revision = None

    def wait(self):
        if self._h is not None and self._h.value is not None:
            h, self._h = self._h, None
            rev = C.c_uint64(0)
            _check(self._engine._lib.gck_check_wait_at(self._engine._h, h, C.byref(rev)))
            self.revision = rev.value
        return self.revision

    def __del__(self):
        try:
            self.wait()
        except Exception:
            pass


class Batch:
    """A submitted batch (gck_batch): wait() completes it exactly once."""

    def __init__(self, engine, handle, perm, err, items):
        self._engine, self._h = engine, handle
        self.perm, self.err = perm, err
        self._items = items  # host items stay alive until the wait (they are staged at submit anyway)
        self.revision = None  # the revision the batch ran on (gck_check_wait_at), after wait()

    def wait(self):
        if self._h is not None:
            h, self._h = self._h, None
            rev = C.c_uint64(0)
            _check(self._engine._lib.gck_check_wait_at(self._engine._h, h, C.byref(rev)))
            self.revision = rev.value
        return self.perm, self.err

    def __del__(self):
        try:
            self.wait()
        except Exception:
            pass


class UniformBatch:
    """A submitted uniform request (gck_check_submit_uniform): wait() completes it exactly once and
    returns (packed words, errors, evaluated revision)."""

    def __init__(self, engine, hdr, pairs, packed, errs):
        self._engine, self._hdr, self._pairs = engine, hdr, pairs
        self.packed, self.errs = packed, errs
        self._h = _P()
        self._n_errs = C.c_size_t(0)
        self.revision = None

    def wait(self):
        if self._h is not None and self._h.value is not None:
            h, self._h = self._h, None
            rev = C.c_uint64(0)
            _check(self._engine._lib.gck_check_wait_at(self._engine._h, h, C.byref(rev)))
            self.revision = rev.value
        m = min(self._n_errs.value, len(self.errs))
        return self.packed, self.errs[:m], self.revision

    def __del__(self):
        try:
            self.wait()
        except Exception:
            pass


class ShapedBatch(UniformBatch):
    """A submitted shaped request (gck_check_submit_shaped): as UniformBatch; it keeps the shape
    table and the index bytes alive until the wait."""


class CrossBatch(UniformBatch):
    """A submitted cross request (gck_check_submit_cross): as UniformBatch; `packed` is the
    row-padded plane (unpack_cross)."""


class ListBatch(UniformBatch):
    """A submitted list request (gck_check_submit_list): as UniformBatch; it keeps the id list alive
    until the wait."""


def _context_json(ctx) -> str:
    if ctx is None:
        return ""
    if isinstance(ctx, (str, bytes)):
        return ctx.decode() if isinstance(ctx, bytes) else ctx
    return json.dumps(ctx, sort_keys=True, separators=(",", ":"))


class Contexts:
    """Check-time caveat contexts marshalled once for the C ABI (the `contexts` / `context_lens`
    arrays of gck_check_bulk_ctx): pass it wherever `contexts` is taken to reuse the arrays
    across calls (a caller that builds its requests ahead, as a Go caller's slices are)."""

    def __init__(self, contexts):
        self._enc = [_context_json(c).encode() for c in contexts]
        self.arr = (C.c_char_p * len(self._enc))(*self._enc)
        self.lens = (C.c_size_t * len(self._enc))(*[len(b) for b in self._enc])

    def __len__(self):
        return len(self._enc)


def _context_arrays(contexts):
    if contexts is None or len(contexts) == 0:
        return None, None, 0
    if not isinstance(contexts, Contexts):
        contexts = Contexts(contexts)
    return contexts.arr, contexts.lens, len(contexts)


PART_UNIQUE_ID_BYTES = 128  # GCK_PART_UNIQUE_ID_BYTES


def partition_owner(object_id: int, world: int) -> int:
    return load_library().gck_partition_owner(object_id, world)


def partition_owner_name(type_id: int, name: str, world: int) -> int:
    """The rank that owns (and interns) the named object on a partitioned graph."""
    b = name.encode()
    return load_library().gck_partition_owner_name(type_id, b, len(b), world)
