"""Shaped requests without a GPU (include/gck.h gck_check_bulk_shaped): the driver library exports
its loop, the entry points validate the shape table on the host before anything else, and
shape_request turns items into (shapes, shape_of, pairs) and back exactly."""
import ctypes
import os

import numpy as np
import pytest

from gochugaru_amd import engine as E


@pytest.fixture()
def eng():
    e = E.Engine(device=0)
    yield e
    e.close()


def test_driver_library_exports_the_shaped_loop():
    path = os.path.join(os.path.dirname(E.__file__), "libgck_driver.so")
    assert hasattr(ctypes.CDLL(path), "gckd_run_shaped")


def test_shaped_entry_points_validate_the_table_without_a_snapshot(eng):
    pairs = np.zeros((4, 2), dtype=np.uint32)
    idx = np.zeros(4, dtype=np.uint8)
    plain = (0, 0, 0, E.ELLIPSIS)
    bad_tables = [
        [],                                   # n_shapes 0
        [plain] * 65,                         # n_shapes 65
        [plain, (0, 0, 0, E.ELLIPSIS, 2)],    # context_slot 2 with one context
        [plain, (0, 0, 0, E.ELLIPSIS, 0, 7)],  # reserved != 0
    ]
    for table in bad_tables:
        with pytest.raises(E.GckError) as ei:
            eng.check_shaped(table, idx, pairs, contexts=[{"a": 1}])
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, table
        words = np.zeros(1, dtype=np.uint64)
        errs = np.zeros(4, dtype=E.ITEM_ERROR_DTYPE)
        with pytest.raises(E.GckError) as ei:
            eng.submit_shaped(table, idx, pairs, words, errs, contexts=[{"a": 1}])
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, table
    eng.load_schema("definition user {}")
    # an empty request needs a snapshot like any check, as the uniform call (1 and 64 entries pass the table check)
    for table in ([plain], [plain] * 64):
        with pytest.raises(E.GckError) as ei:
            eng.check_shaped(table, np.zeros(0, dtype=np.uint8), np.zeros((0, 2), dtype=np.uint32))
        assert ei.value.code == E.GCK_E_STATE
    assert eng.shaped_stats() == (0, 0)


def _items(n_shapes, n, seed):
    """n items over n_shapes shapes; shape s first appears at position s (so first-seen order is
    the construction order), later positions draw shapes at random."""
    rng = np.random.default_rng(seed)
    shapes = []
    for s in range(n_shapes):  # distinct in every field combination, slot included
        shapes.append((s % 5, 100 + s // 5, 7 - s % 3, E.ELLIPSIS if s % 2 else 3 + s // 2, s % 4))
    assert len(set(shapes)) == n_shapes
    which = np.concatenate([np.arange(n_shapes), rng.integers(0, n_shapes, n - n_shapes)])
    items = np.zeros(n, dtype=E.ITEM_DTYPE)
    for k, s in enumerate(which):
        rt, p, st, sr, slot = shapes[s]
        items[k] = (rt, p, int(rng.integers(0, 2**32 - 1)), st, sr, int(rng.integers(0, 2**32 - 1)), slot)
    return shapes, which, items


@pytest.mark.parametrize("n_shapes", [1, 2, 64])
def test_shape_request_rebuilds_the_items(n_shapes):
    shapes, which, items = _items(n_shapes, 300, n_shapes)
    got = E.shape_request(items)
    assert got is not None
    g_shapes, shape_of, pairs = got
    assert g_shapes == shapes                      # first-seen order
    assert shape_of.dtype == np.uint8 and shape_of.tolist() == which.tolist()
    assert pairs.dtype == np.uint32 and pairs.shape == (300, 2)
    back = np.zeros(len(items), dtype=E.ITEM_DTYPE)
    for k in range(len(items)):
        rt, p, st, sr, slot = g_shapes[shape_of[k]]
        back[k] = (rt, p, pairs[k, 0], st, sr, pairs[k, 1], slot)
    assert back.tobytes() == items.tobytes()


def test_shape_request_gives_up_above_64_shapes():
    _, _, items = _items(65, 300, 65)
    assert E.shape_request(items) is None
    assert E.MAX_SHAPES == 64
