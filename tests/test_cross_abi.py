"""Cross requests without a GPU (include/gck.h gck_check_bulk_cross): the libraries export the
new entry points, the request errors are reported on the host before anything else, the tiling
rule gck_cross_tile keeps its invariants and its thin rule, and unpack_cross reads the row-padded
plane."""
import ctypes
import os

import numpy as np
import pytest

from gochugaru_amd import engine as E

S_SWEEP = [1, 2, 8, 9, 31, 32, 33, 64, 300, 5000]
R_SWEEP = [1, 31, 32, 33, 1000, 2047, 2048, 70000]
MB_SWEEP = [64, 256, 65536]


@pytest.fixture()
def eng():
    e = E.Engine(device=0)
    yield e
    e.close()


def test_libraries_export_the_cross_symbols():
    lib = E.load_library()
    for name in ("gck_check_bulk_cross", "gck_check_submit_cross", "gck_cross_stats", "gck_cross_tile"):
        assert hasattr(lib, name), name
    path = os.path.join(os.path.dirname(E.__file__), "libgck_driver.so")
    assert hasattr(ctypes.CDLL(path), "gckd_run_cross")
    assert E.CROSS_IDS == 2048


def test_cross_entry_points_report_request_errors_without_a_snapshot(eng):
    plain = (0, 0, 0, E.ELLIPSIS)
    ids = np.arange(4, dtype=np.uint32)
    words = np.zeros(4, dtype=np.uint64)
    errs = np.zeros(16, dtype=E.ITEM_ERROR_DTYPE)
    lib = eng._lib
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    n_errs = ctypes.c_size_t(0)
    rev = ctypes.c_uint64(0)

    def bulk(hdr, sub, S, res, R, out, n_ctx=0):
        return lib.gck_check_bulk_cross(eng._h, ctypes.byref(cs), ctypes.byref(hdr), sub, S, res, R, None, None, n_ctx,
                                        0, out, errs.ctypes.data, len(errs), ctypes.byref(n_errs), ctypes.byref(rev))

    def submit(hdr, sub, S, res, R, out):
        h = ctypes.c_void_p()
        rc = lib.gck_check_submit_cross(eng._h, ctypes.byref(cs), ctypes.byref(hdr), sub, S, res, R, None, None, 0, 0,
                                        out, errs.ctypes.data, len(errs), ctypes.byref(n_errs), ctypes.byref(h))
        assert h.value is None
        return rc

    ok = E.Uniform(*plain, 0, 0)
    p = ids.ctypes.data
    for call in (bulk, submit):
        # null buffers with S * R > 0
        assert call(ok, None, 4, p, 4, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
        assert call(ok, p, 4, None, 4, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
        assert call(ok, p, 4, p, 4, None) == E.GCK_E_INVALID_ARGUMENT
        # reserved != 0, a context slot above n_contexts
        assert call(E.Uniform(*plain, 0, 7), p, 4, p, 4, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
        assert call(E.Uniform(*plain, 1, 0), p, 4, p, 4, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
        # S * R >= 2^32 (checked before the buffers are looked at: they hold 4 ids)
        assert call(ok, p, 1 << 16, p, 1 << 16, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
        assert call(ok, p, 1 << 31, p, 2, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
    # the Python methods raise the same
    with pytest.raises(E.GckError) as ei:
        eng.check_cross(E.Uniform(*plain, 0, 7), ids, ids)
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    with pytest.raises(E.GckError) as ei:
        eng.check_cross((0, 0, 0, E.ELLIPSIS, 2), ids, ids, contexts=[{"a": 1}])
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    # a submit that is not one tile: more ids than the id block holds; a thin request
    big = np.zeros(3000, dtype=np.uint32)
    for S, R in ((1, 3000), (2047, 2), (300, 300)):
        assert E.cross_tile(S, R, 65536) != (S, R)
        assert submit(ok, big.ctypes.data, S, big.ctypes.data, R, words.ctypes.data) == E.GCK_E_INVALID_ARGUMENT
    # a valid request needs a snapshot like any check, an empty one included
    eng.load_schema("definition user {}")
    for S, R in ((4, 4), (0, 4), (4, 0), (0, 0)):
        with pytest.raises(E.GckError) as ei:
            eng.check_cross(plain, ids[:S], ids[:R])
        assert ei.value.code == E.GCK_E_STATE
    assert eng.cross_stats() == (0, 0)


def _tile_ok(S, R, mb, rows, cols):
    """The invariants a returned tile satisfies (include/gck.h gck_cross_tile)."""
    return (1 <= rows <= S and 1 <= cols <= R and rows * 32 * -(-cols // 32) <= mb and rows + cols <= E.CROSS_IDS
            and (cols % 32 == 0 or cols == R))


def _best_tile(S, R, mb):
    """The rule by exhaustion over every width: the most checks, the wider tile on a tie."""
    best = None
    for cols in range(1, min(R, E.CROSS_IDS - 1) + 1):
        if cols % 32 and cols != R:
            continue
        rows = min(S, mb // (32 * -(-cols // 32)), E.CROSS_IDS - cols)
        if rows >= 1 and (best is None or (rows * cols, cols) > (best[0] * best[1], best[1])):
            best = (rows, cols)
    return best


@pytest.mark.parametrize("mb", MB_SWEEP)
def test_cross_tile_invariants_and_thin_rule(mb):
    for S in S_SWEEP:
        for R in R_SWEEP:
            got = E.cross_tile(S, R, mb)
            best = _best_tile(S, R, mb)
            assert best is not None and _tile_ok(S, R, mb, *best), (S, R, mb, best)
            # 0 exactly on the thin rule: more checks than the best tile, which is below max_batch / 4
            thin = S * R > best[0] * best[1] and best[0] * best[1] < mb // 4
            assert (got is None) == thin, (S, R, mb, got, best)
            if got is None:
                continue
            rows, cols = got
            assert _tile_ok(S, R, mb, rows, cols), (S, R, mb, got)
            assert got == best, (S, R, mb, got, best)
            # the tiles cover the request: left to right and top to bottom, ragged last ones
            n_tiles = -(-S // rows) * -(-R // cols)
            assert n_tiles * rows * cols >= S * R
            covered = sum(min(rows, S - r0) * min(cols, R - c0) for r0 in range(0, S, rows) for c0 in range(0, R, cols))
            assert covered == S * R
            # every tile but the last of a band starts and ends on a word
            assert cols % 32 == 0 or cols == R


def test_cross_tile_named_cases():
    assert E.cross_tile(256, 256, 65536) == (256, 256)
    assert E.cross_tile(32, 2016, 65536) == (32, 2016)
    assert E.cross_tile(1, 1024, 65536) == (1, 1024)       # one tile: not thin, whatever its size
    assert E.cross_tile(1, 60000, 65536) is None            # thirty 2,016-check dispatches otherwise
    assert E.cross_tile(0, 5, 65536) is None and E.cross_tile(5, 0, 65536) is None
    assert E.cross_tile(5, 5, 16) is None                   # no 32-check wave fits max_batch
    assert E.cross_tile(10, 100, 256) == (4, 64)            # 8 x 32 holds as many checks: the wider one
    assert E.cross_tile(1, 500, 64) == (1, 64)              # a full batch per tile: not thin
    assert E.cross_tile(60, 3, 64) is None                  # 2 x 3 tiles: thin
    r, c = ctypes.c_uint32(9), ctypes.c_uint32(9)
    assert E.load_library().gck_cross_tile(1, 60000, 65536, ctypes.byref(r), ctypes.byref(c)) == 0
    assert (r.value, c.value) == (0, 0)


def _naive_unpack(words, S, R):
    stride = (R + 31) // 32
    out = np.zeros((S, R), dtype=np.uint8)
    for s in range(S):
        for r in range(R):
            out[s, r] = (int(words[s * stride + r // 32]) >> (2 * (r % 32))) & 3
    return out


@pytest.mark.parametrize("S,R", [(1, 1), (3, 31), (2, 32), (5, 33), (4, 65), (7, 100)])
def test_unpack_cross_matches_a_naive_loop(S, R):
    rng = np.random.default_rng(S * 1000 + R)
    stride = (R + 31) // 32
    words = rng.integers(0, 2**64 - 1, S * stride, dtype=np.uint64, endpoint=True)  # (padding bits random: ignored)
    got = E.unpack_cross(words, S, R)
    assert got.dtype == np.uint8 and got.shape == (S, R)
    assert np.array_equal(got, _naive_unpack(words, S, R))
