"""The row-segmented selection over a cross plane (gochugaru_amd/csrc/select_plane.hpp: the per-word
functions k_dc_rows_count and k_dc_rows_write run, called here on the host through libgck.so's test
hook gck_test_select_rows, which walks rows and 64-word pieces as the kernels do) against numpy: row
lengths on both sides of every lane-group width and of the 64-word piece, row counts across a scan
tile, every mask, row limit and kind of cap, random and degenerate fills — offsets, unclipped row
counts and records compared exactly, nothing written beyond min(total, cap). The lane scans inside a
wave are the GPU tests' ground (tests/test_gpu_device_cross_filter.py). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests.test_select_plane import MASKS

RS = (1, 31, 32, 33, 64, 65, 200, 2047, 2049, 4097)
SMALL_R = (1, 31, 32, 33, 64, 65)  # S = 257 (across a 256-entry scan tile) stays well under a second here
SHAPES = [(S, R) for R in RS for S in (1, 2, 5)] + [(257, R) for R in SMALL_R]
P32, P8 = 0xDEADBEEF, 0xA5


@pytest.fixture(scope="module")
def hook():
    lib = E.load_library()
    fn = lib.gck_test_select_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def pack_rows(values):
    """An S x R array of 2-bit values as the row-padded plane: S rows of ceil(R / 32) u64 words,
    check r of a row in bits 2 (r % 32) .. of word r / 32, padding bits 0."""
    S, R = values.shape
    stride = (R + 31) // 32
    v = np.zeros((S, stride * 32), dtype=np.uint64)
    v[:, :R] = values
    v = v.reshape(S, stride, 32)
    return np.ascontiguousarray((v << (2 * np.arange(32, dtype=np.uint64))).sum(axis=2, dtype=np.uint64))


def fills(S, R, rng):
    last = np.zeros((S, R), dtype=np.uint8)
    last[-1, -1] = 2
    alt = np.fromfunction(lambda s, r: 1 + (s + r) % 2, (S, R)).astype(np.uint8)
    out = {"random": rng.integers(0, 4, (S, R)).astype(np.uint8), "zero": np.zeros((S, R), dtype=np.uint8),
           "alternating": alt, "last": last}
    for v in (1, 2, 3):
        out[f"all{v}"] = np.full((S, R), v, dtype=np.uint8)
    return out


def expect(values, src, mask, row_limit):
    """(row_off, row_n, ids, col, perm) of the whole selection, uncapped."""
    surv = ((mask >> values.astype(np.uint32)) & 1).astype(bool)
    row_n = surv.sum(axis=1).astype(np.uint32)
    kept = np.minimum(row_n, row_limit) if row_limit else row_n
    row_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint32)
    keep = surv & (np.cumsum(surv, axis=1) - 1 < kept[:, None])
    _, col = np.nonzero(keep)  # (row-major: ascending s, then ascending r)
    return row_off, row_n, src[col], col.astype(np.uint32), values[keep]


def run(hook, words, S, R, mask, row_limit, cap, src, want=("row_n", "ids", "col", "perm")):
    out = {"row_off": np.full(S + 3, P32, dtype=np.uint32), "row_n": np.full(S + 2, P32, dtype=np.uint32),
           "ids": np.full(cap + 2, P32, dtype=np.uint32), "col": np.full(cap + 2, P32, dtype=np.uint32),
           "perm": np.full(cap + 2, P8, dtype=np.uint8)}
    n = C.c_uint32(0x7777)
    ptr = lambda k: out[k].ctypes.data if k in want else None
    rc = hook(words.ctypes.data, S, R, mask, row_limit, cap, src.ctypes.data, out["row_off"].ctypes.data,
              ptr("row_n"), ptr("ids"), ptr("col"), ptr("perm"), C.byref(n))
    return rc, out, n.value


def check(out, n, S, cap, exp, want, where):
    row_off, row_n, ids, col, perm = exp
    total = int(row_off[-1])
    assert n == total, where
    assert np.array_equal(out["row_off"][:S + 1], row_off) and (out["row_off"][S + 1:] == P32).all(), where
    if "row_n" in want:
        assert np.array_equal(out["row_n"][:S], row_n) and (out["row_n"][S:] == P32).all(), where
    else:
        assert (out["row_n"] == P32).all(), where
    k = min(total, cap)
    for name, full, poison in (("ids", ids, P32), ("col", col, P32), ("perm", perm, P8)):
        if name in want:
            assert np.array_equal(out[name][:k], full[:k]) and (out[name][k:] == poison).all(), (where, name)
        else:
            assert (out[name] == poison).all(), (where, name)


@pytest.mark.parametrize("S,R", SHAPES)
def test_hook_matches_numpy(hook, S, R):
    rng = np.random.default_rng(S * 10007 + R)
    src = rng.integers(0, max(2, R // 2), R).astype(np.uint32)  # (repeated ids)
    want = ("row_n", "ids", "col", "perm")
    for name, values in fills(S, R, rng).items():
        words = pack_rows(values)
        assert words.shape == (S, (R + 31) // 32)
        for mask, row_limit in itertools.product(MASKS, (0, 1, 3, R, R + 1)):
            exp = expect(values, src, mask, row_limit)
            total = int(exp[0][-1])
            for cap in sorted({0, max(total - 1, 0), total, total + 5}):
                where = (name, mask, row_limit, cap)
                rc, out, n = run(hook, words, S, R, mask, row_limit, cap, src)
                assert rc == 0, where
                check(out, n, S, cap, exp, want, where)


def test_row_limit_clips_offsets_but_not_row_counts(hook):
    values = np.full((3, 70), 2, dtype=np.uint8)
    values[1, :68] = 1  # row 1: two survivors, at the end of its third word
    src = np.arange(100, 170, dtype=np.uint32)
    rc, out, n = run(hook, pack_rows(values), 3, 70, E.SELECT_LOOKUP, 3, 100, src)
    assert rc == 0 and n == 8
    assert out["row_off"][:4].tolist() == [0, 3, 5, 8] and out["row_n"][:3].tolist() == [70, 2, 70]
    assert out["col"][:8].tolist() == [0, 1, 2, 68, 69, 0, 1, 2]
    assert out["ids"][:8].tolist() == [100, 101, 102, 168, 169, 100, 101, 102]


@pytest.mark.parametrize("S,R", [(5, 65), (2, 2081)])
def test_each_output_may_be_null(hook, S, R):
    rng = np.random.default_rng(R)
    values = rng.integers(0, 4, (S, R)).astype(np.uint8)
    src = rng.integers(0, 1000, R).astype(np.uint32)
    words = pack_rows(values)
    names = ("row_n", "ids", "col", "perm")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            for row_limit in (0, 3):
                exp = expect(values, src, E.SELECT_LOOKUP, row_limit)
                total = int(exp[0][-1])
                records = [w for w in want if w != "row_n"]
                for cap in (0, total - 1, total + 5):
                    rc, out, n = run(hook, words, S, R, E.SELECT_LOOKUP, row_limit, cap, src, want)
                    if cap and not records:  # cap > 0 with all three record arrays NULL
                        assert rc == -1 and n == 0x7777, (want, cap)
                        assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in out), (want, cap)
                        continue
                    assert rc == 0, (want, cap)
                    check(out, n, S, cap, exp, want, (want, row_limit, cap))


def test_empty_requests(hook):
    src = np.zeros(1, dtype=np.uint32)
    words = np.zeros(1, dtype=np.uint64)
    # S == 0: row_off[0] and the count alone
    rc, out, n = run(hook, words, 0, 40, 4, 0, 4, src)
    assert rc == 0 and n == 0 and out["row_off"].tolist() == [0, P32, P32]
    assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in ("row_n", "ids", "col", "perm"))
    # R == 0: S + 1 zero offsets, S zero row counts, no plane read
    rc, out, n = run(hook, words, 3, 0, 4, 0, 4, src)
    assert rc == 0 and n == 0 and out["row_off"].tolist() == [0, 0, 0, 0, P32, P32]
    assert out["row_n"].tolist() == [0, 0, 0, P32, P32] and (out["ids"] == P32).all()
    rc, out, n = run(hook, words, 0, 0, 4, 0, 0, src)
    assert rc == 0 and n == 0 and out["row_off"].tolist() == [0, P32, P32]


def test_argument_errors(hook):
    values = np.random.default_rng(3).integers(0, 4, (2, 40)).astype(np.uint8)
    words, src = pack_rows(values), np.arange(40, dtype=np.uint32)
    row_off, ids = np.full(3, P32, dtype=np.uint32), np.full(16, P32, dtype=np.uint32)
    n = C.c_uint32(0x7777)
    good = [words.ctypes.data, 2, 40, E.SELECT_LOOKUP, 0, 8, src.ctypes.data, row_off.ctypes.data, None,
            ids.ctypes.data, None, None, C.byref(n)]
    assert hook(*good) == 0 and n.value != 0x7777
    row_off[:], ids[:], n.value = P32, P32, 0x7777

    def bad(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert hook(*args) == -1, changes
        assert (row_off == P32).all() and (ids == P32).all() and n.value == 0x7777, changes

    for mask in (0, 1, 3, 15, 16, 0x12):  # gck_select's rule
        bad(a3=mask)
    bad(a7=None)                          # null row_off
    bad(a12=None)                         # null count word
    bad(a9=None)                          # cap > 0 with all three record arrays null
    bad(a7=row_off.ctypes.data + 2)       # a u32 output that is not 4-byte aligned
    bad(a8=row_off.ctypes.data + 1)
    bad(a9=ids.ctypes.data + 2)
    bad(a10=ids.ctypes.data + 1)
    bad(a0=None)                          # a plane to read and none given
