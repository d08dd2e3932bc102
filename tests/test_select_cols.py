"""The column-segmented selection over a cross plane (gochugaru_amd/csrc/select_plane.hpp: the per-word
functions k_dc_cols_count and k_dc_cols_write run, called here on the host through libgck.so's test
hook gck_test_select_cols, which walks blocks of 64 columns, tiles of 2,048 rows, 16 chunks of a tile's
rows and batches of words as the kernels do) against numpy: the row test's selection
(tests/test_select_rows.py expect) applied to the transposed matrix is the expected CSR by resource.
Row counts on both sides of the 16 chunks, of a batch of 8 words and of a tile, column counts on both
sides of a plane word and of a block of 64 columns, every mask, column limit and kind of cap, random
and degenerate fills and one whose padding bits are garbage — offsets, unclipped column counts and
records compared exactly, nothing written beyond min(total, cap). The staging of a tile in LDS and the
barriers between a block's waves are the GPU tests' ground (tests/test_gpu_device_cross_cols.py). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests.test_select_plane import MASKS
from tests.test_select_rows import expect, fills, pack_rows

SS = (1, 2, 63, 64, 65, 129)
RS = (1, 31, 32, 33, 65, 200)
# besides the crossed shapes: a second block of 64 word-columns; S on both sides of the 16 chunks and
# of 16 chunks of one batch of 8 rows; R on both sides of a block of 64 columns and of two
SHAPES = ([(S, R) for S in SS for R in RS] + [(5, 2049), (70, 2081)]
          + [(S, 33) for S in (15, 16, 17, 127, 128, 144, 145)] + [(9, R) for R in (63, 64, 128, 129)]
          + [(2047, 3), (2048, 33), (2049, 3), (4100, 2)])  # on both sides of a tile of 2,048 rows, and a third tile
P32, P8 = 0xDEADBEEF, 0xA5
NAMES = ("col_n", "ids", "row", "perm")


@pytest.fixture(scope="module")
def hook():
    lib = E.load_library()
    fn = lib.gck_test_select_cols
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def garbage_padding(words, R, rng):
    """The plane with every padding bit of each row's last word set at random."""
    if R % 32 == 0:
        return words
    out = words.copy()
    keep = np.uint64((1 << (2 * (R % 32))) - 1)
    # (every padding field 1, 2 or 3 — a survivor of some mask, were it looked at: never 0)
    junk = rng.integers(0, 2 ** 63, out.shape[0], dtype=np.uint64) << np.uint64(1)
    junk = np.where(rng.integers(0, 2, out.shape[0]).astype(bool), junk | np.uint64(0x5555555555555555),
                    junk | np.uint64(0xAAAAAAAAAAAAAAAA))
    out[:, -1] = (out[:, -1] & keep) | (junk & ~keep)
    return out


def expect_cols(values, src, mask, col_limit):
    """(col_off, col_n, ids, row, perm): the row selection over the transposed matrix."""
    return expect(np.ascontiguousarray(values.T), src, mask, col_limit)


def run(hook, words, S, R, mask, col_limit, cap, src, want=NAMES):
    out = {"col_off": np.full(R + 3, P32, dtype=np.uint32), "col_n": np.full(R + 2, P32, dtype=np.uint32),
           "ids": np.full(cap + 2, P32, dtype=np.uint32), "row": np.full(cap + 2, P32, dtype=np.uint32),
           "perm": np.full(cap + 2, P8, dtype=np.uint8)}
    n = C.c_uint32(0x7777)
    ptr = lambda k: out[k].ctypes.data if k in want else None
    rc = hook(words.ctypes.data, S, R, mask, col_limit, cap, src.ctypes.data, out["col_off"].ctypes.data,
              ptr("col_n"), ptr("ids"), ptr("row"), ptr("perm"), C.byref(n))
    return rc, out, n.value


def check(out, n, R, cap, exp, want, where):
    col_off, col_n, ids, row, perm = exp
    total = int(col_off[-1])
    assert n == total, where
    assert np.array_equal(out["col_off"][:R + 1], col_off) and (out["col_off"][R + 1:] == P32).all(), where
    if "col_n" in want:
        assert np.array_equal(out["col_n"][:R], col_n) and (out["col_n"][R:] == P32).all(), where
    else:
        assert (out["col_n"] == P32).all(), where
    k = min(total, cap)
    for name, full, poison in (("ids", ids, P32), ("row", row, P32), ("perm", perm, P8)):
        if name in want:
            assert np.array_equal(out[name][:k], full[:k]) and (out[name][k:] == poison).all(), (where, name)
        else:
            assert (out[name] == poison).all(), (where, name)


@pytest.mark.parametrize("S,R", SHAPES)
def test_hook_matches_numpy(hook, S, R):
    rng = np.random.default_rng(S * 10007 + R)
    src = rng.integers(0, max(2, S // 2), S).astype(np.uint32)  # (repeated ids)
    planes = {name: (values, pack_rows(values)) for name, values in fills(S, R, rng).items()}
    values = rng.integers(0, 4, (S, R)).astype(np.uint8)
    planes["garbage-padding"] = (values, garbage_padding(pack_rows(values), R, rng))
    if R % 32:
        pad = E.unpack_cross(planes["garbage-padding"][1], S, 32 * ((R + 31) // 32))[:, R:]
        assert pad.all()  # the fill is what it says: every padding field holds a Permissionship
    for name, (values, words) in planes.items():
        assert words.shape == (S, (R + 31) // 32)
        for mask, col_limit in itertools.product(MASKS, (0, 1, 3, S, S + 1)):
            exp = expect_cols(values, src, mask, col_limit)
            total = int(exp[0][-1])
            for cap in sorted({0, max(total - 1, 0), total, total + 5}):
                where = (name, mask, col_limit, cap)
                rc, out, n = run(hook, words, S, R, mask, col_limit, cap, src)
                assert rc == 0, where
                check(out, n, R, cap, exp, NAMES, where)


def test_col_limit_clips_offsets_but_not_col_counts(hook):
    values = np.full((70, 3), 2, dtype=np.uint8)
    values[:68, 1] = 1  # column 1: two survivors, in the last chunk of rows
    src = np.arange(100, 170, dtype=np.uint32)
    rc, out, n = run(hook, pack_rows(values), 70, 3, E.SELECT_LOOKUP, 3, 100, src)
    assert rc == 0 and n == 8
    assert out["col_off"][:4].tolist() == [0, 3, 5, 8] and out["col_n"][:3].tolist() == [70, 2, 70]
    assert out["row"][:8].tolist() == [0, 1, 2, 68, 69, 0, 1, 2]
    assert out["ids"][:8].tolist() == [100, 101, 102, 168, 169, 100, 101, 102]


@pytest.mark.parametrize("S,R", [(65, 5), (2, 2081)])
def test_each_output_may_be_null(hook, S, R):
    rng = np.random.default_rng(R)
    values = rng.integers(0, 4, (S, R)).astype(np.uint8)
    src = rng.integers(0, 1000, S).astype(np.uint32)
    words = pack_rows(values)
    for r in range(len(NAMES) + 1):
        for want in itertools.combinations(NAMES, r):
            for col_limit in (0, 3):
                exp = expect_cols(values, src, E.SELECT_LOOKUP, col_limit)
                total = int(exp[0][-1])
                records = [w for w in want if w != "col_n"]
                for cap in (0, total - 1, total + 5):
                    rc, out, n = run(hook, words, S, R, E.SELECT_LOOKUP, col_limit, cap, src, want)
                    if cap and not records:  # cap > 0 with all three record arrays NULL
                        assert rc == -1 and n == 0x7777, (want, cap)
                        assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in out), (want, cap)
                        continue
                    assert rc == 0, (want, cap)
                    check(out, n, R, cap, exp, want, (want, col_limit, cap))


def test_empty_requests(hook):
    src = np.zeros(1, dtype=np.uint32)
    words = np.zeros(1, dtype=np.uint64)
    # R == 0: col_off[0] and the count alone
    rc, out, n = run(hook, words, 40, 0, 4, 0, 4, src)
    assert rc == 0 and n == 0 and out["col_off"].tolist() == [0, P32, P32]
    assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in NAMES)
    # S == 0: R + 1 zero offsets, R zero column counts, no plane read
    rc, out, n = run(hook, words, 0, 3, 4, 0, 4, src)
    assert rc == 0 and n == 0 and out["col_off"].tolist() == [0, 0, 0, 0, P32, P32]
    assert out["col_n"].tolist() == [0, 0, 0, P32, P32] and (out["ids"] == P32).all()
    rc, out, n = run(hook, words, 0, 0, 4, 0, 0, src)
    assert rc == 0 and n == 0 and out["col_off"].tolist() == [0, P32, P32]


def test_argument_errors(hook):
    values = np.random.default_rng(3).integers(0, 4, (40, 2)).astype(np.uint8)
    words, src = pack_rows(values), np.arange(40, dtype=np.uint32)
    col_off, ids = np.full(3, P32, dtype=np.uint32), np.full(16, P32, dtype=np.uint32)
    n = C.c_uint32(0x7777)
    good = [words.ctypes.data, 40, 2, E.SELECT_LOOKUP, 0, 8, src.ctypes.data, col_off.ctypes.data, None,
            ids.ctypes.data, None, None, C.byref(n)]
    assert hook(*good) == 0 and n.value != 0x7777
    col_off[:], ids[:], n.value = P32, P32, 0x7777

    def bad(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert hook(*args) == -1, changes
        assert (col_off == P32).all() and (ids == P32).all() and n.value == 0x7777, changes

    for mask in (0, 1, 3, 15, 16, 0x12):  # gck_select's rule
        bad(a3=mask)
    bad(a7=None)                          # null col_off
    bad(a12=None)                         # null count word
    bad(a9=None)                          # cap > 0 with all three record arrays null
    bad(a7=col_off.ctypes.data + 2)       # a u32 output that is not 4-byte aligned
    bad(a8=col_off.ctypes.data + 1)
    bad(a9=ids.ctypes.data + 2)
    bad(a10=ids.ctypes.data + 1)
    bad(a0=None)                          # a plane to read and none given
