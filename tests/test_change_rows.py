"""The row form of the selection over two planes (gochugaru_amd/csrc/select_plane.hpp: the per-word
functions k_dc_diff_rows_count and k_dc_diff_rows_write run, called here on the host through libgck.so's
test hook gck_test_change_rows, which walks rows and 64-word pieces as the kernels do) against numpy:
row lengths on both sides of every lane-group width and of the 64-word piece, row counts across a scan
tile, every single transition bit and the three named sets, random and degenerate fills, garbage in
the padding lanes of both planes, every kind of cap, every subset of record arrays and a null old
plane — offsets and records compared exactly, nothing written beyond min(total, cap). The lane scans
inside a wave are the GPU tests' ground (tests/test_gpu_device_recheck.py). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests.test_change_plane import TRANSITIONS

RS = (1, 31, 32, 33, 64, 65, 2049)
SHAPES = [(S, R) for R in RS for S in (1, 2, 5, 257)]
P32, P8 = 0xDEADBEEF, 0xA5


@pytest.fixture(scope="module")
def hook():
    lib = E.load_library()
    fn = lib.gck_test_change_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def pack_rows(values, rng=None):
    """An S x R array of 2-bit values as the row-padded plane: S rows of ceil(R / 32) u64 words; the
    padding lanes of each row's last word 0, or with `rng` random non-zero garbage."""
    S, R = values.shape
    stride = (R + 31) // 32
    v = np.zeros((S, stride * 32), dtype=np.uint64)
    v[:, :R] = values
    if rng is not None:
        v[:, R:] = rng.integers(1, 4, (S, stride * 32 - R))
    v = v.reshape(S, stride, 32)
    return np.ascontiguousarray((v << (2 * np.arange(32, dtype=np.uint64))).sum(axis=2, dtype=np.uint64))


def expect(old, new, transitions, src):
    """(row_off, ids, col, trans) of the whole diff, uncapped."""
    t = (4 * old.astype(np.uint32) + new).astype(np.uint32)
    ch = (old != new) & (((transitions >> t) & 1) == 1)
    row_off = np.concatenate([[0], np.cumsum(ch.sum(axis=1))]).astype(np.uint32)
    _, col = np.nonzero(ch)  # (row-major: ascending s, then ascending r)
    return row_off, src[col], col.astype(np.uint32), t[ch].astype(np.uint8)


def fills(S, R, rng):
    old = rng.integers(0, 4, (S, R)).astype(np.uint8)
    last = old.copy()
    last[-1, -1] = (last[-1, -1] + 1) % 4
    return {"random": (old, rng.integers(0, 4, (S, R)).astype(np.uint8)), "identical": (old, old.copy()),
            "every": (old, ((old + rng.integers(1, 4, (S, R))) % 4).astype(np.uint8)), "last": (old, last)}


def run(hook, old_w, new_w, S, R, transitions, cap, src, want=("ids", "col", "trans")):
    out = {"row_off": np.full(S + 3, P32, dtype=np.uint32), "ids": np.full(cap + 2, P32, dtype=np.uint32),
           "col": np.full(cap + 2, P32, dtype=np.uint32), "trans": np.full(cap + 2, P8, dtype=np.uint8)}
    cnt = C.c_uint32(0x7777)
    ptr = lambda k: out[k].ctypes.data if k in want else None
    rc = hook(None if old_w is None else old_w.ctypes.data, new_w.ctypes.data, S, R, transitions, cap, src.ctypes.data,
              out["row_off"].ctypes.data, ptr("ids"), ptr("col"), ptr("trans"), C.byref(cnt))
    return rc, out, cnt.value


def check(out, cnt, S, cap, exp, want, where):
    row_off, ids, col, trans = exp
    total = int(row_off[-1])
    assert cnt == total, where
    assert np.array_equal(out["row_off"][:S + 1], row_off) and (out["row_off"][S + 1:] == P32).all(), where
    k = min(total, cap)
    for name, full, poison in (("ids", ids, P32), ("col", col, P32), ("trans", trans, P8)):
        if name in want:
            assert np.array_equal(out[name][:k], full[:k]) and (out[name][k:] == poison).all(), (where, name)
        else:
            assert (out[name] == poison).all(), (where, name)


@pytest.mark.parametrize("S,R", SHAPES)
def test_hook_matches_numpy(hook, S, R):
    rng = np.random.default_rng(S * 10007 + R)
    src = rng.integers(0, max(2, R // 2), R).astype(np.uint32)  # (repeated ids)
    want = ("ids", "col", "trans")
    for name, (old, new) in fills(S, R, rng).items():
        for garbage in (False, True):
            old_w, new_w = pack_rows(old, rng if garbage else None), pack_rows(new, rng if garbage else None)
            assert new_w.shape == (S, (R + 31) // 32)
            for tr in TRANSITIONS:
                exp = expect(old, new, tr, src)
                total = int(exp[0][-1])
                if name == "identical":
                    assert total == 0
                if name == "every" and tr == E.CHANGE_ANY:
                    assert total == S * R
                for cap in sorted({0, max(total - 1, 0), total + 2}):
                    where = (name, garbage, hex(tr), cap)
                    rc, out, cnt = run(hook, old_w, new_w, S, R, tr, cap, src)
                    assert rc == 0, where
                    check(out, cnt, S, cap, exp, want, where)


@pytest.mark.parametrize("S,R", [(5, 33), (2, 2049), (257, 31)])
def test_null_old_plane_reads_as_zeros(hook, S, R):
    rng = np.random.default_rng(S + R)
    new = rng.integers(0, 4, (S, R)).astype(np.uint8)
    src = np.arange(500, 500 + R, dtype=np.uint32)
    new_w = pack_rows(new, rng)
    for tr in (E.CHANGE_GAINED, E.CHANGE_ANY, 1 << 1, E.CHANGE_LOST):
        exp = expect(np.zeros((S, R), dtype=np.uint8), new, tr, src)
        rc, out, cnt = run(hook, None, new_w, S, R, tr, S * R + 2, src)
        assert rc == 0
        check(out, cnt, S, S * R + 2, exp, ("ids", "col", "trans"), (S, R, hex(tr)))


@pytest.mark.parametrize("S,R", [(5, 65), (2, 2081)])
def test_each_output_may_be_null(hook, S, R):
    rng = np.random.default_rng(R)
    old, new = rng.integers(0, 4, (S, R)).astype(np.uint8), rng.integers(0, 4, (S, R)).astype(np.uint8)
    src = rng.integers(0, 1000, R).astype(np.uint32)
    old_w, new_w = pack_rows(old), pack_rows(new)
    exp = expect(old, new, E.CHANGE_ANY, src)
    total = int(exp[0][-1])
    names = ("ids", "col", "trans")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            for cap in (0, total - 1, total + 2):
                rc, out, cnt = run(hook, old_w, new_w, S, R, E.CHANGE_ANY, cap, src, want)
                if cap and not want:  # cap > 0 with all three record arrays NULL
                    assert rc == -1 and cnt == 0x7777, (want, cap)
                    assert all((out[k] == (P8 if k == "trans" else P32)).all() for k in out), (want, cap)
                    continue
                assert rc == 0, (want, cap)
                check(out, cnt, S, cap, exp, want, (want, cap))


def test_empty_requests(hook):
    src = np.zeros(1, dtype=np.uint32)
    words = np.zeros(1, dtype=np.uint64)
    # S == 0: row_off[0] and the count alone
    rc, out, cnt = run(hook, None, words, 0, 40, E.CHANGE_ANY, 4, src)
    assert rc == 0 and cnt == 0 and out["row_off"].tolist() == [0, P32, P32]
    assert all((out[k] == (P8 if k == "trans" else P32)).all() for k in ("ids", "col", "trans"))
    # R == 0: S + 1 zero offsets, no plane read
    rc, out, cnt = run(hook, None, words, 3, 0, E.CHANGE_ANY, 4, src)
    assert rc == 0 and cnt == 0 and out["row_off"].tolist() == [0, 0, 0, 0, P32, P32]
    assert (out["ids"] == P32).all()
    rc, out, cnt = run(hook, None, words, 0, 0, E.CHANGE_ANY, 0, src)
    assert rc == 0 and cnt == 0 and out["row_off"].tolist() == [0, P32, P32]


def test_argument_errors(hook):
    rng = np.random.default_rng(3)
    old_w = pack_rows(rng.integers(0, 4, (2, 40)).astype(np.uint8))
    new_w = pack_rows(rng.integers(0, 4, (2, 40)).astype(np.uint8))
    src = np.arange(40, dtype=np.uint32)
    row_off, ids = np.full(3, P32, dtype=np.uint32), np.full(90, P32, dtype=np.uint32)
    cnt = C.c_uint32(0x7777)
    good = [old_w.ctypes.data, new_w.ctypes.data, 2, 40, E.CHANGE_ANY, 80, src.ctypes.data, row_off.ctypes.data,
            ids.ctypes.data, None, None, C.byref(cnt)]
    assert hook(*good) == 0 and cnt.value != 0x7777
    row_off[:], ids[:], cnt.value = P32, P32, 0x7777

    def bad(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert hook(*args) == -1, changes
        assert (row_off == P32).all() and (ids == P32).all() and cnt.value == 0x7777, changes

    for tr in (0, 1, 1 << 5, 1 << 10, 1 << 15, 0x8000, 0x10000, E.CHANGE_ANY | 1):
        bad(a4=tr)
    bad(a7=None)                          # null row_off
    bad(a11=None)                         # null count word
    bad(a8=None)                          # cap > 0 with all three record arrays null
    bad(a7=row_off.ctypes.data + 2)       # a u32 output that is not 4-byte aligned
    bad(a8=ids.ctypes.data + 2)
    bad(a9=ids.ctypes.data + 1)
    bad(a0=old_w.ctypes.data + 4)         # a plane that is not 8-byte aligned
    bad(a1=None)                          # a new plane to read and none given
    bad(a0=new_w.ctypes.data + 8)         # the old plane's range overlaps the new one's
    bad(a6=None)                          # ids wanted and no resource list
