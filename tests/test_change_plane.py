"""The dense selection over two planes (gochugaru_amd/csrc/select_plane.hpp: the per-word functions
k_dc_diff runs, called here on the host through libgck.so's test hook gck_test_change_plane, which
walks chunks and 256-word tiles as dc_diff_plane and the kernel's blocks do) against numpy: lengths on
both sides of a word and of a tile and across chunks, every single transition bit and the three named
sets, random and degenerate fills, garbage in the padding lanes of both planes, every kind of cap,
every subset of record arrays and a null old plane — records compared exactly, nothing written beyond
min(total, cap). The lane scan inside a wave is the GPU tests' ground
(tests/test_gpu_device_recheck.py). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E

SINGLE = [1 << (4 * v + w) for v in range(4) for w in range(4) if v != w]
TRANSITIONS = SINGLE + [E.CHANGE_GAINED, E.CHANGE_LOST, E.CHANGE_ANY]
# (n, chunk_words): a word's edges, a 256-word tile's edges inside one chunk, and lengths of several chunks
LENGTHS = [(1, 2048), (31, 2048), (32, 2048), (33, 2048), (8191, 2048), (8192, 2048), (8193, 2048),
           (300, 4), (2 * 300 * 32 - 7, 300), (97, 1)]
P32, P8 = 0xDEADBEEF, 0xA5


@pytest.fixture(scope="module")
def hook():
    lib = E.load_library()
    fn = lib.gck_test_change_plane
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def pack(values, rng=None):
    """n 2-bit values as the dense plane of ceil(n / 32) u64 words; the padding lanes of the last word
    0, or with `rng` random non-zero garbage."""
    n = len(values)
    words = (n + 31) // 32
    v = np.zeros(words * 32, dtype=np.uint64)
    v[:n] = values
    if rng is not None:
        v[n:] = rng.integers(1, 4, words * 32 - n)
    return np.ascontiguousarray((v.reshape(words, 32) << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64))


def expect(old, new, transitions, src, first_id=0):
    """(ids, pos, trans) of the whole diff, uncapped."""
    t = (4 * old.astype(np.uint32) + new).astype(np.uint32)
    pos = np.nonzero((old != new) & (((transitions >> t) & 1) == 1))[0].astype(np.uint32)
    ids = src[pos] if src is not None else (first_id + pos).astype(np.uint32)
    return ids, pos, t[pos].astype(np.uint8)


def fills(n, rng):
    old = rng.integers(0, 4, n).astype(np.uint8)
    last = old.copy()
    last[-1] = (last[-1] + 1) % 4
    return {"random": (old, rng.integers(0, 4, n).astype(np.uint8)), "identical": (old, old.copy()),
            "every": (old, ((old + rng.integers(1, 4, n)) % 4).astype(np.uint8)), "last": (old, last)}


def run(hook, old_w, new_w, n, transitions, chunk, cap, src, first_id=0, want=("ids", "pos", "trans")):
    out = {"ids": np.full(cap + 2, P32, dtype=np.uint32), "pos": np.full(cap + 2, P32, dtype=np.uint32),
           "trans": np.full(cap + 2, P8, dtype=np.uint8)}
    cnt = C.c_uint32(0x7777)
    ptr = lambda k: out[k].ctypes.data if k in want else None
    rc = hook(None if old_w is None else old_w.ctypes.data, new_w.ctypes.data, n, transitions, chunk, cap,
              None if src is None else src.ctypes.data, first_id, ptr("ids"), ptr("pos"), ptr("trans"), C.byref(cnt))
    return rc, out, cnt.value


def check(out, cnt, cap, exp, want, where):
    total = len(exp[1])
    assert cnt == total, where
    k = min(total, cap)
    for name, full, poison in (("ids", exp[0], P32), ("pos", exp[1], P32), ("trans", exp[2], P8)):
        if name in want:
            assert np.array_equal(out[name][:k], full[:k]) and (out[name][k:] == poison).all(), (where, name)
        else:
            assert (out[name] == poison).all(), (where, name)


@pytest.mark.parametrize("n,chunk", LENGTHS)
def test_hook_matches_numpy(hook, n, chunk):
    rng = np.random.default_rng(n * 31 + chunk)
    src = rng.integers(0, max(2, n // 2), n).astype(np.uint32)  # (repeated ids)
    want = ("ids", "pos", "trans")
    for name, (old, new) in fills(n, rng).items():
        for garbage in (False, True):
            old_w, new_w = pack(old, rng if garbage else None), pack(new, rng if garbage else None)
            for tr in TRANSITIONS:
                exp = expect(old, new, tr, src)
                total = len(exp[1])
                if name == "identical":
                    assert total == 0
                if name == "every" and tr == E.CHANGE_ANY:
                    assert total == n
                for cap in sorted({0, max(total - 1, 0), total + 2}):
                    where = (name, garbage, hex(tr), cap)
                    rc, out, cnt = run(hook, old_w, new_w, n, tr, chunk, cap, src)
                    assert rc == 0, where
                    check(out, cnt, cap, exp, want, where)


@pytest.mark.parametrize("n,chunk", [(33, 2048), (8193, 2048), (300, 4)])
def test_null_old_plane_reads_as_zeros_and_a_range_gives_ids(hook, n, chunk):
    rng = np.random.default_rng(n)
    new = rng.integers(0, 4, n).astype(np.uint8)
    new_w = pack(new, rng)
    for tr in (E.CHANGE_GAINED, E.CHANGE_ANY, 1 << 1, E.CHANGE_LOST):
        exp = expect(np.zeros(n, dtype=np.uint8), new, tr, None, first_id=1000)
        rc, out, cnt = run(hook, None, new_w, n, tr, chunk, n + 2, None, first_id=1000)
        assert rc == 0
        check(out, cnt, n + 2, exp, ("ids", "pos", "trans"), (n, hex(tr)))
    # GAINED against nothing: the initial grant set
    exp = expect(np.zeros(n, dtype=np.uint8), new, E.CHANGE_GAINED, None)
    assert np.array_equal(exp[1], np.nonzero(new >= 2)[0])


@pytest.mark.parametrize("n,chunk", [(65, 2048), (8193 + 40, 2048), (300, 4)])
def test_each_output_may_be_null(hook, n, chunk):
    rng = np.random.default_rng(n + 1)
    old, new = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)
    src = rng.integers(0, 1000, n).astype(np.uint32)
    old_w, new_w = pack(old), pack(new)
    exp = expect(old, new, E.CHANGE_ANY, src)
    total = len(exp[1])
    names = ("ids", "pos", "trans")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            for cap in (0, total - 1, total + 2):
                rc, out, cnt = run(hook, old_w, new_w, n, E.CHANGE_ANY, chunk, cap, src, want=want)
                if cap and not want:  # cap > 0 with all three record arrays NULL
                    assert rc == -1 and cnt == 0x7777, (want, cap)
                    assert all((out[k] == (P8 if k == "trans" else P32)).all() for k in out), (want, cap)
                    continue
                assert rc == 0, (want, cap)
                check(out, cnt, cap, exp, want, (want, cap))


def test_ranks_run_on_across_tiles_and_chunks(hook):
    # one change in the last word of a tile, one in the first word of the next, the same across a chunk edge
    n = 3 * 256 * 32
    old = np.ones(n, dtype=np.uint8)
    new = old.copy()
    marks = [256 * 32 - 1, 256 * 32, 2 * 256 * 32 - 1, 2 * 256 * 32]
    new[marks] = 2
    for chunk in (2048, 512, 256):
        rc, out, cnt = run(hook, pack(old), pack(new), n, E.CHANGE_GAINED, chunk, 8, None, first_id=7)
        assert rc == 0 and cnt == 4
        assert out["pos"][:4].tolist() == marks and out["ids"][:4].tolist() == [7 + m for m in marks]
        assert out["trans"][:4].tolist() == [4 * 1 + 2] * 4


def test_empty_request_writes_the_count_alone(hook):
    rc, out, cnt = run(hook, None, np.zeros(1, dtype=np.uint64), 0, E.CHANGE_ANY, 2048, 4, None)
    assert rc == 0 and cnt == 0
    assert all((out[k] == (P8 if k == "trans" else P32)).all() for k in out)


def test_argument_errors(hook):
    rng = np.random.default_rng(5)
    old_w, new_w = pack(rng.integers(0, 4, 70).astype(np.uint8)), pack(rng.integers(0, 4, 70).astype(np.uint8))
    ids = np.full(80, P32, dtype=np.uint32)
    cnt = C.c_uint32(0x7777)
    good = [old_w.ctypes.data, new_w.ctypes.data, 70, E.CHANGE_ANY, 2048, 72, None, 0, ids.ctypes.data, None, None,
            C.byref(cnt)]
    assert hook(*good) == 0 and cnt.value != 0x7777
    ids[:], cnt.value = P32, 0x7777

    def bad(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert hook(*args) == -1, changes
        assert (ids == P32).all() and cnt.value == 0x7777, changes

    for tr in (0, 1, 1 << 5, 1 << 10, 1 << 15, 0x8000, 0x10000, E.CHANGE_ANY | 1):  # a diagonal bit, or beyond the word
        bad(a3=tr)
    bad(a11=None)                       # null count word
    bad(a8=None)                        # cap > 0 with all three record arrays null
    bad(a8=ids.ctypes.data + 2)         # a u32 output that is not 4-byte aligned
    bad(a9=ids.ctypes.data + 1)
    bad(a0=old_w.ctypes.data + 4)       # a plane that is not 8-byte aligned
    bad(a1=None)                        # a new plane to read and none given
    bad(a0=new_w.ctypes.data)           # the old plane is the new one
    bad(a4=0)                           # no chunk
