"""The group-segmented selection over a dense plane (gochugaru_amd/csrc/select_plane.hpp: the group
lookup k_dc_group_pairs runs and the per-word functions k_dc_groups_count and k_dc_groups_write run,
called here on the host through libgck.so's test hooks gck_test_group_of and gck_test_select_groups,
which walk groups and pieces of L words as the kernels do) against numpy: group lengths on both sides
of a word, of every lane-group width and of 64 words, groups starting at every bit offset of a word,
several groups inside one word, empty groups in every place, group counts across a scan tile, every
mask, group limit and kind of cap, random and degenerate fills — offsets, unclipped group counts and
records compared exactly, nothing written beyond S + 1, S and min(total, cap). Malformed offsets keep
the lookup inside [0, S - 1] and the selection inside its arrays. The lane scans inside a wave are the
GPU tests' ground (tests/test_gpu_device_groups.py). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests.test_select_plane import MASKS

P32, P8 = 0xDEADBEEF, 0xA5
LENGTHS = (0, 1, 31, 32, 33, 64, 65, 2047, 2049, 4097)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uint32)


def offset_sets():
    """name -> group lengths. Every case the kernels' walk distinguishes."""
    rng = np.random.default_rng(7)
    sets = {}
    for S in (1, 2, 5):  # each length alone, doubled, and among four others (the third of five)
        for n in LENGTHS:
            sets[f"S{S}_len{n}"] = [n] * S if S < 5 else [3, 40, n, 0, 17]
    sets["all_lengths"] = list(LENGTHS)
    sets["every_bit_offset"] = [1] * 32 + [33] * 32          # 33-check groups begin at bits 0, 1, ... 31 of their word
    sets["every_bit_offset_long"] = sum(([k, 70] for k in range(1, 33)), [])
    sets["three_in_a_word"] = [5, 9, 7, 11, 3, 4, 25, 2, 2, 2]
    sets["empties"] = [0, 0, 5, 0, 0, 0, 40, 0, 33, 0, 0]    # leading, consecutive and trailing empty groups
    sets["only_empties"] = [0, 0, 0]
    sets["S257_short"] = rng.integers(0, 4, 257).tolist()     # across the 256-entry scan tile
    sets["S257_mixed"] = rng.integers(0, 70, 257).tolist()
    sets["one_long_among_short"] = [2] * 40 + [2100] + [3] * 40
    return sets


SETS = offset_sets()


@pytest.fixture(scope="module")
def hook():
    fn = E.load_library().gck_test_select_groups
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32,
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


@pytest.fixture(scope="module")
def group_of():
    fn = E.load_library().gck_test_group_of
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return fn


def pack_dense(values):
    """n 2-bit values as the dense plane: ceil(n / 32) u64 words (at least one), padding bits 0."""
    n = len(values)
    words = max(1, (n + 31) // 32)
    v = np.zeros(words * 32, dtype=np.uint64)
    v[:n] = values
    return np.ascontiguousarray((v.reshape(words, 32) << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64))


def fills(n, rng):
    last = np.zeros(n, dtype=np.uint8)
    if n:
        last[-1] = 2
    out = {"random": rng.integers(0, 4, n).astype(np.uint8), "zero": np.zeros(n, dtype=np.uint8), "last": last}
    for v in (1, 2, 3):
        out[f"all{v}"] = np.full(n, v, dtype=np.uint8)
    return out


def expect(values, off, src, mask, group_limit):
    """(row_off, row_n, ids, pos, perm) of the whole selection, uncapped: a per-group np.nonzero."""
    S = len(off) - 1
    surv = ((mask >> values.astype(np.uint32)) & 1).astype(bool)
    row_n = np.zeros(S, dtype=np.uint32)
    pos = []
    for s in range(S):
        k = np.nonzero(surv[off[s]:off[s + 1]])[0] + int(off[s])
        row_n[s] = len(k)
        pos.append(k[:group_limit] if group_limit else k)
    pos = np.concatenate(pos).astype(np.uint32) if pos else np.zeros(0, dtype=np.uint32)
    kept = np.minimum(row_n, group_limit) if group_limit else row_n
    row_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint32)
    return row_off, row_n, src[pos], pos, values[pos]


def run(hook, words, n, off, mask, group_limit, cap, src, want=("row_n", "ids", "pos", "perm"), lanes=0):
    S = len(off) - 1
    out = {"row_off": np.full(S + 3, P32, dtype=np.uint32), "row_n": np.full(S + 2, P32, dtype=np.uint32),
           "ids": np.full(cap + 2, P32, dtype=np.uint32), "pos": np.full(cap + 2, P32, dtype=np.uint32),
           "perm": np.full(cap + 2, P8, dtype=np.uint8)}
    cnt = C.c_uint32(0x7777)
    ptr = lambda k: out[k].ctypes.data if k in want else None
    rc = hook(words.ctypes.data, n, off.ctypes.data, S, mask, group_limit, cap, lanes, src.ctypes.data,
              out["row_off"].ctypes.data, ptr("row_n"), ptr("ids"), ptr("pos"), ptr("perm"), C.byref(cnt))
    return rc, out, cnt.value


def check(out, cnt, S, cap, exp, want, where):
    row_off, row_n, ids, pos, perm = exp
    total = int(row_off[-1])
    assert cnt == total, where
    assert np.array_equal(out["row_off"][:S + 1], row_off) and (out["row_off"][S + 1:] == P32).all(), where
    if "row_n" in want:
        assert np.array_equal(out["row_n"][:S], row_n) and (out["row_n"][S:] == P32).all(), where
    else:
        assert (out["row_n"] == P32).all(), where
    k = min(total, cap)
    for name, full, poison in (("ids", ids, P32), ("pos", pos, P32), ("perm", perm, P8)):
        if name in want:
            assert np.array_equal(out[name][:k], full[:k]) and (out[name][k:] == poison).all(), (where, name)
        else:
            assert (out[name] == poison).all(), (where, name)


@pytest.mark.parametrize("name", list(SETS))
def test_hook_matches_numpy(hook, name):
    lengths = SETS[name]
    off = offsets(lengths)
    n, S = int(off[-1]), len(lengths)
    rng = np.random.default_rng(n * 31 + S)
    src = rng.integers(0, max(2, n // 2), max(n, 1)).astype(np.uint32)  # (repeated ids)
    want = ("row_n", "ids", "pos", "perm")
    above = max(lengths) + 1
    for fill, values in fills(n, rng).items():
        words = pack_dense(values)
        # the degenerate fills answer alike under every mask that holds their value: two masks are enough
        masks = MASKS if fill in ("random", "last") or n <= 200 else (4, 10)
        for mask, group_limit in itertools.product(masks, (0, 1, 3, above)):
            exp = expect(values, off, src, mask, group_limit)
            total = int(exp[0][-1])
            for cap in sorted({0, 1, max(total - 1, 0), total, total + 5}):
                where = (name, fill, mask, group_limit, cap)
                rc, out, cnt = run(hook, words, n, off, mask, group_limit, cap, src)
                assert rc == 0, where
                check(out, cnt, S, cap, exp, want, where)


@pytest.mark.parametrize("lanes", (1, 2, 4, 8, 16, 32, 64))
def test_every_lane_width_walks_the_same_selection(hook, lanes):
    """The piece length L changes the walk, never the answer: groups below, at and above L words, and
    above 64 words, under every L."""
    lengths = [0, 1, 31, 32, 33, 64, 65, 0, 32 * lanes - 1, 32 * lanes, 32 * lanes + 1, 2100, 5, 4097, 0]
    off = offsets(lengths)
    n, S = int(off[-1]), len(lengths)
    rng = np.random.default_rng(lanes)
    values = rng.integers(0, 4, n).astype(np.uint8)
    src = rng.integers(0, 1000, n).astype(np.uint32)
    words = pack_dense(values)
    for mask, group_limit in itertools.product((4, 12, 14), (0, 3, 70)):
        exp = expect(values, off, src, mask, group_limit)
        total = int(exp[0][-1])
        for cap in (total - 1, total + 5):
            rc, out, cnt = run(hook, words, n, off, mask, group_limit, cap, src, lanes=lanes)
            assert rc == 0
            check(out, cnt, S, cap, exp, ("row_n", "ids", "pos", "perm"), (lanes, mask, group_limit, cap))


def test_group_limit_clips_offsets_but_not_group_counts(hook):
    lengths = [40, 3, 0, 70]
    off = offsets(lengths)
    values = np.full(113, 2, dtype=np.uint8)
    values[40:42] = 1  # group 1: one survivor, its last candidate
    src = np.arange(1000, 1113, dtype=np.uint32)
    rc, out, cnt = run(hook, pack_dense(values), 113, off, E.SELECT_LOOKUP, 3, 100, src)
    assert rc == 0 and cnt == 7
    assert out["row_off"][:5].tolist() == [0, 3, 4, 4, 7] and out["row_n"][:4].tolist() == [40, 1, 0, 70]
    assert out["pos"][:7].tolist() == [0, 1, 2, 42, 43, 44, 45]
    assert out["ids"][:7].tolist() == [1000, 1001, 1002, 1042, 1043, 1044, 1045]
    assert out["perm"][:7].tolist() == [2] * 7


@pytest.mark.parametrize("name", ["three_in_a_word", "one_long_among_short"])
def test_each_output_may_be_null(hook, name):
    off = offsets(SETS[name])
    n, S = int(off[-1]), len(off) - 1
    rng = np.random.default_rng(n)
    values = rng.integers(0, 4, n).astype(np.uint8)
    src = rng.integers(0, 1000, n).astype(np.uint32)
    words = pack_dense(values)
    names = ("row_n", "ids", "pos", "perm")
    for r in range(len(names) + 1):
        for want in itertools.combinations(names, r):
            for group_limit in (0, 3):
                exp = expect(values, off, src, E.SELECT_LOOKUP, group_limit)
                total = int(exp[0][-1])
                records = [w for w in want if w != "row_n"]
                for cap in (0, total - 1, total + 5):
                    rc, out, cnt = run(hook, words, n, off, E.SELECT_LOOKUP, group_limit, cap, src, want)
                    if cap and not records:  # cap > 0 with all three record arrays NULL
                        assert rc == -1 and cnt == 0x7777, (want, cap)
                        assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in out), (want, cap)
                        continue
                    assert rc == 0, (want, cap)
                    check(out, cnt, S, cap, exp, want, (want, group_limit, cap))


def test_empty_requests(hook):
    src, words = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    # S == 0: row_off[0] and the count alone
    rc, out, cnt = run(hook, words, 0, np.zeros(1, dtype=np.uint32), 4, 0, 4, src)
    assert rc == 0 and cnt == 0 and out["row_off"].tolist() == [0, P32, P32]
    assert all((out[k] == (P8 if k == "perm" else P32)).all() for k in ("row_n", "ids", "pos", "perm"))
    # n == 0 with S == 3: S + 1 zero offsets, S zero counts, and the offsets are not read (garbage here)
    rc, out, cnt = run(hook, words, 0, np.array([9, 4, 77, 1], dtype=np.uint32), 4, 0, 4, src)
    assert rc == 0 and cnt == 0 and out["row_off"].tolist() == [0, 0, 0, 0, P32, P32]
    assert out["row_n"].tolist() == [0, 0, 0, P32, P32] and (out["ids"] == P32).all()


def test_argument_errors(hook):
    off = offsets([30, 10])
    values = np.random.default_rng(3).integers(0, 4, 40).astype(np.uint8)
    words, src = pack_dense(values), np.arange(40, dtype=np.uint32)
    row_off, ids = np.full(3, P32, dtype=np.uint32), np.full(16, P32, dtype=np.uint32)
    cnt = C.c_uint32(0x7777)
    good = [words.ctypes.data, 40, off.ctypes.data, 2, E.SELECT_LOOKUP, 0, 8, 0, src.ctypes.data, row_off.ctypes.data,
            None, ids.ctypes.data, None, None, C.byref(cnt)]
    assert hook(*good) == 0 and cnt.value != 0x7777
    row_off[:], ids[:], cnt.value = P32, P32, 0x7777

    def bad(**changes):
        args = list(good)
        for k, v in changes.items():
            args[int(k[1:])] = v
        assert hook(*args) == -1, changes
        assert (row_off == P32).all() and (ids == P32).all() and cnt.value == 0x7777, changes

    for mask in (0, 1, 3, 15, 16, 0x12):  # gck_select's rule
        bad(a4=mask)
    bad(a9=None)                          # null row_off
    bad(a14=None)                         # null count word
    bad(a11=None)                         # cap > 0 with all three record arrays null
    bad(a9=row_off.ctypes.data + 2)       # a u32 output that is not 4-byte aligned
    bad(a10=row_off.ctypes.data + 1)
    bad(a11=ids.ctypes.data + 2)
    bad(a12=ids.ctypes.data + 1)
    bad(a0=None)                          # a plane to read and none given
    bad(a2=None)                          # offsets to read and none given
    bad(a3=0)                             # candidates without a group
    bad(a7=3)                             # a lane count that is no power of two
    bad(a7=128)


# ---- the group lookup ----

def lookup(group_of, off, ks):
    ks = np.ascontiguousarray(ks, dtype=np.uint32)
    out = np.full(len(ks) + 1, P32, dtype=np.uint32)
    assert group_of(off.ctypes.data, len(off) - 1, ks.ctypes.data, len(ks), out.ctypes.data) == 0
    assert out[-1] == P32
    return out[:-1]


@pytest.mark.parametrize("name", [k for k, v in SETS.items() if sum(v)])
def test_group_of_matches_searchsorted(group_of, name):
    off = offsets(SETS[name])
    n, S = int(off[-1]), len(off) - 1
    ks = np.arange(n + 3, dtype=np.uint32)  # every check, and three positions beyond the request (clamped)
    want = np.clip(np.searchsorted(off, ks, side="right").astype(np.int64) - 1, 0, S - 1)
    got = lookup(group_of, off, ks)
    assert np.array_equal(got, want), name
    inside = got[:n]
    assert (off[inside] <= ks[:n]).all() and (ks[:n] < off[inside + 1]).all()  # off[s] <= k < off[s + 1]


MALFORMED = {
    "descending": [0, 50, 20, 90, 100],
    "all_descending": [100, 80, 60, 40, 0],
    "beyond_n": [0, 10, 5000, 0xFFFFFFFF, 100],
    "first_not_zero": [7, 10, 20, 30, 100],
    "last_not_n": [0, 10, 20, 30, 64],
    "last_beyond_n": [0, 10, 20, 30, 1000],
    "huge": [0xFFFFFFFF] * 5,
    "one_group_bad": [5, 3],
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_offsets_stay_in_bounds(hook, group_of, name):
    """Offsets nobody validated: the lookup stays within [0, S - 1], and the selection — whose answer is
    then unspecified — reads only the plane's words and the candidates below n and writes only below
    S + 1, S and cap."""
    off = np.array(MALFORMED[name], dtype=np.uint32)
    S, n = len(off) - 1, 100
    ks = np.concatenate([np.arange(n + 40), [2 ** 31, 2 ** 32 - 1]]).astype(np.uint32)
    got = lookup(group_of, off, ks)
    assert (got < S).all(), name
    rng = np.random.default_rng(S)
    values = rng.integers(0, 4, n).astype(np.uint8)
    words, src = pack_dense(values), np.arange(n, dtype=np.uint32)
    for group_limit, cap in itertools.product((0, 3), (0, 7, 500)):
        rc, out, cnt = run(hook, words, n, off, E.SELECT_LOOKUP, group_limit, cap, src)
        assert rc == 0
        assert (out["row_off"][S + 1:] == P32).all() and (out["row_n"][S:] == P32).all()
        for k, poison in (("ids", P32), ("pos", P32), ("perm", P8)):
            assert (out[k][cap:] == poison).all(), (name, k)
            written = out[k][:min(cnt, cap)]
            if k != "perm":
                assert (written < n).all(), (name, k)  # a candidate of the request, never beyond it
