"""The packing of an over-full user's cover entries into its slot (gochugaru_amd/csrc/slot_pack.hpp:
the code the slot-build kernels run, called here on the host through libgck.so's test hooks
gck_test_slot_window / gck_test_slot_pack) against brute force over random entry sets of 21-64 entries, at
both entry widths: the omitted run's open range must be the narrowest there is, every omitted entry
must lie strictly inside it and every other entry be inline, and the slot round's rule over the
packed slot (HAS from an inline entry, NO when no interval reaches into the range) must never
contradict the whole list. No GPU."""
import ctypes as C

import numpy as np
import pytest

from gochugaru_amd import engine as E

LIST, LO_OPEN, HI_OPEN, COUNT = 0x40000000, 0x20000000, 0x10000000, 0x0FFFFFFF
CAP = {24: 20, 32: 15}
SORT_MAX = 64


@pytest.fixture(scope="module")
def lib():
    lib = E.load_library()
    lib.gck_test_slot_window.restype = C.c_uint32
    lib.gck_test_slot_window.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.gck_test_slot_pack.restype = C.c_int
    lib.gck_test_slot_pack.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def pack(lib, bits, raw, list_at):
    raw = np.ascontiguousarray(raw, dtype=np.uint32)
    w = np.full(16, 0xDEADBEEF, dtype=np.uint32)
    m = lib.gck_test_slot_pack(bits, raw.ctypes.data, len(raw), list_at, w.ctypes.data)
    return m, w


def entries(bits, w):
    """The slot's cap entry positions, as closure.inc slot_entry reads them."""
    if bits == 32:
        return [int(x) for x in w[1:16]]
    big = sum(int(x) << (32 * i) for i, x in enumerate(w))
    return [(big >> (32 + 24 * k)) & 0xFFFFFF for k in range(20)]


def width(e, s, n_om):
    lo1 = e[s - 1] + 1 if s else 0
    hi = e[s + n_om] if s + n_om < len(e) else 0xFFFFFFFF
    return hi - lo1


def random_sets(rng, bits, n):
    top = (1 << 24) - 2 if bits == 24 else (1 << 32) - 2
    for _ in range(n):
        m = int(rng.integers(CAP[bits] + 1, SORT_MAX + 1))
        kind = rng.integers(0, 4)
        if kind == 0:    # anywhere
            e = rng.integers(0, top, size=m)
        elif kind == 1:  # a dense block (ties between windows; neighbours one apart)
            e = int(rng.integers(0, top - 200)) + rng.choice(200, size=m, replace=False)
        elif kind == 2:  # two clusters far apart, including 0 and the largest value
            e = np.concatenate([rng.choice(500, size=m // 2, replace=False), top - rng.choice(500, size=m - m // 2, replace=False)])
            e[0], e[-1] = 0, top
        else:            # a dense block with duplicates up to the raw bound
            e = int(rng.integers(0, top - 100)) + rng.integers(0, 40, size=m)
        yield np.unique(np.asarray(e, dtype=np.uint64)).astype(np.uint32), np.asarray(e, dtype=np.uint32)


@pytest.mark.parametrize("bits", [24, 32])
def test_window_is_narrowest_and_holds_every_omitted_entry(lib, bits):
    rng = np.random.default_rng(bits)
    cap, n_in = CAP[bits], CAP[bits] - 2
    unused = 0xFFFFFF if bits == 24 else 0xFFFFFFFF
    n_listed = 0
    for uniq, raw in random_sets(rng, bits, 600):
        rng.shuffle(raw)
        m, w = pack(lib, bits, raw, 0x12345678)
        e = [int(x) for x in uniq]
        assert m == len(e)
        p = entries(bits, w)
        if m <= cap:  # (fits once the duplicates are gone: an ordinary inline slot)
            assert int(w[0]) == m and p[:m] == e and all(x == unused for x in p[m:])
            continue
        n_listed += 1
        n_om = m - n_in
        h = int(w[0])
        assert h & LIST and not h & 0x80000000 and h & COUNT == m and int(w[15]) == 0x12345678
        s = lib.gck_test_slot_window(uniq.ctypes.data, m, n_in)
        best = min(width(e, k, n_om) for k in range(n_in + 1))
        assert width(e, s, n_om) == best, (e, s)
        assert bool(h & LO_OPEN) == (s == 0) and bool(h & HI_OPEN) == (s == n_in)
        inline, omitted = p[:n_in], e[s:s + n_om]
        assert sorted(inline) == e[:s] + e[s + n_om:]
        lo = -1 if h & LO_OPEN else inline[-1]
        hi = 0xFFFFFFFF if h & HI_OPEN else inline[0]  # (beyond the list's end: above every entry)
        assert hi - (lo + 1) == best
        assert all(lo < x < hi for x in omitted), (lo, hi, omitted)
        if bits == 32:
            assert int(w[14]) == 0
        else:
            assert int(w[14]) >> 16 == 0
    assert n_listed > 300


def decide(bits, w, intervals):
    """closure.inc slot_decide_wave over one listed or inline slot: 2 HAS, 1 NO, 3 the list round."""
    h = int(w[0])
    p = entries(bits, w)
    n_in = CAP[bits] - 2
    unused = 0xFFFFFF if bits == 24 else 0xFFFFFFFF
    listed = bool(h & LIST)
    if listed:
        p[n_in] = p[n_in + 1] = unused
    hi = 0xFFFFFFFF if h & HI_OPEN else p[0]
    lo1 = 0 if h & LO_OPEN else p[n_in - 1] + 1
    hit = any(a <= x < b for a, b in intervals for x in p)
    reach = any(a < hi and b > lo1 for a, b in intervals)
    return 2 if hit else 3 if listed and reach else 1


@pytest.mark.parametrize("bits", [24, 32])
def test_slot_rule_never_contradicts_the_list(lib, bits):
    rng = np.random.default_rng(100 + bits)
    n_in = CAP[bits] - 2
    seen = {1: 0, 2: 0, 3: 0}
    for uniq, raw in random_sets(rng, bits, 300):
        m, w = pack(lib, bits, raw, 7)
        e = [int(x) for x in uniq]
        if m <= CAP[bits]:
            continue
        s = lib.gck_test_slot_window(uniq.ctypes.data, m, n_in)
        om = e[s:s + m - n_in]
        lo = e[s - 1] if s else None
        hi = e[s + m - n_in] if s + m - n_in < m else None
        cases = [[]]
        cases += [[(x, x + 1)] for x in (e[0], e[-1], e[n_in // 2], om[0], om[-1])]  # one entry each
        if om[0] + 1 < om[-1] and om[0] + 1 not in e:
            cases.append([(om[0] + 1, om[0] + 2)])           # inside the window, no entry
        if lo is not None:
            cases += [[(max(lo - 3, 0), lo + 1)], [(lo + 1, lo + 2)] if lo + 1 not in e else []]  # ends at lo + 1; begins there
        if hi is not None:
            cases += [[(hi, hi + 5)], [(hi - 1, hi)] if hi - 1 not in e else []]          # begins at hi; ends at it
        cases.append([(om[0], om[-1] + 1)])                   # spans the omitted run
        cases.append([(0, e[-1] + 1)])                        # everything
        for _ in range(20):
            k = int(rng.integers(1, 8))
            a = rng.choice(np.array(e + [x + 1 for x in e] + [max(x - 1, 0) for x in e]), size=k)
            cases.append([(int(x), int(x) + int(rng.integers(0, 4))) for x in a])
        # (no interval ends above the unused-entry mark: the snapshot picks the width so)
        unused = 0xFFFFFF if bits == 24 else 0xFFFFFFFF
        cases = [[(a, min(b, unused)) for a, b in iv] for iv in cases]
        for iv in cases:
            truth = 2 if any(a <= x < b for a, b in iv for x in e) else 1
            got = decide(bits, w, iv)
            seen[got] += 1
            assert got == truth or got == 3, (e, s, iv, got, truth)
    assert all(v > 100 for v in seen.values()), seen


@pytest.mark.parametrize("bits", [24, 32])
def test_more_raw_entries_than_the_sorting_bound_keep_a_plain_list(lib, bits):
    raw = np.arange(65, dtype=np.uint32) * 3
    m, w = pack(lib, bits, raw, 99)
    assert m == 65 and int(w[0]) == LIST | LO_OPEN | HI_OPEN | 65 and int(w[15]) == 99
    assert decide(bits, w, [(0, 1)]) == 3 and decide(bits, w, [(5000, 5001)]) == 3 and decide(bits, w, []) == 1
    assert decide(bits, w, [(0, 0)]) == 1  # (an empty interval, as an unused one of a resource slot is)
