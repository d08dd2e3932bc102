"""The 16-B front of a resource slot (gochugaru_amd/csrc/slot_pack.hpp front_pack / front_unpack,
through the gck_test_front_pack hook): what packs, what is flagged "read the slot", and that a
packed front stands for exactly the first half of its slot. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from gochugaru_amd import engine as E

OVERFLOW = 0x80000000
LEN_MAX = (1 << 18) - 1
FLAG = np.full(4, 0xFFFFFFFF, dtype=np.uint32)


@pytest.fixture(scope="module")
def lib():
    lib = E.load_library()
    lib.gck_test_front_pack.restype = C.c_int
    lib.gck_test_front_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def slot_of(intervals, count=None):
    """A resource slot as k_res_slots writes it: the count, a zero word, [start, end) per interval."""
    w = np.zeros(16, dtype=np.uint32)
    w[0] = len(intervals) if count is None else count
    for k, (lo, ln) in enumerate(intervals[:7]):
        w[2 + 2 * k] = lo
        w[3 + 2 * k] = (lo + ln) & 0xFFFFFFFF
    return w


def pack(lib, w):
    f = np.zeros(4, dtype=np.uint32)
    d = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    rc = lib.gck_test_front_pack(w.ctypes.data, f.ctypes.data, d.ctypes.data)
    assert rc in (0, 1)
    if rc == 0:
        assert (f == FLAG).all() and (d == 0xDEADBEEF).all()
    else:
        assert not (f == FLAG).all()
        assert (d == w[:8]).all() and not w[8:].any(), (w, d)  # the intervals equal the slot's first three
    return rc, f


def ivs(n, start=1000, ln=7):
    return [(start + 100 * k, ln + k) for k in range(n)]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 7])
def test_counts(lib, n):
    rc, _ = pack(lib, slot_of(ivs(n)))
    assert rc == (1 if n <= 3 else 0)


def test_count_8_is_an_overflow_slot(lib):
    w = np.zeros(16, dtype=np.uint32)  # (k_res_slots: more than 7 groups)
    w[0] = OVERFLOW
    assert pack(lib, w)[0] == 0


@pytest.mark.parametrize("ln,ok", [(1, 1), (LEN_MAX, 1), (LEN_MAX + 1, 0), (0, 0)])
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_lengths(lib, ln, ok, pos):
    iv = ivs(3)
    iv[pos] = (iv[pos][0], ln)
    assert pack(lib, slot_of(iv))[0] == ok


@pytest.mark.parametrize("start,ok", [(0, 1), ((1 << 24) - 2, 1), ((1 << 24) - 1, 1), (1 << 24, 0)])
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_starts(lib, start, ok, pos):
    for ln in (1, LEN_MAX):
        iv = ivs(3)
        iv[pos] = (start, ln)
        assert pack(lib, slot_of(iv))[0] == ok


def test_the_record_that_would_read_as_the_flag_is_flagged(lib):
    assert pack(lib, slot_of([((1 << 24) - 1, LEN_MAX)] * 3))[0] == 0
    assert pack(lib, slot_of([((1 << 24) - 1, LEN_MAX)] * 2 + [((1 << 24) - 1, LEN_MAX - 1)]))[0] == 1


def test_an_end_below_its_start_and_stray_words_are_flagged(lib):
    w = slot_of(ivs(2))
    w[3] = w[2] - 1
    assert pack(lib, w)[0] == 0
    for at, v in ((1, 1), (6, 5), (8, 1), (15, 1)):  # word 1, an interval past the count, the second half
        w = slot_of(ivs(2))
        w[at] = v
        assert pack(lib, w)[0] == 0
    w = slot_of(ivs(2))
    w[3] |= OVERFLOW  # (a flag bit on an end: a length beyond 18 bits)
    assert pack(lib, w)[0] == 0


def test_random_slots_round_trip(lib):
    rng = np.random.default_rng(12)
    packed = 0
    for _ in range(4000):
        n = int(rng.integers(0, 8))
        iv = [(int(rng.integers(0, 1 << 24)), int(rng.choice([1, 2, 255, 256, 1023, LEN_MAX - 1, LEN_MAX, LEN_MAX + 1,
                                                                int(rng.integers(1, 1 << 19))]))) for _ in range(n)]
        rc, _ = pack(lib, slot_of(iv))
        want = n <= 3 and all(ln <= LEN_MAX for _, ln in iv)
        assert rc == int(want), (iv, rc)
        packed += rc
    assert packed > 500


def test_bad_arguments(lib):
    w = slot_of(ivs(1))
    f = np.zeros(4, dtype=np.uint32)
    assert lib.gck_test_front_pack(None, f.ctypes.data, w.ctypes.data) == -1
    assert lib.gck_test_front_pack(w.ctypes.data, None, w.ctypes.data) == -1
