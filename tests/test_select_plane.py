"""The ordered selection over a plane of 2-bit results (gochugaru_amd/csrc/select_plane.hpp: the
functions k_dc_select runs, called here on the host through libgck.so's test hook
gck_test_select_plane) against numpy: for every mask, word counts at the edges of a 256-word tile,
random and degenerate fills, a zero and a non-zero rank base, and every kind of cap — positions and
Permissionships compared exactly, nothing written beyond min(total, cap). No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gochugaru_amd import engine as E

MASKS = (2, 4, 8, 6, 10, 12, 14)
WORDS = (1, 2, 255, 256, 257, 2047, 2048)
POISON_POS, POISON_PERM = 0xDEADBEEF, 0xA5


@pytest.fixture(scope="module")
def hook():
    lib = E.load_library()
    fn = lib.gck_test_select_plane
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return fn


def pack(values):
    """32 two-bit values per little-endian u64 word, check b in bits 2b .. 2b + 1."""
    v = np.asarray(values, dtype=np.uint64).reshape(-1, 32)
    return (v << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def fills(n_words, rng):
    n = n_words * 32
    last = np.zeros(n, dtype=np.uint8)
    last[-1] = 2
    out = {"random": rng.integers(0, 4, n).astype(np.uint8), "zero": np.zeros(n, dtype=np.uint8),
           "alternating": np.tile(np.array([1, 2], dtype=np.uint8), n // 2), "last": last}
    for v in (1, 2, 3):
        out[f"all{v}"] = np.full(n, v, dtype=np.uint8)
    return out


def run(hook, words, mask, base, cap):
    pos = np.full(cap + 2, POISON_POS, dtype=np.uint32)
    perm = np.full(cap + 2, POISON_PERM, dtype=np.uint8)
    n = C.c_uint32(0x7777)
    assert hook(words.ctypes.data, len(words), mask, base, cap, pos.ctypes.data, perm.ctypes.data, C.byref(n)) == 0
    return pos, perm, n.value


@pytest.mark.parametrize("n_words", WORDS)
def test_hook_matches_numpy(hook, n_words):
    rng = np.random.default_rng(n_words)
    for name, values in fills(n_words, rng).items():
        words = pack(values)
        for mask, base in itertools.product(MASKS, (0, 1000)):
            want_pos = np.flatnonzero((mask >> values.astype(np.uint32)) & 1).astype(np.uint32)
            want_perm = values[want_pos]
            total = len(want_pos)
            caps = {0, max(total - 1, 0), total, total + 5}
            # survivors of the chunk take ranks base .. base + total - 1 of the request: a cap below
            # base leaves nothing to write, one inside the chunk cuts it, one above takes all of it
            for cap in sorted(caps | {base + c for c in caps}):
                pos, perm, n = run(hook, words, mask, base, cap)
                assert n == base + total, (name, mask, base, cap)
                k = max(0, min(total, cap - base))
                assert np.array_equal(pos[base:base + k], want_pos[:k]), (name, mask, base, cap)
                assert np.array_equal(perm[base:base + k], want_perm[:k]), (name, mask, base, cap)
                untouched = np.ones(cap + 2, dtype=bool)
                untouched[base:base + k] = False
                assert (pos[untouched] == POISON_POS).all() and (perm[untouched] == POISON_PERM).all(), \
                    (name, mask, base, cap)


def test_either_output_may_be_null_and_bad_masks_are_refused(hook):
    values = np.random.default_rng(7).integers(0, 4, 64 * 32).astype(np.uint8)
    words = pack(values)
    want = np.flatnonzero((E.SELECT_LOOKUP >> values.astype(np.uint32)) & 1).astype(np.uint32)
    n = C.c_uint32(0)
    pos = np.full(len(want) + 2, POISON_POS, dtype=np.uint32)
    assert hook(words.ctypes.data, len(words), E.SELECT_LOOKUP, 0, len(want), pos.ctypes.data, None, C.byref(n)) == 0
    assert n.value == len(want) and np.array_equal(pos[:len(want)], want) and (pos[len(want):] == POISON_POS).all()
    perm = np.full(len(want) + 2, POISON_PERM, dtype=np.uint8)
    assert hook(words.ctypes.data, len(words), E.SELECT_LOOKUP, 0, len(want), None, perm.ctypes.data, C.byref(n)) == 0
    assert np.array_equal(perm[:len(want)], values[want]) and (perm[len(want):] == POISON_PERM).all()
    for mask in (0, 1, 3, 15, 16, 0x12):
        assert hook(words.ctypes.data, len(words), mask, 0, 0, None, None, C.byref(n)) == -1, mask
