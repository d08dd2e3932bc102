"""The compact request path on the GPU where its formats meet (include/gck.h gck_check_bulk_uniform /
_shaped, gck_check_submit_uniform / _shaped): one request sent as items, as a uniform request and
as shaped requests gives the same words and error list; the error list is cut at the caller's cap
across chunks and at the wait; a submit above max_batch fails and gives its workspace back.

The requests are checks of one shape over the near_budget graph at its depth budget of 8, where
about half of the checks end in an item error, with the oracle's answers computed once."""
import ctypes as C
import random
import threading
import time

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests import gen
from tests.helpers import oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF
DEPTH = gen.FAMILY_DEPTH["near_budget"]
# test_submit_above_max_batch: its follow-up request took 2.2 ms on the parent commit (see
# profiles/r10/compact_path/README.md); a leaked workspace would block it for ever
FOLLOW_UP_LIMIT_S = 5.0


@pytest.fixture(scope="module")
def graph():
    """The graph, 100 doc#view@user checks over it and the oracle's (permissionship, error) of each."""
    schema, tuples, _ = gen.near_budget(2)
    ck = oracle_for(schema, tuples, max_depth=DEPTH, now=NOW_US / 1e6)
    rng = random.Random(7)
    picks = rng.sample([(d, u) for d in range(40) for u in range(40)], 100)
    checks = [f"doc:d{d}#view@user:u{u}" for d, u in picks]
    want = [tuple(ck.check(to_oracle_item(parse_check(c)))) for c in checks]
    return schema, tuples, checks, want


def _engine(graph, **kw):
    e = E.Engine(device=0, max_depth=DEPTH, **kw)
    e.load_schema(graph[0])
    e.load_snapshot_text(1, "\n".join(graph[1]))
    return e


def _request(e, checks):
    """The checks as items, their one shape and their (resource id, subject id) pairs."""
    items = e.make_items([parse_check(c) for c in checks])
    shapes, shape_of, pairs = E.shape_request(items)
    assert len(shapes) == 1 and not shape_of.any()
    return items, shapes[0], pairs


def _pack(perm, err):
    """What a compact request answers for these item results: the words and the error records."""
    words = np.zeros((len(perm) + 31) // 32, dtype=np.uint64)
    for k, (p, x) in enumerate(zip(perm, err)):
        if x == 0:
            words[k >> 5] |= np.uint64((int(p) & 3) << (2 * (k & 31)))
    return words.tolist(), [(k, int(x)) for k, x in enumerate(err) if x != 0]


def _records(errs):
    return [(int(r["index"]), int(r["code"])) for r in errs]


# ---- 1. the three request formats agree ------------------------------------------------------------

def test_formats_agree(graph):
    n = 65  # three words, the last holding one check
    checks, want = graph[2][:n], graph[3][:n]
    assert any(w[1] != 0 for w in want) and any(w[1] == 0 and w[0] != 0 for w in want)
    e = _engine(graph)
    items, shape, pairs = _request(e, checks)
    spread = (np.arange(n) % 4).astype(np.uint8)  # the same header four times, indices over the copies
    pin_pairs, pin_idx = e.host_array(2 * n, np.uint32).reshape(-1, 2), e.host_array(n, np.uint8)
    pin_words = e.host_array(3, np.uint64)

    def four_ways(pinned):
        perm, err = e.check_bulk(items, now_us=NOW_US)
        ref = _pack(perm, err)
        assert ref == _pack([w[0] for w in want], [w[1] for w in want])  # (and the oracle's)
        got = {}
        for what, table, idx in (("uniform", None, None), ("one shape", [shape], np.zeros(n, np.uint8)),
                                 ("four copies", [shape] * 4, spread)):
            p, out = pairs, None
            if pinned:
                pin_pairs[:] = pairs
                pin_words[:] = POISON  # every word must be written
                p, out = pin_pairs, pin_words
                if idx is not None:
                    pin_idx[:] = idx
                    idx = pin_idx
            if table is None:
                words, errs, _ = e.check_uniform(shape, p, now_us=NOW_US, out_packed=out)
            else:
                words, errs, _ = e.check_shaped(table, idx, p, now_us=NOW_US, out_packed=out)
            got[what] = (words.tolist(), _records(errs))
        assert got == {what: ref for what in got}

    four_ways(pinned=True)
    four_ways(pinned=False)
    e.set_profile(True)  # a profiled batch takes the expanded path
    before = e.shaped_stats()
    four_ways(pinned=True)
    four_ways(pinned=False)
    assert e.shaped_stats() == (before[0], before[1] + 4)
    e.close()


# ---- 2. the error list's cap ----------------------------------------------------------------------

def _raw(e, shape, n_copies, pairs, cap, submit):
    """One request through the C entry points themselves (the Python methods do not return the
    count): uniform (n_copies == 0), or shaped over n_copies copies of the header. Returns (words,
    the records written, *n_errs)."""
    n = len(pairs)
    lib, cs = e._lib, E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32)
    words = np.full((n + 31) // 32, POISON, dtype=np.uint64)
    errs = np.zeros(max(1, cap), dtype=E.ITEM_ERROR_DTYPE)
    n_errs, handle = C.c_size_t(12345), C.c_void_p()
    last = C.byref(handle) if submit else None  # (synchronous: out_revision)
    tail = (pairs.ctypes.data, n, None, None, 0, NOW_US, words.ctypes.data, errs.ctypes.data if cap else None, cap,
            C.byref(n_errs), last)
    if n_copies == 0:
        hdr = E.Uniform(*shape[:4], shape[4], 0)
        fn = lib.gck_check_submit_uniform if submit else lib.gck_check_bulk_uniform
        E._check(fn(e._h, C.byref(cs), C.byref(hdr), *tail))
    else:
        table, m = E._shape_table([shape] * n_copies)
        idx = (np.arange(n) % n_copies).astype(np.uint8)
        fn = lib.gck_check_submit_shaped if submit else lib.gck_check_bulk_shaped
        E._check(fn(e._h, C.byref(cs), C.addressof(table), m, idx.ctypes.data, *tail))
    if submit:
        E._check(lib.gck_check_wait(e._h, handle))
    return words.tolist(), _records(errs[:cap]), n_errs.value


@pytest.mark.parametrize("submit", (False, True), ids=("sync", "submit"))
def test_error_list_cap(graph, submit):
    checks, want = graph[2], graph[3]
    want_words, want_errs = _pack([w[0] for w in want], [w[1] for w in want])
    # the oracle's errors: at least 3, in at least 2 of the four chunks of 32
    assert len(checks) == 100 and len(want_errs) >= 3 and len({k // 32 for k, _ in want_errs}) >= 2
    # synchronous: four chunks; a submitted batch is one chunk, so its engine holds the request whole
    e = _engine(graph, max_batch=128 if submit else 32)
    _, shape, pairs = _request(e, checks)
    for n_copies in (0, 4):
        words, errs, count = _raw(e, shape, n_copies, pairs, 2, submit)
        assert (words, errs, count) == (want_words, want_errs[:2], len(want_errs)), n_copies
        words, errs, count = _raw(e, shape, n_copies, pairs, 0, submit)  # no list: the count alone
        assert (words, errs, count) == (want_words, [], len(want_errs)), n_copies
    e.close()


# ---- 3. a submit above max_batch ------------------------------------------------------------------

def test_submit_above_max_batch(graph):
    e = _engine(graph, max_batch=64, workspaces=1)
    _, shape, pairs = _request(e, graph[2][:65])
    words, errs = np.zeros(3, dtype=np.uint64), np.zeros(65, dtype=E.ITEM_ERROR_DTYPE)
    with pytest.raises(E.GckError) as ex:
        e.submit_uniform(shape, pairs, words, errs, now_us=NOW_US)
    assert ex.value.code == E.GCK_E_INVALID_ARGUMENT
    with pytest.raises(E.GckError) as ex:
        e.submit_shaped([shape], np.zeros(65, dtype=np.uint8), pairs, words, errs, now_us=NOW_US)
    assert ex.value.code == E.GCK_E_INVALID_ARGUMENT
    # the one workspace went back to the pool both times: a request that fits runs (in a thread of
    # its own: with the workspace leaked it would wait for ever)
    got = {}

    def follow_up():
        t0 = time.perf_counter()
        got["uniform"] = e.submit_uniform(shape, pairs[:64], words, errs, now_us=NOW_US).wait()
        got["seconds"] = time.perf_counter() - t0

    t = threading.Thread(target=follow_up, daemon=True)
    t.start()
    t.join(timeout=FOLLOW_UP_LIMIT_S)
    assert not t.is_alive(), "the 64-check request is blocked: a failed submit kept the workspace"
    print(f"follow-up request: {got['seconds'] * 1e3:.2f} ms")
    want = graph[3][:64]
    out, out_errs, _ = got["uniform"]
    assert (out[:2].tolist(), _records(out_errs)) == _pack([w[0] for w in want], [w[1] for w in want])
    e.close()
