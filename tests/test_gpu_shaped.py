"""Shaped requests on the GPU (include/gck.h gck_check_bulk_shaped / gck_check_submit_shaped).

A request that mixes permissions, resource types, subject kinds and context slots check by check
travels as a table of at most 64 shapes, one index byte per check and the id pairs, and is answered
with the uniform request's packed words and error list. Bar, against the oracle throughout: the
words equal the oracle's Permissionship (0 for an errored check) and the error list equals the
oracle's errored checks in order — on the zero-copy join (closure and label join, pinned and
pageable buffers, every size at the edges of the half wave, the wave and the block, every table
lane), on the expanded fallback (check contexts, profiling, no join), across chunks, in flight,
after a Watch batch and through the Client. A shape index beyond the table fails the request on the
host's side, naming the check, and leaves the engine usable."""
import json
import random

import numpy as np
import pytest

from gochugaru_amd import consistency
from gochugaru_amd import engine as E
from gochugaru_amd.client import CheckItemError, Client, WithCompactRequests
from tests import gen
from tests.helpers import load_golden, oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF


def _engine(schema, tuples, revision=1, **kw):
    e = E.Engine(device=0, **kw)
    e.load_schema(schema)
    e.load_snapshot_text(revision, "\n".join(tuples))
    return e


def _want(schema, tuples, checks, depth=50, contexts=None):
    ck = oracle_for(schema, tuples, max_depth=depth, now=NOW_US / 1e6)
    ctx = contexts or [None] * len(checks)
    return [tuple(ck.check(to_oracle_item(parse_check(c), x))) for c, x in zip(checks, ctx)]


def _expected(want):
    perm = [w[0] if w[1] == 0 else 0 for w in want]
    errs = [(k, w[1]) for k, w in enumerate(want) if w[1] != 0]
    return perm, errs


class _Pinned:
    """Pinned request buffers of one engine, allocated once and sliced per request."""

    def __init__(self, e, cap):
        self.pairs = e.host_array(2 * cap, np.uint32)
        self.idx = e.host_array(cap, np.uint8)
        self.words = e.host_array((cap + 31) // 32, np.uint64)

    def load(self, shape_of, pairs):
        n = len(shape_of)
        self.pairs[:2 * n] = np.asarray(pairs, dtype=np.uint32).reshape(-1)
        self.idx[:n] = shape_of
        w = self.words[:(n + 31) // 32]
        w[:] = POISON  # every word must be written
        return self.idx[:n], self.pairs[:2 * n].reshape(-1, 2), w


def _check(e, shapes, shape_of, pairs, want, pin=None, contexts=None, what=None):
    """One shaped request (pinned through `pin`, else pageable) against the oracle's answers."""
    n = len(shape_of)
    shape_of = np.asarray(shape_of, dtype=np.uint8)
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    if pin is not None:
        idx_arg, pairs_arg, words = pin.load(shape_of, pairs)
    else:
        idx_arg, pairs_arg, words = shape_of, pairs, None
    out, errs, rev = e.check_shaped(shapes, idx_arg, pairs_arg, now_us=NOW_US, contexts=contexts, out_packed=words)
    assert rev == e.revision
    got = E.unpack_results(out, n).tolist()
    wp, we = _expected(want)
    bad = [(k, int(shape_of[k]), pairs[k].tolist(), wp[k], got[k]) for k in range(n) if wp[k] != got[k]]
    assert not bad, (what, n, bad[:5])
    assert [(int(r["index"]), int(r["code"])) for r in errs] == we, (what, n)
    return out, errs


# ---- 1. every family's whole check list, interleaved as generated, as ONE request ---------------

FAMS = sorted(gen.FAMILIES)


@pytest.mark.parametrize("family", FAMS)
def test_family_as_one_shaped_request(family):
    schema, tuples, checks = gen.FAMILIES[family](2)
    depth = gen.FAMILY_DEPTH.get(family, 50)
    e = _engine(schema, tuples, max_depth=depth)
    want = _want(schema, tuples, checks, depth)
    items = e.make_items([parse_check(c) for c in checks])
    shapes, shape_of, pairs = E.shape_request(items)
    assert 2 <= len(shapes) <= 64
    pin = _Pinned(e, len(checks))
    e.reset_stats()
    s0 = e.shaped_stats()
    _check(e, shapes, shape_of, pairs, want, pin=pin, what="pinned")
    _check(e, shapes, shape_of, pairs, want, what="pageable")
    # the item path is the second witness
    perm, err = e.check_bulk(items, now_us=NOW_US)
    assert [(int(p), int(x)) for p, x in zip(perm, err)] == want
    if family in ("nested", "gdocs", "github"):  # the join read the requests in place
        st = e.stats()
        assert e.shaped_stats()[0] >= s0[0] + 2
        assert st["aql_batches"] > 0 and st["closure_checks"] > 0
    e.close()


# ---- 2. edges of the half wave, the wave and the block ------------------------------------------

SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
EXTRA = {
    "nested": ["doc:d3#view@user:*", "doc:d17#view@user:*", "doc:d5#view@group:g7#member"],
    "github": ["repo:r3#read@team:t2#member", "repo:r7#read@team:t5#member", "repo:r9#write@team:t1#member",
               "repo:r3#read@user:*", "repo:r8#write@user:*"],
    "gdocs": ["doc:d4#view@user:*", "doc:d9#edit@user:*", "folder:f2#view@group:g3#member"],
}


class _Pool:
    """A family's checks (and a few userset / wildcard subjects) with the oracle's answers, grouped
    by shape: requests of any pattern are drawn from it without asking the oracle again."""

    def __init__(self, family):
        self.schema, self.tuples, checks = gen.FAMILIES[family](2)
        self.checks = checks + EXTRA[family]
        self.want = _want(self.schema, self.tuples, self.checks)
        self.e = _engine(self.schema, self.tuples, workspaces=8)
        self.items = self.e.make_items([parse_check(c) for c in self.checks])
        shapes, shape_of, self.pairs = E.shape_request(self.items)
        self.by_shape = {s: np.flatnonzero(shape_of == j) for j, s in enumerate(shapes)}
        wild = self.items["subject_id"] == E.ID_WILDCARD
        plain = [s for s in shapes if s[3] == E.ELLIPSIS]
        # plain shapes with the most checks first; their wildcard-subject checks are kept apart
        self.plain = sorted(plain, key=lambda s: -np.count_nonzero(~wild[self.by_shape[s]]))
        self.userset = [s for s in shapes if s[3] != E.ELLIPSIS]
        self.wild = {s: [i for i in self.by_shape[s] if wild[i]] for s in plain}
        self.by_shape = {s: [i for i in idx if not wild[i]] for s, idx in self.by_shape.items()}
        self.pin = _Pinned(self.e, max(SIZES))
        self.cursor = {}

    def draw(self, shape, wildcard=False):
        src = self.wild[shape] if wildcard else self.by_shape[shape]
        k = self.cursor.get((shape, wildcard), 0)
        self.cursor[(shape, wildcard)] = k + 1
        return src[k % len(src)]

    def request(self, table, shape_of, wildcard_at=()):
        """Pool positions for a request whose check k has shape table[shape_of[k]]."""
        return [self.draw(table[s], k in wildcard_at) for k, s in enumerate(shape_of)]


@pytest.fixture(scope="module", params=["nested", "github", "gdocs"])
def pool(request):
    p = _Pool(request.param)
    yield p
    p.e.close()


def _run_pattern(pool, table, shape_of, what, pinned, wildcard_at=()):
    pos = pool.request(table, shape_of, wildcard_at)
    want = [pool.want[i] for i in pos]
    return pos, _check(pool.e, table, shape_of, pool.pairs[pos], want, pin=pool.pin if pinned else None, what=what)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_wave_and_block_edges(pool, pinned):
    e = pool.e
    plain, userset = pool.plain, pool.userset
    assert len(plain) >= 2 and userset
    three = (plain + userset)[:3]
    with_wild = next(s for s in plain if pool.wild[s])
    s0 = e.shaped_stats()
    for n in SIZES:
        # one shape: the uniform call's words and errors
        pos, (words, errs) = _run_pattern(pool, [plain[0]], [0] * n, "one shape", pinned)
        u_words, u_errs, _ = e.check_uniform(plain[0], pool.pairs[pos], now_us=NOW_US)
        assert np.array_equal(np.asarray(words), u_words) and errs.tolist() == u_errs.tolist()
        # two and three shapes alternating per check
        _run_pattern(pool, plain[:2], [k % 2 for k in range(n)], "two alternating", pinned)
        _run_pattern(pool, three, [k % 3 for k in range(n)], "three alternating", pinned)
        # the shape changing exactly at 16, 32 and 128
        steps = [(k >= 16) + (k >= 32) + (k >= 128) for k in range(n)]
        _run_pattern(pool, [three[j % 3] for j in range(4)], steps, "steps at 16/32/128", pinned)
        # a 64-entry table (entries repeated) used at 0, 31, 32, 63: lanes 32-63 load entries too
        table = [three[(j * 7 + j // 32) % 3] for j in range(64)]
        _run_pattern(pool, table, [(0, 31, 32, 63)[k % 4] for k in range(n)], "64 entries", pinned)
        # a userset shape and wildcard subject ids among plain checks: deferred beside decided
        mixed = [1 if k % 5 == 3 else 0 for k in range(n)]
        wild_at = {k for k in range(n) if k % 7 == 2 and mixed[k] == 0}
        _run_pattern(pool, [with_wild, userset[0]], mixed, "userset and wildcard", pinned, wild_at)
    assert e.shaped_stats()[0] >= s0[0] + 6 * len(SIZES) and e.shaped_stats()[1] == s0[1]


# ---- 3. a shape index beyond the table ----------------------------------------------------------

def _nested_request(n, seed=3, **kw):
    schema, tuples, _ = gen.nested(5, n_users=400, n_groups=160, n_docs=200)
    rng = np.random.default_rng(seed)
    checks = [f"doc:d{rng.integers(0, 205)}#view@user:u{rng.integers(0, 405)}" if rng.random() < 0.7 else
              f"doc:d{rng.integers(0, 205)}#view@group:g{rng.integers(0, 165)}#member" for _ in range(n)]
    e = _engine(schema, tuples, **kw)
    items = e.make_items([parse_check(c) for c in checks])
    shapes, shape_of, pairs = E.shape_request(items)
    assert len(shapes) == 2
    return e, schema, tuples, checks, shapes, shape_of, pairs


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("n,bad_at,kw", [(100, [5, 40], {}), (100, [97], {}), (5000, [4321, 3210], {"max_batch": 1000})],
                         ids=["first-wave", "last-partial-wave", "later-chunk"])
def test_bad_shape_index_fails_the_request(n, bad_at, kw, pinned):
    e, schema, tuples, checks, shapes, shape_of, pairs = _nested_request(n, **kw)
    pin = _Pinned(e, n) if pinned else None
    broken = shape_of.copy()
    broken[bad_at] = len(shapes)
    s0 = e.shaped_stats()
    with pytest.raises(E.GckError) as ei:
        if pinned:
            idx, prs, words = pin.load(broken, pairs)
            e.check_shaped(shapes, idx, prs, now_us=NOW_US, out_packed=words)
        else:
            e.check_shaped(shapes, broken, pairs, now_us=NOW_US)
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    assert f"shape_of[{min(bad_at)}]" in ei.value.message, ei.value.message
    assert e.shaped_stats()[0] > s0[0]  # (the join met the index: the device clamped it)
    # the engine answers the next request
    m = min(n, 300)
    _check(e, shapes, shape_of[:m], pairs[:m], _want(schema, tuples, checks[:m]), pin=pin)
    e.close()


# ---- 4. chunks above max_batch ------------------------------------------------------------------

def test_shaped_chunks_above_max_batch():
    e, schema, tuples, checks, shapes, shape_of, pairs = _nested_request(5000, seed=4, max_batch=1000)
    want = _want(schema, tuples, checks)
    _check(e, shapes, shape_of, pairs, want, pin=_Pinned(e, 5000), what="pinned")
    _check(e, shapes, shape_of, pairs, want, what="pageable")
    assert e.shaped_stats() == (2 * -(-5000 // 992), 0)  # chunks of max_batch rounded down to 32 checks
    e.close()
    e = _engine(schema, tuples, max_batch=1000, workspaces=1)
    _check(e, shapes, shape_of, pairs, want, pin=_Pinned(e, 5000), what="one workspace, pinned")
    _check(e, shapes, shape_of, pairs, want, what="one workspace, pageable")
    e.close()


# ---- 5. check contexts: the expanded path -------------------------------------------------------

def test_shaped_with_check_contexts():
    schema, tuples, checks = gen.FAMILIES["caveated"](2)
    e = _engine(schema, tuples)
    ctxs = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]
    slot = [1 + k % 2 for k in range(len(checks))]
    items = e.make_items([parse_check(c) for c in checks])
    items["context_slot"] = slot
    shapes, shape_of, pairs = E.shape_request(items)
    assert any(a[:4] == b[:4] and a[4] != b[4] for a in shapes for b in shapes)  # entries differing in the slot only
    want = _want(schema, tuples, checks, contexts=[ctxs[s - 1] for s in slot])
    assert len({w for w in want}) >= 2
    s0 = e.shaped_stats()
    _check(e, shapes, shape_of, pairs, want, contexts=ctxs)
    _check(e, shapes, shape_of, pairs, want, pin=_Pinned(e, len(checks)), contexts=[json.dumps(c) for c in ctxs])
    assert e.shaped_stats() == (s0[0], s0[1] + 2)
    e.close()


# ---- 6. the engine's other paths ----------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"labels": False}, {"closure": False, "labels": False}, {"wide_only": True},
                                {"profile": True}, {"resident": True, "workspaces": 8}],
                         ids=["no-labels", "no-join", "wide-only", "profiling", "resident"])
def test_shaped_on_every_engine_path(kw):
    family = "nested" if "resident" in kw else "gdocs"
    schema, tuples, checks = gen.FAMILIES[family](4)
    want = _want(schema, tuples, checks)
    e = _engine(schema, tuples, **kw)
    items = e.make_items([parse_check(c) for c in checks])
    shapes, shape_of, pairs = E.shape_request(items)
    assert len(shapes) >= 2
    pin = _Pinned(e, len(checks))
    for _ in range(2):  # (twice: the second request meets the workspace's table already written)
        _check(e, shapes, shape_of, pairs, want, pin=pin, what="pinned")
        _check(e, shapes, shape_of, pairs, want, what="pageable")
    # another table on the same workspace: its entries are rewritten
    rev = list(reversed(shapes))
    _check(e, rev, (len(shapes) - 1 - shape_of).astype(np.uint8), pairs, want, pin=pin, what="reversed table")
    e.close()


# ---- 7. in flight -------------------------------------------------------------------------------

def test_shaped_batches_in_flight(pool):
    e = pool.e
    rng = np.random.default_rng(11)
    table = (pool.plain + pool.userset)[:4]
    n, k = 1000, 24
    reqs = []
    for b in range(k):
        shape_of = rng.integers(0, len(table), n).astype(np.uint8)
        pos = pool.request(table, shape_of)
        buf = _Pinned(e, n)
        idx, pairs, words = buf.load(shape_of, pool.pairs[pos])
        errs = e.host_array(n, E.ITEM_ERROR_DTYPE)
        reqs.append((pos, idx, pairs, words, errs, buf))

    def verify(b, words, errs):
        wp, we = _expected([pool.want[i] for i in reqs[b][0]])
        assert E.unpack_results(words, n).tolist() == wp, b
        assert [(int(r["index"]), int(r["code"])) for r in errs] == we, b

    batches = [e.submit_shaped(table, r[1], r[2], r[3], r[4], now_us=NOW_US) for r in reqs[:8]]
    for b, sb in enumerate(batches):
        words, errs, rev = sb.wait()
        assert rev == e.revision
        verify(b, words, errs)
    for r in reqs:
        r[3][:] = POISON
    loop = e.prepare_shaped([table] * k, [r[1].ctypes.data for r in reqs], [r[2].ctypes.data for r in reqs], [n] * k,
                            [r[3].ctypes.data for r in reqs], [r[4].ctypes.data for r in reqs], n, 8, now_us=NOW_US)
    loop.run()
    for b, r in enumerate(reqs):
        verify(b, r[3], r[4][:loop.n_errs[b]])


# ---- 8. after a Watch batch ---------------------------------------------------------------------

def test_shaped_after_a_watch_batch():
    """Direct grants written and removed by a Watch batch: the label join's dirty subjects in the
    shaped mode, exact against the oracle of the updated relationships."""
    schema, tuples, checks = gen.gdocs(2)
    e = _engine(schema, tuples)
    rnd = random.Random(5)
    live = [t for t in tuples if t.startswith("doc:") and "#viewer@user:u" in t]
    ups = [("DELETE", t) for t in rnd.sample(live, 6)]
    ups += [("CREATE", f"doc:d{rnd.randrange(60)}#viewer@user:u{rnd.randrange(60)}") for _ in range(8)]
    ups = sorted({(op, t) for op, t in ups if op == "DELETE" or t not in tuples})
    store = [t for t in tuples if ("DELETE", t) not in ups] + [t for op, t in ups if op == "CREATE"]
    checks = checks + [t.replace("#viewer@", "#view@") for _, t in ups]
    items = e.make_items([parse_check(c) for c in checks])
    shapes, shape_of, pairs = E.shape_request(items)
    pin = _Pinned(e, len(checks))
    _check(e, shapes, shape_of, pairs, _want(schema, tuples, checks), pin=pin, what="before")
    e.apply_updates_text(2, "\n".join(f"{op} {t}" for op, t in ups))
    items = e.make_items([parse_check(c) for c in checks])  # (the batch may have created names)
    shapes, shape_of, pairs = E.shape_request(items)
    want = _want(schema, store, checks)
    s0 = e.shaped_stats()
    _check(e, shapes, shape_of, pairs, want, pin=pin, what="after, pinned")
    _check(e, shapes, shape_of, pairs, want, what="after, pageable")
    assert e.shaped_stats()[0] == s0[0] + 2
    e.close()


# ---- 9. the Client ------------------------------------------------------------------------------

def test_client_with_compact_requests():
    golden = load_golden("client_check.json")
    e = _engine(golden["schema"], golden["tuples"])
    plain, compact = Client(e), Client(e, WithCompactRequests())
    s0 = e.shaped_stats()
    for case in golden["cases"]:
        cs = consistency.Full() if case["consistency"] == "full" else consistency.MinLatency()
        rs = [parse_check(s) for s in case["checks"]]
        got = compact.Check(None, cs, *rs)
        assert got == plain.Check(None, cs, *rs), case["name"]
        assert got == (case["expected"], None), case["name"]
    # the first errored item: the prefix before it and the error (client/client.go:279-280)
    ok = parse_check("document:check_test1#view@user:bob")
    bad = [ok] * 3 + [parse_check("document:README#owner@user:bot")] + [ok] * 3
    r0, err0 = plain.Check(None, consistency.MinLatency(), *bad)
    r1, err1 = compact.Check(None, consistency.MinLatency(), *bad)
    assert r1 == r0 == [True, True, True]
    assert isinstance(err1, CheckItemError) and str(err1) == str(err0)
    assert compact.Check(None, consistency.MinLatency()) == ([], None)
    assert sum(e.shaped_stats()) > sum(s0)
    e.close()
