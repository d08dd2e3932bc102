"""List requests on the GPU (include/gck.h gck_check_bulk_list): one fixed id against an id list
or a range of ids under one header, the ids read in place by the joins (4 B per check, or none)
and answered as the uniform call's dense plane of 2-bit Permissionships; and the lookups among
candidates built on them (gck_lookup_resources_among / _subjects_among, Client.FilterResources /
FilterSubjects).

Bar: for every shape of every family the plane equals the oracle's Permissionship of every check
— 0 for an errored check, padding bits 0, every word written — the error list equals the oracle's
errored checks in ascending order, and both equal check_uniform on the expanded pairs; on pinned
and pageable buffers, on both sides, in list and range form, across chunks, on the expanded path
(a check context, GCK_AQL=0), through submit / wait and the compiled loop, on a resident engine,
and through the lookups and the client."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gochugaru_amd import consistency, rel
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client, InvalidArgument
from tests import gen
from tests.helpers import load_golden, oracle_for, parse_check, to_oracle_item
from tests.lookup_cases import WILD_SCHEMA

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF
CTXS = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]
R, S = E.VARY_RESOURCE, E.VARY_SUBJECT
FAMS = ["nested", "gdocs", "github", "hub_arrow", "cyclic", "near_budget", "caveated"]
MAX_DEPTH = 1  # GCK_ITEM_ERR_MAX_DEPTH


class _Family:
    """A family's graph, its oracle with every answer remembered, and its checks grouped by shape:
    (resource type, permission, subject type, subject relation) -> the distinct resource names and
    subject names occurring in them, first seen first (at most 200 of each)."""

    def __init__(self, name, seed=2):
        self.schema, self.tuples, self.checks = gen.FAMILIES[name](seed)
        self.depth = gen.FAMILY_DEPTH.get(name, 50)
        self.ck = oracle_for(self.schema, self.tuples, max_depth=self.depth, now=NOW_US / 1e6)
        self.memo = {}
        self.shapes = {}
        for c in self.checks:
            r = parse_check(c)
            res, sub = self.shapes.setdefault((r.ResourceType, r.ResourceRelation, r.SubjectType, r.SubjectRelation),
                                              ({}, {}))
            res.setdefault(r.ResourceID), sub.setdefault(r.SubjectID)
        for k, (res, sub) in self.shapes.items():
            self.shapes[k] = (list(res)[:200], list(sub)[:200])

    def one(self, shape, sn, rn, ctx=None):
        rt, perm, st, srel = shape
        k = (shape, sn, rn, json.dumps(ctx, sort_keys=True))
        if k not in self.memo:
            self.memo[k] = tuple(self.ck.check(to_oracle_item(
                rel.FromTriple(f"{rt}:{rn}", perm, f"{st}:{sn}" + (f"#{srel}" if srel else "")), ctx)))
        return self.memo[k]

    def want(self, shape, fixed, vary, names, ctx=None):
        """(perm[n] with 0 for an errored check, [(index, code)] ascending) of `fixed` against names."""
        out = np.zeros(len(names), dtype=np.uint8)
        errs = []
        for i, nm in enumerate(names):
            p, e = self.one(shape, fixed, nm, ctx) if vary == R else self.one(shape, nm, fixed, ctx)
            if e:
                errs.append((i, e))
            else:
                out[i] = p
        return out, errs

    def engine(self, **kw):
        e = E.Engine(device=0, max_depth=self.depth, **kw)
        e.load_schema(self.schema)
        e.load_snapshot_text(1, "\n".join(self.tuples))
        return e


_FAMILIES = {}


def _family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = _Family(name)
    return _FAMILIES[name]


def _header(e, shape):
    rt, perm, st, srel = shape
    t_r, t_s = e.type_id(rt), e.type_id(st)
    return (t_r, e.relation_id(t_r, perm), t_s, E.ELLIPSIS if srel in ("", "...") else e.relation_id(t_s, srel))


def _intern(e, t, names):
    """Ids as a caller interns them (an unknown name or type: ABSENT; "*": the wildcard)."""
    if t == E.TYPE_INVALID:
        return np.array([E.ID_WILDCARD if n == "*" else E.ID_ABSENT for n in names], dtype=np.uint32)
    return np.asarray(e.intern(t, list(names)), dtype=np.uint32)


def _dense(perm):
    """The dense plane of perm[n]: padding bits 0."""
    words = np.zeros((len(perm) + 31) // 32, dtype=np.uint64)
    for i, p in enumerate(perm):
        words[i // 32] |= np.uint64(int(p) << (2 * (i % 32)))
    return words


def _records(errs):
    return [(int(x["index"]), int(x["code"])) for x in errs]


def _exact(e, fam, shape, fixed, vary, names, pinned=False, contexts=None, slot=0, uniform=True, first=None):
    """One list request against the oracle and against check_uniform on the expanded pairs.
    first: send it as the range first .. first + len(names) - 1 (names are then those ids' names)."""
    hdr = _header(e, shape)
    fid = int(_intern(e, hdr[2] if vary == R else hdr[0], [fixed])[0])
    ids = _intern(e, hdr[0] if vary == R else hdr[2], names)
    n = len(names)
    n_words = (n + 31) // 32
    words = e.host_array(n_words, np.uint64) if pinned else np.zeros(n_words, dtype=np.uint64)
    words[:] = POISON  # every word must be written
    if first is None:
        src = ids
        if pinned:
            src = e.host_array(n, np.uint32)
            src[:] = ids
        out, errs, rev = e.check_list(hdr + (slot,), fid, vary, src, now_us=NOW_US, contexts=contexts, out_packed=words)
    else:
        assert list(ids) == list(range(first, first + n))
        out, errs, rev = e.check_list(hdr + (slot,), fid, vary, None, first, n, now_us=NOW_US, contexts=contexts,
                                      out_packed=words)
    assert rev == e.revision
    wp, we = fam.want(shape, fixed, vary, names, contexts[slot - 1] if slot else None)
    got = E.unpack_results(out, n)
    bad = [(fixed, names[i], int(wp[i]), int(got[i])) for i in np.nonzero(wp != got)[0]]
    assert not bad, (shape, vary, n, bad[:5])
    rec = _records(errs)
    assert rec == we and rec == sorted(rec), shape
    assert np.array_equal(np.asarray(out), _dense(wp)), "padding bits or unwritten words"
    if uniform:
        fx = np.full(n, fid, dtype=np.uint32)
        pairs = np.stack([ids, fx] if vary == R else [fx, ids], axis=1).astype(np.uint32)
        uw, uerrs, _ = e.check_uniform(hdr + (slot,), pairs, now_us=NOW_US, contexts=contexts)
        assert np.array_equal(E.unpack_results(uw, n), got)
        assert _records(uerrs) == rec
    return got, rec


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("family", FAMS)
def test_list_matches_oracle(family, pinned):
    fam = _family(family)
    e = fam.engine()
    e.reset_stats()
    assert len(fam.shapes) >= 2
    for shape, (res, sub) in fam.shapes.items():
        _exact(e, fam, shape, sub[0], R, res, pinned=pinned)
        _exact(e, fam, shape, res[0], S, sub, pinned=pinned)
    if family in ("nested", "gdocs", "github"):  # the joins read the lists in place
        assert e.list_stats()[0] > 0 and e.stats()["aql_batches"] > 0
    e.close()


def _cycle(xs, n):
    return [xs[k % len(xs)] for k in range(n)]


@pytest.mark.parametrize("family,sizes", [("nested", (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)),
                                          ("gdocs", (1, 16, 17, 32, 33, 129)), ("github", (1, 16, 17, 32, 33, 129))])
def test_list_edges(family, sizes):
    """A lone lane, half waves, the closure join's 64-check two-word waves and the label join's
    16- and 32-check waves, a block plus one; names repeated in a cycle (ids are not deduplicated)."""
    fam = _family(family)
    e = fam.engine()
    shape = ("doc", "view", "user", "") if family == "nested" else next(iter(fam.shapes))
    res, sub = fam.shapes[shape]
    k = 0
    for n in sizes:
        _exact(e, fam, shape, sub[n % len(sub)], R, _cycle(res, n), pinned=(n % 2 == 0), uniform=False)
        _exact(e, fam, shape, res[n % len(res)], S, _cycle(sub, n), pinned=(n % 2 == 1), uniform=False)
        k += 2
    assert e.list_stats() == (k, 0)
    e.close()


def _type_names(e, type_name):
    t = e.type_id(type_name)
    return [e.object_name(t, i) for i in range(e.object_count(t))]


@pytest.mark.parametrize("family", ["nested", "gdocs"])
def test_list_range(family):
    fam = _family(family)
    e = fam.engine()
    shape = ("doc", "view", "user", "") if family == "nested" else next(iter(fam.shapes))
    names = _type_names(e, shape[0])
    n = len(names)
    assert n > 55
    sub = fam.shapes[shape][1][0]
    as_range, rerr = _exact(e, fam, shape, sub, R, names, first=0, pinned=True)
    as_list, lerr = _exact(e, fam, shape, sub, R, names, uniform=False)
    assert np.array_equal(as_range, as_list) and rerr == lerr
    # a first id that is no multiple of 32 and a count that is none either; a range ending with the type's last object
    _exact(e, fam, shape, sub, R, names[5:5 + 45], first=5)
    _exact(e, fam, shape, sub, R, names[n - 33:], first=n - 33)
    assert e.list_stats()[1] == 0
    e.close()


@pytest.mark.parametrize("kw", [{"workspaces": 1}, {}], ids=["one_workspace", "default"])
def test_list_chunks(kw):
    fam = _family("nested")
    e = fam.engine(max_batch=64, **kw)
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    hdr = _header(e, shape)
    names = _cycle(res, 500)
    ids = e.host_array(500, np.uint32)
    ids[:] = _intern(e, hdr[0], names)
    fid = int(_intern(e, hdr[2], [sub[0]])[0])
    wp, we = fam.want(shape, sub[0], R, names)
    out, errs, _ = e.check_list(hdr, fid, R, ids, now_us=NOW_US)
    ids[:] = 0  # (the call has returned: the list is the caller's again)
    assert np.array_equal(out, _dense(wp)) and _records(errs) == we
    assert e.list_stats() == (8, 0)
    # a range of 500 from a first id that is no multiple of 32: 8 chunks, each with its own first id. nested
    # has fewer doc objects than that, so most of the range lies past the type's last object — legal, and
    # answered as a nonexistent object is (the oracle's answer for an unknown name; check_uniform's for the ids)
    tnames = _type_names(e, "doc")
    first, n = 3, 500
    assert first + 64 < len(tnames) < first + n
    rn = [tnames[i] if i < len(tnames) else "no_object_of_this_name" for i in range(first, first + n)]
    # (a subject with a HAS in the first chunk, by the oracle: a later chunk that repeated that chunk's ids,
    # instead of being all NO past the type's end, would show)
    sn = next(x for x in sub if (fam.want(shape, x, R, rn[:64])[0] == E.PERM_HAS).any())
    rfid = int(_intern(e, hdr[2], [sn])[0])
    rp, rerr = fam.want(shape, sn, R, rn)
    words = e.host_array((n + 31) // 32, np.uint64)
    words[:] = POISON
    before = e.list_stats()
    out, errs, _ = e.check_list(hdr, rfid, R, None, first, n, now_us=NOW_US, out_packed=words)
    assert e.list_stats() == (before[0] + 8, before[1]) == (16, 0)
    assert np.array_equal(np.asarray(out), _dense(rp)) and _records(errs) == rerr
    pairs = np.stack([np.arange(first, first + n, dtype=np.uint32), np.full(n, rfid, dtype=np.uint32)], axis=1)
    uw, uerrs, _ = e.check_uniform(hdr, pairs, now_us=NOW_US)
    assert np.array_equal(np.asarray(out), uw) and _records(errs) == _records(uerrs)
    # a submitted chunk's pinned list is the caller's again once the wait has returned
    ids[:64] = _intern(e, hdr[0], names[:64])
    words = e.host_array(2, np.uint64)
    words[:] = POISON
    b = e.submit_list(hdr, fid, R, words, np.zeros(4, dtype=E.ITEM_ERROR_DTYPE), ids[:64], now_us=NOW_US)
    w, er, _ = b.wait()
    ids[:] = 0
    assert np.array_equal(np.asarray(w), _dense(wp[:64])) and len(er) == 0
    e.close()


def _budget_case(fam, e, want_code=MAX_DEPTH):
    """(shape, subject, names of the whole resource type) whose sweep meets the depth budget, by the oracle."""
    for shape, (res, sub) in fam.shapes.items():
        names = _type_names(e, shape[0])
        for sn in sub[:12]:
            if any(c == want_code for _, c in fam.want(shape, sn, R, names)[1]):
                return shape, sn, names
    return None


@pytest.mark.parametrize("family", ["near_budget", "cyclic"])
def test_list_deferred_checks_come_back(family):
    """Checks the join leaves to the bundle stages: their results and their depth-budget errors at
    the right indices, in list and in range form (expected values: the oracle's)."""
    fam = _family(family)
    e = fam.engine()
    case = _budget_case(fam, e)
    if family == "near_budget":
        assert case is not None, "near_budget has no check at the depth budget"
    shapes = [case[:2]] if case else []
    shapes += [(shape, sub[0]) for shape, (res, sub) in fam.shapes.items()]
    for shape, sn in shapes:
        names = _type_names(e, shape[0])
        a, ea = _exact(e, fam, shape, sn, R, names, first=0, uniform=False)
        order = list(reversed(names))
        b, eb = _exact(e, fam, shape, sn, R, order, pinned=True)
        assert np.array_equal(a, b[::-1]) and sorted((len(names) - 1 - i, c) for i, c in eb) == ea
        res0 = fam.shapes[shape][0][0]
        _exact(e, fam, shape, res0, S, _type_names(e, shape[2]) if e.type_id(shape[2]) != E.TYPE_INVALID else ["x"])
    if family == "near_budget":  # its join reads the requests in place and leaves checks: the items were rebuilt
        assert e.list_stats()[0] > 0 and e.list_stats()[1] == 0 and e.stats()["deferred"] > 0
    e.close()


def test_list_ids_beyond_the_type():
    """nested, read in place: ids no slot holds — ABSENT entries in the middle of a wave, a range
    that passes the type's last object — index nothing and are answered as check_uniform answers
    them."""
    fam = _family("nested")
    e = fam.engine()
    e.reset_stats()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    hdr = _header(e, shape)
    names = _cycle(res, 100)
    for at in (0, 31, 32, 40, 99):
        names[at] = "no_object_of_this_name"
    _exact(e, fam, shape, sub[0], R, names, pinned=True)
    subs = _cycle(sub, 70)
    subs[1] = subs[64] = "nobody_of_that_name"
    _exact(e, fam, shape, res[0], S, subs)
    n_doc = e.object_count(hdr[0])
    fid = int(_intern(e, hdr[2], [sub[0]])[0])
    out, errs, _ = e.check_list(hdr, fid, R, None, n_doc - 10, 50, now_us=NOW_US)
    far = np.stack([np.arange(n_doc - 10, n_doc + 40, dtype=np.uint32), np.full(50, fid, dtype=np.uint32)], axis=1)
    uw, uerrs, _ = e.check_uniform(hdr, far, now_us=NOW_US)
    assert np.array_equal(out, uw) and _records(errs) == _records(uerrs)
    assert e.list_stats() == (3, 0)
    e.close()


def test_list_with_a_check_context():
    """A header context slot: check contexts force the expansion to items; exact under the context."""
    fam = _family("caveated")
    e = fam.engine()
    before = e.list_stats()
    for shape, (res, sub) in fam.shapes.items():
        _exact(e, fam, shape, sub[0], R, res[:40], contexts=CTXS, slot=1)
        _exact(e, fam, shape, res[0], S, sub[:40], contexts=CTXS, slot=1, pinned=True)
    after = e.list_stats()
    assert after[1] > before[1] and after[0] == before[0]
    e.close()


_AQL0_PROBE = """
import json, sys
sys.path.insert(0, {root!r})
import numpy as np
from tests import test_gpu_list as T
fam = T._family("nested")
e = fam.engine(max_batch=128)
shape = ("doc", "view", "user", "")
res, sub = fam.shapes[shape]
T._exact(e, fam, shape, sub[0], T.R, T._cycle(res, 300), pinned=True)
T._exact(e, fam, shape, res[0], T.S, T._cycle(sub, 300))
rn = T._type_names(e, "doc")[5:205]
T._exact(e, fam, shape, sub[0], T.R, rn, first=5, uniform=False)
print(json.dumps({{"stats": e.list_stats(), "chunks": 3 + 3 + (len(rn) + 127) // 128, "aql": int(e.stats()["aql_batches"])}}))
"""


def test_list_without_aql():
    """GCK_AQL=0 (read once per process: a child): every chunk is expanded, and stays exact."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GCK_AQL="0")
    r = subprocess.run([sys.executable, "-c", _AQL0_PROBE.format(root=root)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["stats"] == [0, out["chunks"]] and out["chunks"] > 6 and out["aql"] == 0, out


def test_list_request_errors():
    fam = _family("nested")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    hdr = _header(e, shape)
    ids = _intern(e, hdr[0], res[:40])
    fid = int(_intern(e, hdr[2], [sub[0]])[0])

    def good():
        _exact(e, fam, shape, sub[0], R, res[:40], uniform=False)

    def refused(*a, **kw):
        with pytest.raises(E.GckError) as ei:
            e.check_list(*a, **kw)
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value
        good()

    good()
    for vary in (0, 3, 7):
        refused(hdr, fid, vary, ids)
    refused(E.Uniform(*hdr, 0, 1), fid, R, ids)            # reserved != 0
    refused(hdr + (1,), fid, R, ids)                       # a context slot without contexts
    refused(hdr + (3,), fid, R, ids, contexts=CTXS)        # ... beyond the contexts
    refused(hdr, fid, R, None, 0xFFFFFFF0, 17)             # first_id + n > 2^32
    refused(hdr, fid, S, None, 0, 8)                       # a range varies the resource id
    # null outputs with n > 0 (the raw call: the wrapper always passes buffers)
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    h = E.Uniform(*hdr, 0, 0)
    n_errs, rev = C.c_size_t(7), C.c_uint64(0)
    rc = e._lib.gck_check_bulk_list(e._h, C.byref(cs), C.byref(h), fid, R, ids.ctypes.data, 0, len(ids), None, None, 0,
                                    NOW_US, None, None, 0, C.byref(n_errs), C.byref(rev))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    rc = e._lib.gck_check_bulk_list(e._h, C.byref(cs), C.byref(h), fid, R, ids.ctypes.data, 0, len(ids), None, None, 0,
                                    NOW_US, np.zeros(2, dtype=np.uint64).ctypes.data, None, 4, C.byref(n_errs),
                                    C.byref(rev))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    good()
    # n == 0 succeeds and writes nothing: list form, range form (a range at the very end included)
    w = np.full(1, POISON, dtype=np.uint64)
    for args in ((np.zeros(0, dtype=np.uint32),), (None, 0xFFFFFFFF, 0), (None, 5, 0)):
        out, errs, rev = e.check_list(hdr, fid, R, *args, out_packed=w[:0])
        assert len(out) == 0 and len(errs) == 0 and rev == e.revision
    assert w[0] == POISON
    # the last range that fits: ids far beyond the type's objects, answered as the uniform call answers them
    out, errs, _ = e.check_list(hdr, fid, R, None, 0xFFFFFFF0, 16, now_us=NOW_US)
    far = np.stack([np.arange(0xFFFFFFF0, 0x100000000, dtype=np.uint64).astype(np.uint32),
                    np.full(16, fid, dtype=np.uint32)], axis=1)
    uw, uerrs, _ = e.check_uniform(hdr, far, now_us=NOW_US)
    assert np.array_equal(out, uw) and _records(errs) == _records(uerrs)
    good()
    e.close()


def test_list_submit_and_wait():
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    hdr = _header(e, shape)
    tnames = _type_names(e, "doc")
    reqs = []
    for k in range(8):  # eight in flight on eight workspaces: lists of both sides and ranges
        n = 30 + 13 * k
        vary = S if k % 3 == 1 else R
        first = None
        if k % 3 == 2:
            first = 7 * k
            names = tnames[first:first + n]
            n = len(names)
            assert n > 0
        else:
            names = [(sub_all if vary == S else res_all)[(5 * k + j) % len(sub_all if vary == S else res_all)]
                     for j in range(n)]
        fixed = (res_all if vary == S else sub_all)[k]
        fid = int(_intern(e, hdr[0] if vary == S else hdr[2], [fixed])[0])
        words = e.host_array((n + 31) // 32, np.uint64)
        words[:] = POISON
        errs = np.zeros(16, dtype=E.ITEM_ERROR_DTYPE)
        ids = None if first is not None else _intern(e, hdr[2] if vary == S else hdr[0], names)
        b = e.submit_list(hdr, fid, vary, words, errs, ids, first or 0, n, now_us=NOW_US)
        if ids is not None:
            ids[:] = 0  # (a pageable list was copied by the call)
        reqs.append((b, fixed, vary, names))
    for b, fixed, vary, names in reqs:
        words, errs, rev = b.wait()
        wp, we = fam.want(shape, fixed, vary, names)
        assert rev == e.revision and _records(errs) == we
        assert np.array_equal(np.asarray(words), _dense(wp))
    # a submitted request above max_batch is refused, and the engine goes on
    e2 = fam.engine(max_batch=64)
    with pytest.raises(E.GckError) as ei:
        e2.submit_list(_header(e2, shape), 0, R, np.zeros(3, dtype=np.uint64), np.zeros(4, dtype=E.ITEM_ERROR_DTYPE),
                       None, 0, 65)
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    _exact(e2, fam, shape, sub_all[0], R, res_all[:64])
    e2.close()
    e.close()


def test_list_compiled_loop():
    """gckd_run_list: 50 requests of 1,024 checks, 8 in flight, pinned lists and planes, every one
    read in place; the answers are check_uniform's."""
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    hdr = _header(e, shape)
    rid_all, sid_all = _intern(e, hdr[0], res_all), _intern(e, hdr[2], sub_all)
    n_doc = e.object_count(hdr[0])
    k, n = 50, 1024
    fixed, lists, first, planes, errs, want = [], [], [], [], [], []
    for b in range(k):
        fid = int(sid_all[b % len(sid_all)])
        fixed.append(fid)
        if b % 5 == 4:  # a range (it may pass the type's last object: answered as the uniform call does)
            f0 = (37 * b) % max(1, n_doc)
            ids = np.arange(f0, f0 + n, dtype=np.uint32)
            lists.append(None), first.append(f0)
        else:
            ids = e.host_array(n, np.uint32)
            ids[:] = rid_all[(np.arange(n) * 3 + b) % len(rid_all)]
            lists.append(ids), first.append(0)
        pairs = np.stack([np.asarray(ids), np.full(n, fid, dtype=np.uint32)], axis=1).astype(np.uint32)
        want.append(e.check_uniform(hdr, pairs, now_us=NOW_US))
        w = e.host_array(n // 32, np.uint64)
        w[:] = POISON
        planes.append(w), errs.append(e.host_array(8, E.ITEM_ERROR_DTYPE))
    before = e.list_stats()
    p = e.prepare_list([hdr] * k, fixed, R, [0 if x is None else x.ctypes.data for x in lists], first, [n] * k,
                       [x.ctypes.data for x in planes], [x.ctypes.data for x in errs], 8, 8, now_us=NOW_US)
    assert p.run() > 0
    for b in range(k):
        uw, uerrs, _ = want[b]
        assert np.array_equal(np.asarray(planes[b]), uw), b
        assert p.n_errs[b] == len(uerrs) == 0
    assert e.list_stats() == (before[0] + k, before[1])
    e.close()


def test_list_on_a_resident_engine():
    """GCK_FLAG_RESIDENT: a list batch is dispatched normally, and stays exact."""
    fam = _family("nested")
    e = fam.engine(resident=True, workspaces=8)
    e.reset_stats()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    _exact(e, fam, shape, sub[1], R, _cycle(res, 70), uniform=False)
    _exact(e, fam, shape, res[1], S, _cycle(sub, 70), pinned=True, uniform=False)
    _exact(e, fam, shape, sub[1], R, _type_names(e, "doc")[3:90], first=3, uniform=False)
    st = e.stats()
    assert e.list_stats() == (3, 0) and st["resident_batches"] == 0 and st["aql_batches"] == 3
    e.close()


# ---- lookups among candidates ---------------------------------------------------------------

def _outcome(fn):
    try:
        ids, perms = fn()
        return [int(i) for i in ids], [int(p) for p in perms]
    except E.GckError as err:
        return err.code, str(err)


@pytest.mark.parametrize("family", FAMS)
def test_lookup_resources_among(family):
    fam = _family(family)
    e = fam.engine()
    rng = np.random.default_rng(5)
    for shape, (res, sub) in fam.shapes.items():
        hdr = _header(e, shape)
        if E.TYPE_INVALID in hdr[::2] or E.REL_INVALID in hdr[1::2]:
            continue
        names = _type_names(e, shape[0])
        for sn in sub[:2]:
            sid = int(_intern(e, hdr[2], [sn])[0])
            old = _outcome(lambda: e.lookup_resources(*hdr, sid, now_us=NOW_US))
            new = _outcome(lambda: e.lookup_resources_among(*hdr, sid, None, now_us=NOW_US))
            assert new == old, (shape, sn)
            # a shuffled candidate list with duplicates and ABSENT entries, most of it not matching
            wp_all, we_all = fam.want(shape, sn, R, names)
            yes = [i for i in range(len(names)) if wp_all[i] in (E.PERM_HAS, E.PERM_CONDITIONAL)]
            errored = {i for i, _ in we_all}
            no = [i for i in range(len(names)) if wp_all[i] == E.PERM_NO and i not in errored]
            pick = yes[:5] + yes[:2] + no[:3 * len(yes[:7]) + 9]
            rng.shuffle(pick)
            cand = [int(i) for i in pick]
            for at in (len(cand) // 3, len(cand)):
                cand.insert(at, E.ID_ABSENT)
            absent = fam.one(shape, sn, "no_object_of_this_name")
            got = _outcome(lambda: e.lookup_resources_among(*hdr, sid, np.array(cand, dtype=np.uint32), now_us=NOW_US))
            exp = [(c, int(wp_all[c]) if c != E.ID_ABSENT else absent[0]) for c in cand]
            exp = [(c, p) for c, p in exp if p in (E.PERM_HAS, E.PERM_CONDITIONAL)]
            assert got == ([c for c, _ in exp], [p for _, p in exp]), (shape, sn)
    e.close()


def test_lookup_subjects_among_wildcards():
    """WILD_SCHEMA: a wildcard grant makes every candidate match — an unknown name too — and no "*"
    is reported; exclusions and intersections still apply. Expected values: the oracle's."""
    tuples = ["doc:d#viewer@user:*", "doc:d#banned@user:bob", "doc:d#viewer@user:bob", "doc:d#member@user:tom",
              "doc:e#viewer@user:ann", "doc:e#viewer@group:g#member", "group:g#member@user:amy",
              "doc:f#viewer@user:*[tuesday]", "doc:f#viewer@user:tom"]
    ck = oracle_for(WILD_SCHEMA, tuples, now=NOW_US / 1e6)
    e = E.Engine(device=0)
    e.load_schema(WILD_SCHEMA)
    e.load_snapshot_text(1, "\n".join(tuples))
    t_doc, t_user = e.type_id("doc"), e.type_id("user")
    cands = ["tom", "bob", "nobody_of_that_name", "amy", "ann", "bob", "tom"]
    ids = _intern(e, t_user, cands)
    assert ids[2] == E.ID_ABSENT
    for doc in ("d", "e", "f"):
        for perm in ("view", "view_unbanned", "view_member"):
            want = [ck.check(to_oracle_item(rel.FromTriple(f"doc:{doc}", perm, f"user:{c}"))) for c in cands]
            assert all(err == 0 for _, err in want)
            exp = [(int(i), p) for i, (p, _) in zip(ids, want) if p in (E.PERM_HAS, E.PERM_CONDITIONAL)]
            got_ids, got_perms = e.lookup_subjects_among(t_doc, int(e.intern(t_doc, [doc])[0]), e.relation_id(t_doc, perm),
                                                         t_user, ids, now_us=NOW_US)
            assert ([int(i) for i in got_ids], [int(p) for p in got_perms]) == ([i for i, _ in exp], [p for _, p in exp])
            assert E.ID_WILDCARD not in [int(i) for i in got_ids]
    # d#view: the wildcard grants everyone, the unknown name included
    got_ids, _ = e.lookup_subjects_among(t_doc, int(e.intern(t_doc, ["d"])[0]), e.relation_id(t_doc, "view"), t_user, ids)
    assert list(got_ids) == list(ids)
    # a candidate list is required; an empty one yields nothing
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    n = C.c_size_t(0)
    rc = e._lib.gck_lookup_subjects_among(e._h, C.byref(cs), t_doc, 0, e.relation_id(t_doc, "view"), t_user, E.ELLIPSIS,
                                          None, 3, NOW_US, None, None, 0, C.byref(n))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    got_ids, _ = e.lookup_subjects_among(t_doc, 0, e.relation_id(t_doc, "view"), t_user, np.zeros(0, dtype=np.uint32))
    assert len(got_ids) == 0
    e.close()


def test_lookup_among_capacity_protocol():
    fam = _family("nested")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    hdr = _header(e, shape)
    names = _type_names(e, "doc")
    sn = next(s for s in fam.shapes[shape][1]
              if sum(p in (E.PERM_HAS, E.PERM_CONDITIONAL) for p in fam.want(shape, s, R, names)[0]) >= 2)
    sid = int(_intern(e, hdr[2], [sn])[0])
    full_ids, full_perms = e.lookup_resources(*hdr, sid, now_us=NOW_US)
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    for cand in (None, np.asarray(list(full_ids) + [E.ID_ABSENT] + list(full_ids), dtype=np.uint32)):
        exp = list(full_ids) if cand is None else list(full_ids) * 2
        n = C.c_size_t(0)
        ids, perms = np.zeros(len(exp), dtype=np.uint32), np.zeros(len(exp), dtype=np.uint8)
        args = (e._h, C.byref(cs), *hdr, sid, None if cand is None else cand.ctypes.data, 0 if cand is None else len(cand),
                NOW_US)
        s0 = e.list_stats()
        rc = e._lib.gck_lookup_resources_among(*args, ids.ctypes.data, perms.ctypes.data, 1, C.byref(n))
        assert rc == E.GCK_E_CAPACITY and n.value == len(exp)
        s1 = e.list_stats()
        assert s1[0] > s0[0]
        rc = e._lib.gck_lookup_resources_among(*args, ids.ctypes.data, perms.ctypes.data, len(exp), C.byref(n))
        assert rc == 0 and n.value == len(exp) and list(ids) == exp
        assert e.list_stats() == s1  # the kept result: no second sweep
        rc = e._lib.gck_lookup_resources_among(*args, ids.ctypes.data, perms.ctypes.data, len(exp), C.byref(n))
        assert rc == 0 and list(ids) == exp and e.list_stats()[0] > s1[0]  # (dropped once copied out)
    e.close()


def test_lookup_among_fails_at_the_depth_budget():
    fam = _family("near_budget")
    e = fam.engine()
    case = _budget_case(fam, e)
    assert case is not None
    shape, sn, names = case
    hdr = _header(e, shape)
    sid = int(_intern(e, hdr[2], [sn])[0])
    old = _outcome(lambda: e.lookup_resources(*hdr, sid, now_us=NOW_US))
    assert old[0] == E.GCK_E_INVALID_ARGUMENT and "max depth" in old[1]
    assert _outcome(lambda: e.lookup_resources_among(*hdr, sid, None, now_us=NOW_US)) == old
    at = next(i for i, c in fam.want(shape, sn, R, names)[1] if c == MAX_DEPTH)
    cand = np.array([0, at, 1], dtype=np.uint32)
    assert _outcome(lambda: e.lookup_resources_among(*hdr, sid, cand, now_us=NOW_US)) == old
    e.close()


# ---- the client ----------------------------------------------------------------------------

def _names(it):
    out = list(it)
    assert all(err is None for _, err in out), out
    return [n for n, _ in out]


def _error(it):
    out = list(it)
    assert len(out) == 1 and out[0][0] == "" and out[0][1] is not None, out
    return out[0][1]


def test_client_filter_founders():
    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(3, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jimmy", "user:nobody_of_that_name", "user:jake", "user:jimmy", "user:joey"]
    flat, err = c.Check(None, cs, *[rel.MustFromTriple("company:authzed", "founder", s) for s in subjects])
    assert err is None
    assert _names(c.FilterSubjects(None, cs, "company:authzed", "founder", subjects)) == \
        [s.split(":")[1] for s, ok in zip(subjects, flat) if ok]
    assert flat == [True, False, True, True, True]
    resources = ["company:no_such_company", "company:authzed", "company:authzed"]
    assert _names(c.FilterResources(None, cs, "company#founder", "user:jake", resources)) == ["authzed", "authzed"]
    assert _names(c.FilterResources(None, cs, "company#founder", "user:nobody_of_that_name", resources)) == []
    assert _names(c.FilterResources(None, cs, "company#founder", "user:jake", [])) == []
    assert _names(c.FilterSubjects(None, cs, "company:authzed", "founder", [])) == []
    assert isinstance(_error(c.FilterResources(None, cs, "company#founder", "user:jake", ["company:authzed", "user:jake"])),
                      InvalidArgument)
    assert isinstance(_error(c.FilterSubjects(None, cs, "company:authzed", "founder", ["user:jake", "company:authzed"])),
                      InvalidArgument)
    # AtLeast on a revision the engine has not reached: Unavailable without retries, as Check ...
    ctx = consistency.Context(metadata={})
    object.__setattr__(ctx, "deadline", 0)
    err = _error(c.FilterSubjects(ctx, consistency.AtLeast("4"), "company:authzed", "founder", subjects))
    _, cerr = c.Check(ctx, consistency.AtLeast("4"), rel.MustFromTriple("company:authzed", "founder", "user:jake"))
    assert isinstance(err, E.GckError) and err.code == E.GCK_E_REVISION == cerr.code
    # ... and retried until the snapshot gets there: the first attempt fails, the Watch batch lands, the second answers
    real, calls = e.lookup_subjects_among, []

    def flaky(*a, **kw):
        calls.append(1)
        try:
            return real(*a, **kw)
        except E.GckError:
            e.apply_updates_text(4, "DELETE company:authzed#founder@user:jake")
            raise

    e.lookup_subjects_among = flaky
    assert _names(c.FilterSubjects(None, consistency.AtLeast("4"), "company:authzed", "founder", subjects)) == \
        ["jimmy", "jimmy", "joey"]
    assert len(calls) == 2
    del e.lookup_subjects_among
    e.close()


def test_client_filter_gdocs():
    fam = _family("gdocs")
    e = fam.engine()
    c = Client(e)
    cs = consistency.MinLatency()
    n_shapes = 0
    for shape, (res, sub) in fam.shapes.items():
        rt, perm, st, srel = shape
        tail = f"#{srel}" if srel else ""
        resources = [f"{rt}:{r}" for r in _cycle(res, 45)] + [f"{rt}:no_object_of_this_name"]
        subject = f"{st}:{sub[0]}{tail}"
        wp, we = fam.want(shape, sub[0], R, [r.split(":", 1)[1] for r in resources])
        if we or fam.want(shape, res[0], S, _cycle(sub, 45))[1]:
            continue  # (a shape whose checks have per-item errors: test_lookup_among_* covers those)
        n_shapes += 1
        flat, err = c.Check(None, cs, *[rel.MustFromTriple(r, perm, subject) for r in resources])
        assert err is None
        # (Check is True for HAS; the filters keep CONDITIONAL too, as LookupResources does)
        keep = [p in (E.PERM_HAS, E.PERM_CONDITIONAL) for p in wp]
        assert [bool(p == E.PERM_HAS) for p in wp] == flat
        assert _names(c.FilterResources(None, cs, f"{rt}#{perm}", subject, resources)) == \
            [r.split(":", 1)[1] for r, k in zip(resources, keep) if k]
        subjects = [f"{st}:{s}{tail}" for s in _cycle(sub, 45)]
        wp, we = fam.want(shape, res[0], S, _cycle(sub, 45))
        assert not we
        assert _names(c.FilterSubjects(None, cs, f"{rt}:{res[0]}", perm, subjects)) == \
            [s for s, p in zip(_cycle(sub, 45), wp) if p in (E.PERM_HAS, E.PERM_CONDITIONAL)]
    assert n_shapes >= 2
    e.close()
