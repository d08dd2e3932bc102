"""Cross requests on the GPU (include/gck.h gck_check_bulk_cross): every subject of one id list
against every resource of another under one header, read in place by the joins from the
workspace's id block and answered as a row-padded plane of 2-bit Permissionships.

Bar: for every shape of every family the plane equals the oracle's Permissionship of every
(subject, resource) — 0 for an errored check, padding bits 0, every word written — the error list
equals the oracle's errored checks in ascending s * R + r, and both equal check_uniform on the
expanded pairs; on pinned and pageable planes, across tiles, on the expanded path (check
contexts, a thin request), through submit / wait and the compiled loop, and through
Client.CheckCross.

One case of the issue does not hold as it was written: max_batch=64, S=1, R=500 is cut into eight
1 x 64 tiles by the tiling rule (a 64-check tile is not below max_batch / 4 = 16), so it is no
thin request. The test keeps the case, bit-exact, expects of the counters what gck_cross_tile
says, and adds a request the rule does call thin at that max_batch (60 x 3)."""
import json

import numpy as np
import pytest

from gochugaru_amd import consistency, rel
from gochugaru_amd import engine as E
from gochugaru_amd.client import CheckItemError, Client, InvalidArgument
from tests import gen
from tests.helpers import load_golden, oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF
CTXS = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]


class _Family:
    """A family's graph, its oracle with every answer remembered, and its checks grouped by shape:
    (resource type, permission, subject type, subject relation) -> the distinct resource names and
    subject names occurring in them, first seen first, truncated to S * R <= 2000."""

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
            res, sub = list(res)[:50], list(sub)
            self.shapes[k] = (res, sub[:max(1, 2000 // len(res))])

    def want(self, shape, sub, res, ctx=None):
        """(perm[S, R] with 0 for an errored check, [(s * R + r, code)] ascending)."""
        rt, perm, st, srel = shape
        out = np.zeros((len(sub), len(res)), dtype=np.uint8)
        errs = []
        key_ctx = json.dumps(ctx, sort_keys=True)
        for s, sn in enumerate(sub):
            for r, rn in enumerate(res):
                k = (shape, sn, rn, key_ctx)
                if k not in self.memo:
                    self.memo[k] = tuple(self.ck.check(to_oracle_item(
                        rel.FromTriple(f"{rt}:{rn}", perm, f"{st}:{sn}" + (f"#{srel}" if srel else "")), ctx)))
                p, e = self.memo[k]
                if e:
                    errs.append((s * len(res) + r, e))
                else:
                    out[s, r] = p
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


def _ids(e, shape, sub, res):
    """The header and the two id lists as a caller interns them (unknown names: ABSENT)."""
    rt, perm, st, srel = shape
    t_r, t_s = e.type_id(rt), e.type_id(st)
    hdr = (t_r, e.relation_id(t_r, perm), t_s, E.ELLIPSIS if srel in ("", "...") else e.relation_id(t_s, srel))
    rids = e.intern(t_r, res) if t_r != E.TYPE_INVALID else np.full(len(res), E.ID_ABSENT)
    if t_s != E.TYPE_INVALID:
        sids = e.intern(t_s, sub)
    else:
        sids = np.array([E.ID_WILDCARD if n == "*" else E.ID_ABSENT for n in sub])
    return hdr, np.asarray(sids, dtype=np.uint32), np.asarray(rids, dtype=np.uint32)


def _plane(perm):
    """The row-padded plane of perm[S, R]: padding bits 0."""
    S, R = perm.shape
    stride = (R + 31) // 32
    words = np.zeros(S * stride, dtype=np.uint64)
    for s in range(S):
        for r in range(R):
            words[s * stride + r // 32] |= np.uint64(int(perm[s, r]) << (2 * (r % 32)))
    return words


def _records(errs):
    return [(int(x["index"]), int(x["code"])) for x in errs]


def _exact(e, fam, shape, sub, res, pinned=False, contexts=None, slot=0, uniform=True):
    """One cross request against the oracle and against check_uniform on the expanded pairs."""
    hdr, sids, rids = _ids(e, shape, sub, res)
    S, R = len(sub), len(res)
    n_words = S * ((R + 31) // 32)
    words = e.host_array(n_words, np.uint64) if pinned else np.zeros(n_words, dtype=np.uint64)
    words[:] = POISON  # every word must be written
    out, errs, rev = e.check_cross(hdr + (slot,), sids, rids, now_us=NOW_US, contexts=contexts, out_packed=words)
    assert rev == e.revision
    wp, we = fam.want(shape, sub, res, contexts[slot - 1] if slot else None)
    got = E.unpack_cross(out, S, R)
    bad = [(sub[s], res[r], int(wp[s, r]), int(got[s, r])) for s, r in zip(*np.nonzero(wp != got))]
    assert not bad, (shape, S, R, bad[:5])
    assert _records(errs) == we, shape
    assert np.array_equal(np.asarray(out), _plane(wp)), "padding bits or unwritten words"
    if uniform:
        pairs = np.stack([np.tile(rids, S), np.repeat(sids, R)], axis=1).astype(np.uint32)
        uw, uerrs, _ = e.check_uniform(hdr + (slot,), pairs, now_us=NOW_US, contexts=contexts)
        assert np.array_equal(E.unpack_results(uw, S * R).reshape(S, R), got)
        assert _records(uerrs) == _records(errs)


FAMS = ["nested", "gdocs", "github", "hub_arrow", "cyclic", "near_budget", "caveated"]


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("family", FAMS)
def test_cross_matches_oracle(family, pinned):
    fam = _family(family)
    e = fam.engine()
    e.reset_stats()
    assert len(fam.shapes) >= 2
    for shape, (res, sub) in fam.shapes.items():
        _exact(e, fam, shape, sub, res, pinned=pinned)
    if family in ("nested", "gdocs", "github"):  # the joins read the lists in place
        assert e.cross_stats()[0] > 0 and e.stats()["aql_batches"] > 0
    e.close()


def _nested_lists(fam, S, R):
    """S subjects and R resources of nested's doc#view@user shape, names repeated in a cycle when
    the checks hold fewer (ids are not deduplicated)."""
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    return shape, [sub[k % len(sub)] for k in range(S)], [res[k % len(res)] for k in range(R)]


def test_cross_edges():
    """A lone active lane in a row's last wave (R = 1, 33, 65), a full wave (32), 31 of 32, row
    boundaries inside a block and a partial last block; duplicated ids in both lists."""
    fam = _family("nested")
    e = fam.engine()
    for R in (1, 31, 32, 33, 65):
        for S in (1, 2, 5):
            _exact(e, fam, *_nested_lists(fam, S, R), pinned=(S == 2))
    shape, sub, res = _nested_lists(fam, 4, 40)
    _exact(e, fam, shape, [sub[0], sub[1], sub[0], sub[0]], res[:20] + res[:20])
    assert e.cross_stats() == (16, 0)
    e.close()


def test_cross_tiling():
    fam = _family("nested")
    # several tiles with a ragged right edge and a ragged bottom edge
    assert E.cross_tile(10, 100, 256) == (4, 64)
    for kw in ({}, {"workspaces": 1}):
        e = fam.engine(max_batch=256, **kw)
        _exact(e, fam, *_nested_lists(fam, 10, 100), pinned=True)
        _exact(e, fam, *_nested_lists(fam, 10, 100), uniform=False)
        assert e.cross_stats() == (12, 0)
        e.close()
    e = fam.engine(max_batch=64)
    # (see the module docstring: by the rule this request is eight 1 x 64 tiles, not a thin one)
    tile = E.cross_tile(1, 500, 64)
    _exact(e, fam, *_nested_lists(fam, 1, 500))
    assert e.cross_stats() == ((8, 0) if tile == (1, 64) else (0, 8))
    # the thin rule: 60 x 3 at max_batch 64 would be thirty 2 x 3 tiles; expanded in chunks of 64 checks
    assert E.cross_tile(60, 3, 64) is None
    before = e.cross_stats()
    _exact(e, fam, *_nested_lists(fam, 60, 3), pinned=True)
    assert e.cross_stats() == (before[0], before[1] + 3)
    e.close()
    # ... and at the default max_batch: one subject against more resources than the id block holds
    e = fam.engine()
    assert E.cross_tile(1, 3000, 65536) is None
    _exact(e, fam, *_nested_lists(fam, 1, 3000), uniform=False)
    assert e.cross_stats() == (0, 1)
    e.close()


def test_cross_shadowed_id_block():
    """One workspace: A, then B differing from A in one subject id and one resource id, then A
    again — a stale line of the id block's shadow would answer for the wrong id."""
    fam = _family("nested")
    e = fam.engine(workspaces=1)
    shape, sub, res = _nested_lists(fam, 6, 45)
    sub_b, res_b = list(sub), list(res)
    sub_b[3], res_b[17] = fam.shapes[shape][1][7], fam.shapes[shape][0][46]
    assert sub_b[3] != sub[3] and res_b[17] != res[17]
    for s, r in ((sub, res), (sub_b, res_b), (sub, res)):
        _exact(e, fam, shape, s, r, uniform=False)
    assert e.cross_stats() == (3, 0)
    e.close()


def test_cross_submit_and_wait():
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    reqs = []
    for k in range(8):  # eight in flight on eight workspaces, each with its own lists
        sub = [sub_all[(3 * k + j) % len(sub_all)] for j in range(2 + k)]
        res = [res_all[(5 * k + j) % len(res_all)] for j in range(30 + 3 * k)]
        hdr, sids, rids = _ids(e, shape, sub, res)
        words = e.host_array(len(sub) * ((len(res) + 31) // 32), np.uint64)
        words[:] = POISON
        errs = np.zeros(16, dtype=E.ITEM_ERROR_DTYPE)
        b = e.submit_cross(hdr, sids.copy(), rids.copy(), words, errs, now_us=NOW_US)
        sids[:] = 0  # (both lists were copied by the call)
        rids[:] = 0
        reqs.append((b, sub, res))
    for b, sub, res in reqs:
        words, errs, rev = b.wait()
        wp, we = fam.want(shape, sub, res)
        assert rev == e.revision and _records(errs) == we
        assert np.array_equal(np.asarray(words), _plane(wp))
    # a request that is not one tile is refused, and the engine goes on
    hdr, sids, rids = _ids(e, shape, *_nested_lists(fam, 1, 3000)[1:])
    with pytest.raises(E.GckError) as ei:
        e.submit_cross(hdr, sids, rids, np.zeros(94, dtype=np.uint64), np.zeros(4, dtype=E.ITEM_ERROR_DTYPE))
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    for _ in range(9):  # (every workspace of the pool is still usable)
        _exact(e, fam, *_nested_lists(fam, 3, 40), uniform=False)
    e.close()


def test_cross_compiled_loop():
    """gckd_run_cross: 50 requests, 8 in flight, pinned lists and planes."""
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    k, S, R = 50, 6, 70
    lists, subs, ress, planes, errs = [], [], [], [], []
    for b in range(k):
        sub = [sub_all[(b + 2 * j) % len(sub_all)] for j in range(S)]
        res = [res_all[(3 * b + j) % len(res_all)] for j in range(R)]
        hdr, sids, rids = _ids(e, shape, sub, res)
        hs, hr = e.host_array(S, np.uint32), e.host_array(R, np.uint32)
        hs[:], hr[:] = sids, rids
        w = e.host_array(S * ((R + 31) // 32), np.uint64)
        w[:] = POISON
        lists.append((sub, res)), subs.append(hs), ress.append(hr), planes.append(w)
        errs.append(e.host_array(8, E.ITEM_ERROR_DTYPE))
    p = e.prepare_cross([hdr] * k, [x.ctypes.data for x in subs], [S] * k, [x.ctypes.data for x in ress], [R] * k,
                        [x.ctypes.data for x in planes], [x.ctypes.data for x in errs], 8, 8, now_us=NOW_US)
    assert p.run() > 0
    for b, (sub, res) in enumerate(lists):
        wp, we = fam.want(shape, sub, res)
        assert np.array_equal(np.asarray(planes[b]), _plane(wp)), b
        assert p.n_errs[b] == len(we) == 0
    assert e.cross_stats() == (k, 0)
    e.close()


def test_cross_with_a_check_context():
    """A header context slot: check contexts force the expansion to items; exact under each
    context (CONDITIONAL without one)."""
    fam = _family("caveated")
    e = fam.engine()
    for slot in (0, 1, 2):
        for shape, (res, sub) in fam.shapes.items():
            _exact(e, fam, shape, sub[:12], res[:40], contexts=CTXS, slot=slot)
    e.close()


def test_cross_on_a_resident_engine():
    """GCK_FLAG_RESIDENT: a cross tile is dispatched normally (the running launch would read the
    id block the host rewrites between requests), and stays exact."""
    fam = _family("nested")
    e = fam.engine(resident=True, workspaces=8)
    e.reset_stats()
    for S, R in ((3, 40), (5, 65), (3, 40)):
        _exact(e, fam, *_nested_lists(fam, S, R), uniform=False)
    st = e.stats()
    assert e.cross_stats() == (3, 0) and st["resident_batches"] == 0 and st["aql_batches"] == 3
    e.close()


def test_client_check_cross():
    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(1, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jake", "user:joey", "user:jimmy", "user:nobody_of_that_name"]
    resources = ["company:authzed", "company:no_such_company"]
    rows, err = c.CheckCross(None, cs, "founder", resources, subjects)
    assert err is None
    flat, err = c.Check(None, cs, *[rel.MustFromTriple(r, "founder", s) for s in subjects for r in resources])
    assert err is None
    assert rows == [flat[2 * s:2 * s + 2] for s in range(len(subjects))]
    assert rows[0] == [True, False] and rows[3] == [False, False]  # an unknown name: a nonexistent object
    rows, err = c.CheckCross(None, cs, "founder", ["company:authzed", "user:jake"], subjects)
    assert rows is None and isinstance(err, InvalidArgument)
    rows, err = c.CheckCross(None, cs, "founder", resources, ["user:jake", "company:authzed"])
    assert rows is None and isinstance(err, InvalidArgument)
    assert c.CheckCross(None, cs, "founder", [], subjects) == ([[], [], [], []], None)
    # a per-item error surfaces as Check surfaces it: the results before it, then the error
    rows, err = c.CheckCross(None, cs, "no_such_permission", resources, subjects[:2])
    flat, ferr = c.Check(None, cs, rel.MustFromTriple(resources[0], "no_such_permission", subjects[0]))
    assert isinstance(err, CheckItemError) and isinstance(ferr, CheckItemError) and str(err) == str(ferr)
    assert rows == [[]] and flat == []
    e.close()
