"""Cross requests over device buffers (include/gck.h gck_check_bulk_cross_device and its submit form):
the two id lists, the row-padded plane, the error list and its count all live in device memory
(torch tensors on cuda:0).

Bar: the host cross call on the same request — the words bit for bit, the (index, code) records and
the count — and the oracle's answer of every (subject, resource). Every output buffer starts
poisoned: the plane with 0xFF.. and a word beyond it, which must stay; the error list and the count
with a sentinel (the entries beyond min(count, err_cap) must stay)."""
import json

import numpy as np
import pytest
import torch

from gochugaru_amd import consistency, rel
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client
from tests import gen
from tests.helpers import load_golden, oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF
SENT = 0x5A5A5A5A
MODES = ["sync", "engine", "stream"]  # the synchronous call, a submit on the workspace's stream, one on the caller's
FAMS = ["nested", "gdocs", "github", "hub_arrow", "cyclic", "near_budget", "caveated"]
JOIN_FAMS = ("nested", "gdocs", "github")
CTXS = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]


def _dev():
    return torch.device("cuda", 0)


def _u32(a):
    """A u32 numpy array as a device tensor (its bits as int32)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(_dev())


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


class _Out:
    """The device outputs of one request, poisoned: n_words + 1 words, err_cap + 2 records, the count."""

    def __init__(self, S, R, cap, count=True):
        self.nw, self.cap = S * ((R + 31) // 32), cap
        self.words = torch.full((self.nw + 1,), -1, dtype=torch.int64, device=_dev())
        self.errs = torch.full((cap + 2, 2), SENT, dtype=torch.int32, device=_dev())
        self.cnt = torch.full((1,), SENT, dtype=torch.int32, device=_dev()) if count else None

    def args(self):
        return dict(d_out_packed=self.words.data_ptr(), d_out_errs=self.errs.data_ptr() if self.cap else 0,
                    err_cap=self.cap, d_out_n_errs=self.cnt.data_ptr() if self.cnt is not None else 0)

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.words.cpu().numpy().view(np.uint64) == POISON).all() and (self.errs.cpu().numpy() == SENT).all()
        assert self.cnt is None or int(self.cnt.cpu()[0]) == SENT

    def read(self):
        """(words, records written, count or None); the poison beyond each is asserted here."""
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().view(np.uint64)
        assert int(w[self.nw]) == POISON, "the word after the plane was written"
        errs = self.errs.cpu().numpy()
        cnt = None if self.cnt is None else int(self.cnt.cpu().numpy().view(np.uint32)[0])
        if cnt is None:
            m = 0
            while m < self.cap and not (errs[m] == SENT).all():
                m += 1
        else:
            assert cnt != SENT, "the count was not written"
            m = min(cnt, self.cap)
        assert (errs[m:] == SENT).all(), "records beyond min(count, err_cap) were written"
        return w[:self.nw].copy(), [(int(np.uint32(i)), int(c)) for i, c in errs[:m]], cnt


def _cross(e, mode, hdr, sids, rids, cap=None, count=True, contexts=None, block=False):
    """One cross device request: (words, records written, count or None). block: the two lists as
    views of one buffer in block layout (read in place when the request is one tile)."""
    S, R = len(sids), len(rids)
    if block:
        keep, ds, dr = E.cross_id_block(_u32(sids), _u32(rids))
    else:
        ds, dr = _u32(sids), _u32(rids)
    out = _Out(S, R, S * R if cap is None else cap, count)
    kw = dict(out.args(), now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, ds.data_ptr(), S, dr.data_ptr(), R)
    if mode == "sync":
        rev = e.check_cross_device(*head, stream=st, **kw)
    else:
        rev = e.submit_cross_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read()


def _host(e, hdr, sids, rids, contexts=None):
    """The host cross call's (words, records, count): its list is uncapped."""
    words, errs, _ = e.check_cross(hdr, sids, rids, now_us=NOW_US, contexts=contexts)
    rec = _records(errs)
    return np.asarray(words).copy(), rec, len(rec)


def _same(got, want, what=None):
    """Device results against the host call's: words bit for bit, the records written, the count."""
    gw, gr, gc = got
    ww, wr, wc = want
    assert np.array_equal(gw, ww), (what, [(k, hex(int(a)), hex(int(b))) for k, (a, b) in enumerate(zip(gw, ww)) if a != b][:4])
    assert gr == wr[:len(gr)] and gr == sorted(gr), (what, gr[:6], wr[:6])
    if gc is not None:
        assert gc == wc, (what, gc, wc)
        assert len(gr) <= gc


def _nested_lists(fam, S, R):
    """S subjects and R resources of nested's doc#view@user shape, names repeated in a cycle when
    the checks hold fewer (ids are not deduplicated)."""
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    return shape, [sub[k % len(sub)] for k in range(S)], [res[k % len(res)] for k in range(R)]


def _bad_permission(e, hdr):
    """The header with a permission no relation of the schema has (what relation_id returns for an
    unknown name): every check of the request is an error, answered by the bundle stages."""
    return (hdr[0], E.REL_INVALID, hdr[2], hdr[3])


# ---- 1. every family, against the host call and the oracle ----------------------------------------

@pytest.mark.parametrize("family", FAMS)
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    assert len(fam.shapes) >= 2
    s0 = e.device_compact_stats()
    n_records = 0
    for j, (shape, (res, sub)) in enumerate(fam.shapes.items()):
        hdr, sids, rids = _ids(e, shape, sub, res)
        wp, we = fam.want(shape, sub, res)
        host = _host(e, hdr, sids, rids)
        assert (host[0] == _plane(wp)).all() and host[1] == we, (family, shape)  # the yardstick itself
        for mode in (MODES if j < 2 else [MODES[j % 3]]):
            got = _cross(e, mode, hdr, sids, rids)
            _same(got, host, (family, shape, mode))
            n_records += len(got[1])
    s1 = e.device_compact_stats()
    print(family, "device_compact_stats", s0, "->", s1, "error records", n_records)
    if family in JOIN_FAMS:  # the joins read the lists in place
        assert s1[0] > s0[0]
    if family == "near_budget":
        assert n_records > 0, "near_budget gave no error record"
    assert sum(s1) > sum(s0)
    e.close()


def test_cross_stats_do_not_count_device_requests():
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 3, 40))
    before = e.cross_stats()
    for mode in MODES:
        _cross(e, mode, hdr, sids, rids)
    assert e.cross_stats() == before and e.device_compact_stats() == (3, 0)
    e.close()


# ---- 2. checks the join leaves: the patch and the mapped emit -------------------------------------

def test_deferred_checks_are_patched_and_listed():
    """A userset-subject shape of the Google-Docs graph, whose join leaves checks to the bundle
    stages, on a 5 x 33 tile (two words per row, the second almost all padding): the patch writes
    padded positions; then a header whose every check is an error, so that every record goes through
    the padded -> request index map."""
    fam = _family("gdocs")
    e = fam.engine()
    userset = [k for k in fam.shapes if k[3] not in ("", "...")]
    assert userset
    shape = userset[0]
    res, sub = fam.shapes[shape]
    sub, res = [sub[k % len(sub)] for k in range(5)], [res[k % len(res)] for k in range(33)]
    hdr, sids, rids = _ids(e, shape, sub, res)
    wp, we = fam.want(shape, sub, res)
    for mode in MODES:
        e.reset_stats()
        s0 = e.device_compact_stats()
        got = _cross(e, mode, hdr, sids, rids)
        st = e.stats()
        left = st["queries"] - st["closure_checks"]
        print(f"{mode}: {left} of {st['queries']} checks left by the join")
        assert e.device_compact_stats() == (s0[0] + 1, s0[1]), "not in place"
        assert left >= 3, "the join left too few checks for the patch to matter"
        _same(got, _host(e, hdr, sids, rids), mode)
        assert (got[0] == _plane(wp)).all() and got[1] == we
    # every check an error: S * R records, index s * R + r, through the map (R = 33 is not the row's 64)
    bad = _bad_permission(e, hdr)
    host = _host(e, bad, sids, rids)
    assert [i for i, _ in host[1]] == list(range(5 * 33))
    for mode in MODES:
        s0 = e.device_compact_stats()
        got = _cross(e, mode, bad, sids, rids)
        _same(got, host, ("all errors", mode))
        assert not got[0].any() and got[2] == 165 and len(got[1]) == 165
        assert e.device_compact_stats() == (s0[0] + 1, s0[1])
    e.close()


# ---- 3. edges -------------------------------------------------------------------------------------

def test_edges():
    """A lone active lane in a row's last wave (R = 1, 33, 65), a full wave (32), 31 of 32, rows that
    end inside a block; repeated ids in both lists; the block layout on the same requests."""
    fam = _family("nested")
    e = fam.engine()
    k = 0
    for R in (1, 31, 32, 33, 65):
        for S in (1, 2, 5):
            shape, sub, res = _nested_lists(fam, S, R)
            hdr, sids, rids = _ids(e, shape, sub, res)
            host = _host(e, hdr, sids, rids)
            assert (host[0] == _plane(fam.want(shape, sub, res)[0])).all()
            mode = MODES[k % 3]
            k += 1
            got = _cross(e, mode, hdr, sids, rids)
            _same(got, host, (S, R, mode))
            blk = _cross(e, MODES[k % 3], hdr, sids, rids, block=True)
            _same(blk, host, (S, R, "block"))
            assert np.array_equal(blk[0], got[0])
    shape, sub, res = _nested_lists(fam, 4, 40)
    sub, res = [sub[0], sub[1], sub[0], sub[0]], res[:20] + res[:20]
    hdr, sids, rids = _ids(e, shape, sub, res)
    for mode in MODES:
        _same(_cross(e, mode, hdr, sids, rids), _host(e, hdr, sids, rids), ("repeated", mode))
    assert e.device_compact_stats() == (33, 0)
    e.close()


@pytest.mark.parametrize("mode", MODES)
def test_error_list_protocol(mode):
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 3, 37))
    bad = _bad_permission(e, hdr)
    host = _host(e, bad, sids, rids)
    n = 3 * 37
    assert host[2] == n
    for cap in (0, 1, 40, n + 5):
        for count in (True, False):
            got = _cross(e, mode, bad, sids, rids, cap=cap, count=count)
            _same(got, host, (mode, cap, count))
            assert len(got[1]) == min(cap, n) and got[2] == (n if count else None)
    # an error-free request after them: the count is written as 0
    got = _cross(e, mode, hdr, sids, rids, cap=4)
    assert got[2] == 0 and got[1] == []
    _same(got, _host(e, hdr, sids, rids))
    e.close()


def test_empty_request_writes_only_the_count():
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 3, 40))
    s0 = e.device_compact_stats()
    for mode in MODES:
        for s, r in ((sids[:0], rids), (sids, rids[:0]), (sids[:0], rids[:0])):
            out = _Out(0, 0, 2)
            kw = dict(out.args(), now_us=NOW_US)
            st = torch.cuda.current_stream().cuda_stream
            head = (hdr, _u32(s).data_ptr() if len(s) else 0, len(s), _u32(r).data_ptr() if len(r) else 0, len(r))
            if mode == "sync":
                e.check_cross_device(*head, stream=st, **kw)
            else:
                e.submit_cross_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
            got = out.read()
            assert got[2] == 0 and got[1] == []
    assert e.device_compact_stats() == s0
    e.close()


# ---- 4. several bands -----------------------------------------------------------------------------

@pytest.mark.parametrize("workspaces", [0, 1], ids=["two-workspaces", "one-workspace"])
def test_bands(workspaces):
    """max_batch = 256 cuts S x 100 into 2-row tiles: 10 x 100 is five bands, 9 x 100 five with a
    ragged last one. The records of a request whose every check fails ascend across the bands."""
    fam = _family("nested")
    assert E.cross_tile_device(10, 100, 256) == 2
    e = fam.engine(max_batch=256, workspaces=workspaces)
    for S in (10, 9):
        shape, sub, res = _nested_lists(fam, S, 100)
        hdr, sids, rids = _ids(e, shape, sub, res)
        host = _host(e, hdr, sids, rids)
        assert (host[0] == _plane(fam.want(shape, sub, res)[0])).all()
        s0 = e.device_compact_stats()
        _same(_cross(e, "sync", hdr, sids, rids), host, S)
        _same(_cross(e, "sync", hdr, sids, rids, block=True), host, (S, "block layout, several tiles: gathered"))
        assert e.device_compact_stats() == (s0[0] + 10, s0[1])
        bad = _bad_permission(e, hdr)
        hb = _host(e, bad, sids, rids)
        assert [i for i, _ in hb[1]] == list(range(S * 100))
        for cap, count in ((S * 100, True), (250, True), (250, False), (0, True)):
            got = _cross(e, "sync", bad, sids, rids, cap=cap, count=count)
            _same(got, hb, (S, "errors", cap, count))
            assert len(got[1]) == min(cap, S * 100)
        # a submitted request must be one tile
        with pytest.raises(E.GckError) as ei:
            _cross(e, "engine", hdr, sids, rids)
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    e.close()


# ---- 5. expanded on the device --------------------------------------------------------------------

def test_expanded_chunks_split_words_and_rows():
    """max_batch = 64: 1 x 500 (a row's 512 padded checks exceed a batch) runs as eight chunks of 64
    checks; 60 x 3 (thin) as three, whose boundaries fall inside rows and inside plane words."""
    fam = _family("nested")
    assert E.cross_tile_device(1, 500, 64) == 0 and E.cross_tile_device(60, 3, 64) == 0
    for workspaces in (0, 1):
        e = fam.engine(max_batch=64, workspaces=workspaces)
        for (S, R), chunks in (((1, 500), 8), ((60, 3), 3)):
            shape, sub, res = _nested_lists(fam, S, R)
            hdr, sids, rids = _ids(e, shape, sub, res)
            host = _host(e, hdr, sids, rids)
            assert (host[0] == _plane(fam.want(shape, sub, res)[0])).all()
            s0 = e.device_compact_stats()
            _same(_cross(e, "sync", hdr, sids, rids), host, (S, R))
            assert e.device_compact_stats() == (s0[0], s0[1] + chunks), (S, R)
            bad = _bad_permission(e, hdr)
            hb = _host(e, bad, sids, rids)
            for cap, count in ((S * R, True), (70, True), (70, False)):
                got = _cross(e, "sync", bad, sids, rids, cap=cap, count=count)
                _same(got, hb, (S, R, "errors", cap, count))
                assert len(got[1]) == min(cap, S * R)
        e.close()


@pytest.mark.parametrize("kw", [{"profile": True}, {"closure": False, "labels": False}, {"wide_only": True}],
                         ids=["profiling", "no-join", "wide-only"])
def test_expanded_engine_paths(kw):
    fam = _family("gdocs")
    e = fam.engine(**kw)
    s0 = e.device_compact_stats()
    k = 0
    for shape, (res, sub) in list(fam.shapes.items())[:3]:
        hdr, sids, rids = _ids(e, shape, sub[:7], res[:33])
        host = _host(e, hdr, sids, rids)
        assert (host[0] == _plane(fam.want(shape, sub[:7], res[:33])[0])).all()
        for mode in MODES:
            _same(_cross(e, mode, hdr, sids, rids), host, (shape, mode))
            k += 1
    assert e.device_compact_stats() == (s0[0], s0[1] + k)
    e.close()


def test_check_context():
    """A header context slot: check contexts force the expansion; exact under each context."""
    fam = _family("caveated")
    e = fam.engine()
    s0 = e.device_compact_stats()
    k = 0
    for slot in (0, 1, 2):
        for shape, (res, sub) in fam.shapes.items():
            sub, res = sub[:6], res[:35]
            hdr, sids, rids = _ids(e, shape, sub, res)
            wp, we = fam.want(shape, sub, res, CTXS[slot - 1] if slot else None)
            mode = MODES[k % 3]
            got = _cross(e, mode, hdr + (slot,), sids, rids, contexts=CTXS)
            k += 1
            assert (got[0] == _plane(wp)).all() and got[1] == we and got[2] == len(we), (slot, shape, mode)
            _same(got, _host(e, hdr + (slot,), sids, rids, contexts=CTXS), (slot, shape, mode))
    assert e.device_compact_stats() == (s0[0], s0[1] + k)
    e.close()


# ---- 6. submit / wait -----------------------------------------------------------------------------

def test_eight_in_flight():
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    reqs = []
    torch.cuda.synchronize()
    for k in range(8):  # eight in flight on eight workspaces, each with its own lists
        sub = [sub_all[(3 * k + j) % len(sub_all)] for j in range(2 + k)]
        res = [res_all[(5 * k + j) % len(res_all)] for j in range(30 + 3 * k)]
        hdr, sids, rids = _ids(e, shape, sub, res)
        if k % 2:
            keep, ds, dr = E.cross_id_block(_u32(sids), _u32(rids))
        else:
            keep, ds, dr = None, _u32(sids), _u32(rids)
        out = _Out(len(sub), len(res), 4)
        torch.cuda.synchronize()
        b = e.submit_cross_device(hdr, ds.data_ptr(), len(sub), dr.data_ptr(), len(res), now_us=NOW_US,
                                  stream=torch.cuda.current_stream().cuda_stream, engine_stream=(k % 4 < 2), **out.args())
        reqs.append((b, sub, res, out, ds, dr, keep))
    for b, sub, res, out, ds, dr, keep in reversed(reqs):
        assert b.wait() == e.revision
        ds.zero_(), dr.zero_()  # (the lists are the caller's again only after the wait)
        wp, we = fam.want(shape, sub, res)
        got = out.read()
        assert np.array_equal(got[0], _plane(wp)) and got[1] == we and got[2] == len(we)
    # a request that is not one device tile is refused, and every workspace of the pool stays usable
    hdr, sids, rids = _ids(e, shape, *_nested_lists(fam, 1, 3000)[1:])
    out = _Out(1, 3000, 4)
    ds, dr = _u32(sids), _u32(rids)
    torch.cuda.synchronize()
    for engine_stream in (True, False):
        with pytest.raises(E.GckError) as ei:
            e.submit_cross_device(hdr, ds.data_ptr(), 1, dr.data_ptr(), 3000, engine_stream=engine_stream, **out.args())
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT and "one tile" in ei.value.message
    out.untouched()
    _same(_cross(e, "sync", hdr, sids, rids), _host(e, hdr, sids, rids), "1 x 3000, synchronous: expanded")
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 3, 40))
    host = _host(e, hdr, sids, rids)
    for k in range(9):
        _same(_cross(e, MODES[1 + k % 2], hdr, sids, rids), host, k)
    e.close()


def test_compiled_loop():
    """gckd_run_cross_device: 50 requests, 8 in flight, on the engine's streams and on the caller's."""
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    k, S, R = 50, 6, 70
    lists, keep, subs, ress = [], [], [], []
    for b in range(k):
        sub = [sub_all[(b + 2 * j) % len(sub_all)] for j in range(S)]
        res = [res_all[(3 * b + j) % len(res_all)] for j in range(R)]
        hdr, sids, rids = _ids(e, shape, sub, res)
        if b % 2:
            blk, ds, dr = E.cross_id_block(_u32(sids), _u32(rids))
        else:
            blk, ds, dr = None, _u32(sids), _u32(rids)
        lists.append((sub, res)), keep.append((blk, ds, dr)), subs.append(ds.data_ptr()), ress.append(dr.data_ptr())
    streams = [torch.cuda.Stream() for _ in range(8)]
    for engine_streams in (True, False):
        outs = [_Out(S, R, 8) for _ in range(k)]
        torch.cuda.synchronize()
        s0 = e.device_compact_stats()
        p = e.prepare_cross_device([hdr] * k, subs, [S] * k, ress, [R] * k, [o.words.data_ptr() for o in outs],
                                   [o.errs.data_ptr() for o in outs], 8, 8, n_errs=[o.cnt.data_ptr() for o in outs],
                                   streams=[s.cuda_stream for s in streams], engine_streams=engine_streams,
                                   now_us=NOW_US)
        assert p.run() > 0
        for b, (sub, res) in enumerate(lists):
            wp, we = fam.want(shape, sub, res)
            got = outs[b].read()
            assert np.array_equal(got[0], _plane(wp)) and got[1] == we and got[2] == 0, (engine_streams, b)
        assert e.device_compact_stats() == (s0[0] + k, s0[1])
    e.close()


# ---- 7. the Python layer --------------------------------------------------------------------------

def test_check_cross_ids_and_client():
    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(1, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jake", "user:joey", "user:jimmy", "user:nobody_of_that_name"]
    resources = ["company:authzed", "company:no_such_company"]
    rows, err = c.CheckCross(None, cs, "founder", resources, subjects)
    assert err is None and rows[0] == [True, False]
    user, company = e.type_id("user"), e.type_id("company")
    sids = _u32(e.intern(user, [s.split(":")[1] for s in subjects]))
    rids = _u32(e.intern(company, [r.split(":")[1] for r in resources]))
    plane, err = c.CheckCrossDevice(None, cs, "company#founder", rids, "user", sids)
    assert err is None and plane.is_cuda and plane.dtype == torch.int64 and tuple(plane.shape) == (4, 1)
    perm = E.unpack_cross(plane.cpu().numpy().view(np.uint64), 4, 2)
    assert (perm == E.PERM_HAS).tolist() == rows
    direct = e.check_cross_ids((company, e.relation_id(company, "founder"), user, E.ELLIPSIS), sids, rids)
    assert torch.equal(direct, plane)
    # the same refusals and errors as the host form's siblings
    plane, err = c.CheckCrossDevice(None, cs, "company#founder", rids.cpu(), "user", sids)
    assert plane is None and err is not None
    plane, err = c.CheckCrossDevice(None, cs, "company#no_such_permission", rids, "user", sids)
    assert plane is None and isinstance(err, E.GckError)
    with pytest.raises(E.GckError):  # a per-item error: raised, as filter_ids raises it
        e.check_cross_ids((company, e.relation_id(user, "no_such"), user, E.ELLIPSIS), sids, rids)
    empty, err = c.CheckCrossDevice(None, cs, "company#founder", rids[:0], "user", sids)
    assert err is None and tuple(empty.shape) == (4, 0)
    e.close()


# ---- 8. refusals before any launch ----------------------------------------------------------------

def test_refusals():
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 4, 40))
    ds, dr = _u32(np.concatenate([sids, sids])), _u32(np.concatenate([rids, rids]))
    out = _Out(4, 40, 8)
    torch.cuda.synchronize()
    a = out.args()
    W, X, N = a["d_out_packed"], a["d_out_errs"], a["d_out_n_errs"]
    s0, b0 = e.device_compact_stats(), e.stats()["batches"]

    def refused(fn, *args, **k):
        with pytest.raises(E.GckError) as ei:
            r = fn(*args, **k)
            if hasattr(r, "wait"):
                r.wait()
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        return ei.value.message

    for fn in (e.check_cross_device, e.submit_cross_device):
        assert "d_out_packed" in refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr(), 40, W + 4, X, 8, N)
        assert "2^32" in refused(fn, hdr, ds.data_ptr(), 65536, dr.data_ptr(), 65536, W, X, 8, N)
        assert "reserved" in refused(fn, E.Uniform(*hdr[:4], 0, 7), ds.data_ptr(), 4, dr.data_ptr(), 40, W, X, 8, N)
        assert "d_subjects" in refused(fn, hdr, ds.data_ptr() + 2, 4, dr.data_ptr(), 40, W, X, 8, N)
        assert "d_resources" in refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr() + 1, 40, W, X, 8, N)
        refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr(), 40, W, X + 2, 8, N)     # misaligned records
        refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr(), 40, W, X, 8, N + 2)     # misaligned count
        refused(fn, hdr, 0, 4, dr.data_ptr(), 40, W, X, 8, N)                     # null lists with S * R > 0
        refused(fn, hdr, ds.data_ptr(), 4, 0, 40, W, X, 8, N)
        refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr(), 40, 0, X, 8, N)
        refused(fn, hdr, ds.data_ptr(), 4, dr.data_ptr(), 40, W, 0, 8, N)         # err_cap without a list
        refused(fn, hdr + (1,), ds.data_ptr(), 4, dr.data_ptr(), 40, W, X, 8, N)  # a slot beyond the contexts
    out.untouched()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran
    _same(_cross(e, "engine", hdr, sids, rids), _host(e, hdr, sids, rids), "after refusals")
    e.close()
