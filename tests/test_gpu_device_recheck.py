"""Recheck requests (include/gck.h gck_recheck_list_device, gck_recheck_cross_device, their submit
forms and the plane-only calls gck_diff_planes_device / gck_diff_cross_planes_device): a list or cross
request over device buffers evaluated at the current revision and compared by kernels with the
caller's previous plane; the ordered change records, the new plane and the count words in device
memory (torch tensors on cuda:0).

Bar, never the code under test: a numpy diff of the host calls' planes (Engine.check_cross,
Engine.check_list) taken before and after a Watch batch, those planes themselves against the oracle's
answers at both revisions, and the plain device call for the new plane and the error records. Every
output starts poisoned — the record arrays with a sentinel and two entries beyond cap, the offsets
with two entries beyond S + 1, the plane with a word beyond it, the error list, both count words —
and what the protocol leaves untouched is asserted untouched."""
import numpy as np
import pytest
import torch

from gochugaru_amd import engine as E
from gochugaru_amd.client import Client
from tests import gen
from tests.helpers import oracle_for, to_oracle_item
from tests.test_change_plane import expect as expect_dense
from tests.test_change_plane import pack as pack_dense
from tests.test_change_rows import expect as expect_rows
from tests.test_change_rows import pack_rows
from tests.test_gpu_device_cross import (MODES, NOW_US, POISON, SENT, _cross, _dev, _family, _host, _ids, _records, _same,
                                         _u32)
from gochugaru_amd import rel

pytestmark = pytest.mark.gpu
SENT8 = 0xA5
ANY, GAINED, LOST = E.CHANGE_ANY, E.CHANGE_GAINED, E.CHANGE_LOST
SHAPE = ("doc", "view", "user", "")
R_ = E.VARY_RESOURCE


def _i64(words):
    """A u64 numpy plane as an int64 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1).view(np.int64).copy()).to(_dev())


class _DOut:
    """The device outputs of one recheck request, poisoned. rows: S for the cross form (row_off of
    S + 3 entries), None for the dense form."""

    def __init__(self, nw, cap, rows=None, which=("ids", "pos", "trans"), err_cap=4):
        self.nw, self.cap, self.rows, self.which, self.err_cap = nw, cap, rows, tuple(which), err_cap
        full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=_dev())
        self.ids = full(cap + 2, SENT, torch.int32) if "ids" in which else None
        self.pos = full(cap + 2, SENT, torch.int32) if "pos" in which else None  # (the cross form's columns)
        self.trans = full(cap + 2, SENT8, torch.uint8) if "trans" in which else None
        self.row_off = full(rows + 3, SENT, torch.int32) if rows is not None else None
        self.cnt = full(2, SENT, torch.int32)  # [changes, errors]
        self.errs = torch.full((err_cap + 2, 2), SENT, dtype=torch.int32, device=_dev())
        self.words = full(nw + 1, -1, torch.int64)

    def sel(self):
        p = lambda t: t.data_ptr() if t is not None else 0
        kw = dict(d_out_n=self.cnt.data_ptr(), cap=self.cap, d_out_ids=p(self.ids), d_out_trans=p(self.trans))
        if self.rows is None:
            kw["d_out_pos"] = p(self.pos)
        else:
            kw.update(d_out_col=p(self.pos), d_out_row_off=self.row_off.data_ptr())
        return kw

    def args(self):
        return dict(self.sel(), d_out_packed=self.words.data_ptr(), d_out_errs=self.errs.data_ptr() if self.err_cap else 0,
                    err_cap=self.err_cap, d_out_n_errs=self.cnt.data_ptr() + 4)

    def untouched(self):
        torch.cuda.synchronize()
        for t, v in ((self.ids, SENT), (self.pos, SENT), (self.trans, SENT8), (self.row_off, SENT), (self.cnt, SENT),
                     (self.errs, SENT), (self.words, -1)):
            assert t is None or bool((t == v).all()), "a refused call wrote an output"

    def read(self, request=True):
        """What was written, the poison beyond it asserted. request=False: a plane-only call (no plane,
        no error outputs)."""
        torch.cuda.synchronize()
        total, n_errs = (int(x) for x in self.cnt.cpu().numpy().view(np.uint32))
        assert total != SENT, "the count word was not written"
        m = min(total, self.cap)
        got = {"total": total}
        for name, t, sent in (("ids", self.ids, SENT), ("pos", self.pos, SENT), ("trans", self.trans, SENT8)):
            if t is None:
                got[name] = None
                continue
            a = t.cpu().numpy()
            a = a.view(np.uint32) if a.dtype == np.int32 else a
            assert (a[m:] == sent).all(), f"{name}: entries beyond min(total, cap) were written"
            got[name] = a[:m].copy()
        if self.rows is not None:
            off = self.row_off.cpu().numpy().view(np.uint32)
            assert (off[self.rows + 1:] == SENT).all(), "offsets beyond S + 1 were written"
            got["row_off"] = off[:self.rows + 1].copy()
        errs = self.errs.cpu().numpy()
        w = self.words.cpu().numpy().view(np.uint64)
        if not request:
            assert n_errs == SENT and (errs == SENT).all() and (w == POISON).all()
            return got
        assert n_errs != SENT, "the error count word was not written"
        k = min(n_errs, self.err_cap)
        assert (errs[k:] == SENT).all(), "records beyond min(count, err_cap) were written"
        got.update(n_errs=n_errs, errs=[(int(np.uint32(i)), int(c)) for i, c in errs[:k]])
        assert int(w[self.nw]) == POISON, "the word after the plane was written"
        got["words"] = w[:self.nw].copy()
        return got


def _agree(got, exp, cap, what=None, rows=False):
    """A recheck's records against the numpy diff under the cap protocol. exp: (ids, pos, trans), or
    with rows (row_off, ids, col, trans)."""
    if rows:
        assert np.array_equal(got["row_off"], exp[0]), (what, got["row_off"][:8], exp[0][:8])
        exp = exp[1:]
    total = len(exp[1])
    assert got["total"] == total, (what, got["total"], total)
    m = min(total, cap)
    for name, want in zip(("ids", "pos", "trans"), exp):
        if got[name] is not None:
            assert len(got[name]) == m and np.array_equal(got[name], want[:m]), (what, name, got[name][:8], want[:8])


def _recheck_cross(e, mode, hdr, sids, rids, prev, transitions, out):
    ds, dr = _u32(sids), _u32(rids)
    kw = dict(out.args(), transitions=transitions, now_us=NOW_US)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, ds.data_ptr(), len(sids), dr.data_ptr(), len(rids), prev.data_ptr() if prev is not None else 0)
    if mode == "sync":
        rev = e.recheck_cross_device(*head, stream=st, **kw)
    else:
        rev = e.submit_recheck_cross_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    return rev, out.read()


def _recheck_list(e, mode, hdr, fixed, ids, prev, transitions, out):
    d = _u32(ids)
    kw = dict(out.args(), transitions=transitions, d_ids=d.data_ptr(), now_us=NOW_US)
    if mode != "stream":
        torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, fixed, R_, len(ids), prev.data_ptr() if prev is not None else 0)
    if mode == "sync":
        rev = e.recheck_list_device(*head, stream=st, **kw)
    else:
        rev = e.submit_recheck_list_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    return rev, out.read()


def _plain_list(e, mode, hdr, fixed, ids):
    """The plain list device call's (words, records, count)."""
    n = len(ids)
    d = _u32(ids)
    words = torch.full(((n + 31) // 32 + 1,), -1, dtype=torch.int64, device=_dev())
    errs = torch.full((n + 2, 2), SENT, dtype=torch.int32, device=_dev())
    cnt = torch.full((1,), SENT, dtype=torch.int32, device=_dev())
    kw = dict(d_ids=d.data_ptr(), d_out_errs=errs.data_ptr(), err_cap=n, d_out_n_errs=cnt.data_ptr(), now_us=NOW_US)
    if mode != "stream":
        torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    if mode == "sync":
        e.check_list_device(hdr, fixed, R_, n, words.data_ptr(), stream=st, **kw)
    else:
        e.submit_list_device(hdr, fixed, R_, n, words.data_ptr(), stream=st, engine_stream=(mode == "engine"), **kw).wait()
    torch.cuda.synchronize()
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    return (words.cpu().numpy().view(np.uint64)[:-1].copy(),
            [(int(np.uint32(i)), int(x)) for i, x in errs.cpu().numpy()[:c]], c)


def _host_list(e, hdr, fixed, ids):
    words, errs, _ = e.check_list(hdr, fixed, R_, np.ascontiguousarray(ids, dtype=np.uint32), now_us=NOW_US)
    return np.asarray(words).copy(), _records(errs)


# ---- 1. the plane-only calls at the lane-scan edges ------------------------------------------------

@pytest.fixture(scope="module")
def nested_engine():
    e = _family("nested").engine()
    yield e
    e.close()


@pytest.mark.parametrize("n", [33, 8193])
def test_dense_planes(nested_engine, n):
    e = nested_engine
    rng = np.random.default_rng(n)
    old, new = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)
    src = rng.integers(0, 1 << 31, n).astype(np.uint32)
    d_old, d_new, d_src = _i64(pack_dense(old, rng)), _i64(pack_dense(new, rng)), _u32(src)  # (garbage in the padding lanes)
    st = torch.cuda.current_stream().cuda_stream
    for tr in (ANY, GAINED, LOST, 1 << (4 * 3 + 1)):
        exp = expect_dense(old, new, tr, src)
        total = len(exp[1])
        for cap in (0, max(total - 1, 0), total + 2):
            out = _DOut(0, cap)
            e.diff_planes_device(d_old.data_ptr(), d_new.data_ptr(), n, d_ids=d_src.data_ptr(), transitions=tr, stream=st,
                                 **out.sel())
            _agree(out.read(request=False), exp, cap, (n, hex(tr), cap))
    # a null old plane reads as zeros; a range gives the ids; any subset of the arrays
    exp = expect_dense(np.zeros(n, dtype=np.uint8), new, GAINED, None, first_id=500)
    assert np.array_equal(exp[1], np.flatnonzero(new >= 2))
    for which in (("ids", "pos", "trans"), ("pos",), ("trans",)):
        out = _DOut(0, n, which=which)
        e.diff_planes_device(0, d_new.data_ptr(), n, first_id=500, transitions=GAINED, stream=st, **out.sel())
        _agree(out.read(request=False), exp, n, (n, which))


def test_dense_planes_across_chunks():
    """max_batch = 2,048: a plane of 8,193 checks is five chunks of 64 words, the count chained."""
    e = _family("nested").engine(max_batch=2048)
    n = 8193
    rng = np.random.default_rng(7)
    old, new = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8)
    d_old, d_new = _i64(pack_dense(old, rng)), _i64(pack_dense(new, rng))
    exp = expect_dense(old, new, ANY, None, first_id=9)
    for cap in (len(exp[1]) - 1, len(exp[1]) + 2):
        out = _DOut(0, cap)
        e.diff_planes_device(d_old.data_ptr(), d_new.data_ptr(), n, first_id=9, transitions=ANY,
                             stream=torch.cuda.current_stream().cuda_stream, **out.sel())
        _agree(out.read(request=False), exp, cap, cap)
    e.close()


@pytest.mark.parametrize("S,R", [(5, 33), (257, 31), (2, 2049)])
def test_cross_planes(nested_engine, S, R):
    e = nested_engine
    rng = np.random.default_rng(S * 7 + R)
    old, new = rng.integers(0, 4, (S, R)).astype(np.uint8), rng.integers(0, 4, (S, R)).astype(np.uint8)
    src = rng.integers(0, 1 << 31, R).astype(np.uint32)
    d_old, d_new, d_src = _i64(pack_rows(old, rng)), _i64(pack_rows(new, rng)), _u32(src)
    st = torch.cuda.current_stream().cuda_stream
    for tr in (ANY, GAINED, LOST, 1 << (4 * 0 + 2)):
        exp = expect_rows(old, new, tr, src)
        total = int(exp[0][-1])
        for cap in (0, max(total - 1, 0), total + 2):
            out = _DOut(0, cap, rows=S)
            e.diff_cross_planes_device(d_old.data_ptr(), d_new.data_ptr(), S, R, d_src.data_ptr(), transitions=tr, stream=st,
                                       **out.sel())
            _agree(out.read(request=False), exp, cap, (S, R, hex(tr), cap), rows=True)
    exp = expect_rows(np.zeros((S, R), dtype=np.uint8), new, GAINED, src)
    for which in (("ids", "pos", "trans"), ("ids",), ("pos", "trans")):
        out = _DOut(0, S * R, rows=S, which=which)
        e.diff_cross_planes_device(0, d_new.data_ptr(), S, R, d_src.data_ptr(), transitions=GAINED, stream=st, **out.sel())
        _agree(out.read(request=False), exp, S * R, (S, R, which), rows=True)


# ---- 2. across a Watch batch -------------------------------------------------------------------------

def _oracle_plane(ck, users, docs):
    out = np.zeros((len(users), len(docs)), dtype=np.uint8)
    for s, u in enumerate(users):
        for r, d in enumerate(docs):
            p, err = ck.check(to_oracle_item(rel.FromTriple(f"doc:{d}", "view", f"user:{u}"), None))
            out[s, r] = 0 if err else p
    return out


def _scene(fam, n_users=5, n_docs=40, n_list=70):
    """The requests and the Watch batch of test 2, chosen with the oracle alone: five users with a
    mixed row over forty docs, the first of them the list request's user over about seventy doc names
    (the shape's docs, repeated in a cycle). The batch adds the user to a group that views a doc it
    cannot see, removes one of the user's memberships (the first whose loss the oracle confirms),
    deletes one direct viewer grant of a listed doc and adds another. Returns (users, docs, list docs,
    update lines, tuples after)."""
    res, sub = fam.shapes[SHAPE]
    ck = oracle_for(fam.schema, fam.tuples, max_depth=fam.depth, now=NOW_US / 1e6)
    docs = list(res)[:n_docs]
    rows = _oracle_plane(ck, sub, docs)
    mixed = [u for u, row in zip(sub, rows) if 0 < (row >= 2).sum() < len(docs)]
    viewers = [t for t in fam.tuples if t.startswith("doc:") and "#viewer@" in t and t[4:].split("#")[0] in docs]
    grant_del = viewers[0]
    grant_add = next(f"doc:{d}#viewer@{grant_del.split('@')[1]}" for d in docs
                     if f"doc:{d}#viewer@{grant_del.split('@')[1]}" not in fam.tuples)
    for u in mixed:  # the list request's user: the first for whom such a batch exists
        A = rows[sub.index(u)]
        adds = [f"{t.split('@')[1]}@user:{u}" for t in viewers
                if t.endswith("#member") and A[docs.index(t[4:].split("#")[0])] == 1
                and f"{t.split('@')[1]}@user:{u}" not in fam.tuples]
        if not adds:
            continue
        for gone in (t for t in fam.tuples if t.startswith("group:") and t.endswith(f"@user:{u}")):
            after = [t for t in fam.tuples if t not in (gone, grant_del)] + [adds[0], grant_add]
            B = _oracle_plane(oracle_for(fam.schema, after, max_depth=fam.depth, now=NOW_US / 1e6), [u], docs)[0]
            if ((A >= 2) & (B < 2)).any() and ((A < 2) & (B >= 2)).any():
                lines = [f"CREATE {adds[0]}", f"DELETE {gone}", f"DELETE {grant_del}", f"CREATE {grant_add}"]
                listed = (docs * (n_list // len(docs) + 1))[:n_list]
                users = ([u] + [v for v in mixed if v != u])[:n_users]
                assert len(users) == n_users
                return users, docs, listed, lines, after
    raise AssertionError("no membership of the user whose removal loses a listed doc")


@pytest.mark.parametrize("family", ["nested", "gdocs"])
def test_across_a_watch_batch(family):
    fam = _family(family)
    users, docs, listed, lines, after = _scene(fam)
    e = fam.engine()
    hdr, sids, rids = _ids(e, SHAPE, users, docs)
    _, _, lids = _ids(e, SHAPE, users[:1], listed)
    fixed, S, R, n = int(sids[0]), len(users), len(docs), len(listed)
    rev0 = e.revision

    # revision r: the host planes, equal to the oracle's answers
    A = _host(e, hdr, sids, rids)
    LA = _host_list(e, hdr, fixed, lids)
    ck = oracle_for(fam.schema, fam.tuples, max_depth=fam.depth, now=NOW_US / 1e6)
    vA = E.unpack_cross(A[0], S, R)
    assert np.array_equal(vA, _oracle_plane(ck, users, docs)) and not A[1]
    vLA = E.unpack_results(LA[0], n)
    assert np.array_equal(vLA, _oracle_plane(ck, users[:1], listed)[0]) and not LA[1]

    # prev = None with GAINED is the filter request's survivors (the initial grant set)
    out = _DOut(S * ((R + 31) // 32), S * R, rows=S)
    _, got = _recheck_cross(e, "sync", hdr, sids, rids, None, GAINED, out)
    row_off, f_ids, f_col, f_perm = e.filter_cross_ids(hdr, _u32(sids), _u32(rids), want_col=True, want_perm=True)
    assert np.array_equal(got["row_off"], row_off.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["ids"], f_ids.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["pos"], f_col.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["trans"], f_perm.cpu().numpy())  # (4 * 0 + new)
    assert np.array_equal(got["words"], A[0])
    out = _DOut((n + 31) // 32, n)
    _, got = _recheck_list(e, "sync", hdr, fixed, lids, None, GAINED, out)
    f_ids, f_pos = e.filter_ids(hdr, fixed, R_, _u32(lids), want_pos=True)
    assert np.array_equal(got["ids"], f_ids.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["pos"], f_pos.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["words"], LA[0])

    # the Watch batch -> revision r + 1
    e.apply_updates_text(rev0 + 1, "\n".join(lines))
    assert e.revision == rev0 + 1
    B = _host(e, hdr, sids, rids)
    LB = _host_list(e, hdr, fixed, lids)
    ck = oracle_for(fam.schema, after, max_depth=fam.depth, now=NOW_US / 1e6)
    vB = E.unpack_cross(B[0], S, R)
    assert np.array_equal(vB, _oracle_plane(ck, users, docs)) and not B[1]
    vLB = E.unpack_results(LB[0], n)
    assert np.array_equal(vLB, _oracle_plane(ck, users[:1], listed)[0]) and not LB[1]
    # the condition: the expected diff holds a gained and a lost cell, in both requests
    for a, b in ((vA, vB), (vLA, vLB)):
        assert ((a < 2) & (b >= 2)).any() and ((a >= 2) & (b < 2)).any(), lines

    prev, lprev = _i64(A[0]), _i64(LA[0])
    for mode in MODES:
        plain = _cross(e, mode, hdr, sids, rids)
        lplain = _plain_list(e, mode, hdr, fixed, lids)
        for tr in (ANY, GAINED, LOST):
            exp = expect_rows(vA, vB, tr, rids)
            total = int(exp[0][-1])
            for cap in (S * R, max(total - 1, 0)):
                out = _DOut(S * ((R + 31) // 32), cap, rows=S, err_cap=S * R)
                rev, got = _recheck_cross(e, mode, hdr, sids, rids, prev, tr, out)
                assert rev == rev0 + 1
                _agree(got, exp, cap, (family, mode, hex(tr), cap), rows=True)
                _same((got["words"], got["errs"], got["n_errs"]), plain, (family, mode))
                _same((got["words"], got["errs"], got["n_errs"]), B, (family, mode))
            lexp = expect_dense(vLA, vLB, tr, lids)
            for cap in (n, max(len(lexp[1]) - 1, 0)):
                out = _DOut((n + 31) // 32, cap, err_cap=n)
                rev, got = _recheck_list(e, mode, hdr, fixed, lids, lprev, tr, out)
                assert rev == rev0 + 1
                _agree(got, lexp, cap, (family, mode, hex(tr), cap))
                assert np.array_equal(got["words"], lplain[0]) and got["errs"] == lplain[1] and got["n_errs"] == lplain[2]
                assert np.array_equal(got["words"], LB[0])
        # a second recheck with no update in between, against the plane the first one wrote: no change
        out = _DOut(S * ((R + 31) // 32), S * R, rows=S)
        rev, got = _recheck_cross(e, mode, hdr, sids, rids, _i64(B[0]), ANY, out)
        assert rev == rev0 + 1 and got["total"] == 0 and not got["row_off"].any() and len(got["ids"]) == 0
        out = _DOut((n + 31) // 32, n)
        rev, got = _recheck_list(e, mode, hdr, fixed, lids, _i64(LB[0]), ANY, out)
        assert rev == rev0 + 1 and got["total"] == 0 and len(got["pos"]) == 0
    e.close()


def test_torch_and_client_forms():
    """Engine.recheck_ids / recheck_cross_ids chained through their own planes, and the Client forms'
    names and transitions, across the same Watch batch."""
    fam = _family("nested")
    users, docs, listed, lines, after = _scene(fam)
    e = fam.engine()
    hdr, sids, rids = _ids(e, SHAPE, users, docs)
    _, _, lids = _ids(e, SHAPE, users[:1], listed)
    S, R, n = len(users), len(docs), len(listed)
    vA = E.unpack_cross(_host(e, hdr, sids, rids)[0], S, R)
    vLA = E.unpack_results(_host_list(e, hdr, int(sids[0]), lids)[0], n)
    plane, rev, row_off, ids, col, trans = e.recheck_cross_ids(hdr, _u32(sids), _u32(rids), transitions=GAINED)
    exp = expect_rows(np.zeros_like(vA), vA, GAINED, rids)
    assert rev == 1 and np.array_equal(row_off.cpu().numpy().view(np.uint32), exp[0])
    assert np.array_equal(col.cpu().numpy().view(np.uint32), exp[2]) and np.array_equal(trans.cpu().numpy(), exp[3])
    lplane, rev, _, pos, _ = e.recheck_ids(hdr, int(sids[0]), R_, _u32(lids), transitions=GAINED)
    assert rev == 1 and np.array_equal(pos.cpu().numpy().view(np.uint32), np.flatnonzero(vLA >= 2))
    c = Client(e)
    (cplane, rev, changes), err = c.RecheckCrossDevice(None, None, "doc#view", docs, "user", users, transitions=GAINED)
    assert err is None and rev == 1 and torch.equal(cplane, plane)
    assert changes == [(users[s], docs[r], 0, int(vA[s, r])) for s in range(S) for r in range(R) if vA[s, r] >= 2]

    e.apply_updates_text(2, "\n".join(lines))
    vB = E.unpack_cross(_host(e, hdr, sids, rids)[0], S, R)
    vLB = E.unpack_results(_host_list(e, hdr, int(sids[0]), lids)[0], n)
    plane2, rev, row_off, ids, col, trans = e.recheck_cross_ids(hdr, _u32(sids), _u32(rids), prev=plane)
    exp = expect_rows(vA, vB, ANY, rids)
    assert rev == 2 and int(exp[0][-1]) > 0 and np.array_equal(row_off.cpu().numpy().view(np.uint32), exp[0])
    assert np.array_equal(ids.cpu().numpy().view(np.uint32), exp[1]) and np.array_equal(trans.cpu().numpy(), exp[3])
    _, rev, lids_out, pos, ltrans = e.recheck_ids(hdr, int(sids[0]), R_, _u32(lids), prev=lplane)
    lexp = expect_dense(vLA, vLB, ANY, lids)
    assert rev == 2 and np.array_equal(pos.cpu().numpy().view(np.uint32), lexp[1])
    assert np.array_equal(lids_out.cpu().numpy().view(np.uint32), lexp[0]) and np.array_equal(ltrans.cpu().numpy(), lexp[2])
    (_, rev, changes), err = c.RecheckCrossDevice(None, None, "doc#view", docs, "user", users, prev=cplane)
    assert err is None and rev == 2
    assert changes == [(users[s], docs[r], int(vA[s, r]), int(vB[s, r])) for s in range(S) for r in range(R)
                       if vA[s, r] != vB[s, r]]
    (_, rev, changes), err = c.RecheckResourcesDevice(None, None, "doc#view", f"user:{users[0]}", listed, prev=lplane,
                                                      transitions=LOST)
    assert err is None and rev == 2
    assert changes == [(listed[k], int(vLA[k]), int(vLB[k])) for k in range(n) if vLA[k] >= 2 and vLB[k] < 2] and changes
    (_, rev, changes), err = c.RecheckSubjectsDevice(None, None, f"doc:{docs[0]}", "view", "user", users)
    assert err is None and rev == 2
    assert changes == [(users[s], 0, int(vB[s, 0])) for s in range(S) if vB[s, 0]]
    e.close()


# ---- 3. a list that crosses a chunk boundary ---------------------------------------------------------

@pytest.mark.parametrize("workspaces", [1, 2])
def test_list_across_a_chunk_boundary(workspaces):
    """max_batch = 64: chunks of 64 ids, two plane words each. 100 ids, the docs that change for the
    user at positions 63 (the last word of chunk 0) and 64 (the first word of chunk 1) and further on."""
    fam = _family("nested")
    users, docs, _, lines, _ = _scene(fam)
    e = fam.engine(max_batch=64, workspaces=workspaces)
    hdr, sids, rids = _ids(e, SHAPE, users[:1], docs)
    fixed = int(sids[0])
    a = E.unpack_results(_host_list(e, hdr, fixed, rids)[0], len(docs))
    probe = fam.engine()
    probe.apply_updates_text(2, "\n".join(lines))
    b = E.unpack_results(_host_list(probe, hdr, fixed, rids)[0], len(docs))
    probe.close()
    moved, still = np.flatnonzero(a != b), np.flatnonzero(a == b)
    assert len(moved) >= 2 and len(still)
    n = 100
    pick = still[np.arange(n) % len(still)]
    for k, at in enumerate((40, 62, 63, 64, 65, 99)):
        pick[at] = moved[k % len(moved)]
    lids = rids[pick]
    assert n > (64 & ~31)
    LA = _host_list(e, hdr, fixed, lids)
    e.apply_updates_text(2, "\n".join(lines))
    LB = _host_list(e, hdr, fixed, lids)
    vLA, vLB = E.unpack_results(LA[0], n), E.unpack_results(LB[0], n)
    for tr in (ANY, GAINED, LOST):
        exp = expect_dense(vLA, vLB, tr, lids)
        if tr == ANY:
            assert {63, 64} <= set(exp[1].tolist())  # (both sides of the boundary)
        for cap in (n, max(len(exp[1]) - 1, 0)):
            out = _DOut((n + 31) // 32, cap, err_cap=n)
            rev, got = _recheck_list(e, "sync", hdr, fixed, lids, _i64(LA[0]), tr, out)
            assert rev == 2
            _agree(got, exp, cap, (workspaces, hex(tr), cap))  # (the ranks run on across the chunks)
            assert np.array_equal(got["words"], LB[0]) and got["n_errs"] == 0
    e.close()


# ---- 4. errors ------------------------------------------------------------------------------------------

def _deep():
    """A user eight groups below doc d0's and d2's viewers (beyond a depth budget of 5: the checks end
    in GCK_ITEM_ERR_MAX_DEPTH), directly in d1's group, and not in d3's."""
    L = 8
    t = ["doc:d0#viewer@group:g0#member", f"doc:d1#viewer@group:g{L}#member", "doc:d2#viewer@group:h0#member",
         "doc:d3#viewer@group:q#member", f"group:g{L}#member@user:deep", "group:q#member@user:other",
         f"group:h{L}#member@user:deep"]
    t += [f"group:g{i}#member@group:g{i + 1}#member" for i in range(L)]
    t += [f"group:h{i}#member@group:h{i + 1}#member" for i in range(L)]
    lines = ["DELETE group:g0#member@group:g1#member", "CREATE group:g0#member@user:deep", "CREATE group:q#member@user:deep"]
    after = [x for x in t if x != "group:g0#member@group:g1#member"] + ["group:g0#member@user:deep", "group:q#member@user:deep"]
    return t, lines, after


@pytest.mark.parametrize("mode", MODES)
def test_an_errored_check_that_became_valid(mode):
    schema = gen.FAMILIES["nested"](2)[0]
    tuples, lines, after = _deep()
    names = ["d0", "d1", "d2", "d3"]
    want_a = [(0, 1), (2, 0), (0, 1), (1, 0)]  # (perm, GCK_ITEM_*): errored, HAS, errored, NO
    want_b = [(2, 0), (2, 0), (0, 1), (2, 0)]  # d0 valid now, d2 errored still, d3 gained
    for tup, want in ((tuples, want_a), (after, want_b)):
        ck = oracle_for(schema, tup, max_depth=5, now=NOW_US / 1e6)
        assert [tuple(ck.check(to_oracle_item(rel.FromTriple(f"doc:{d}", "view", "user:deep"), None))) for d in names] == want
    e = E.Engine(device=0, max_depth=5)
    e.load_schema(schema)
    e.load_snapshot_text(1, "\n".join(tuples))
    hdr, sids, rids = _ids(e, SHAPE, ["deep"], names)
    fixed = int(sids[0])
    LA = _host_list(e, hdr, fixed, rids)
    assert E.unpack_results(LA[0], 4).tolist() == [0, 2, 0, 1] and LA[1] == [(0, 1), (2, 1)]
    e.apply_updates_text(2, "\n".join(lines))
    LB = _host_list(e, hdr, fixed, rids)
    assert E.unpack_results(LB[0], 4).tolist() == [2, 2, 0, 2] and LB[1] == [(2, 1)]
    bit = lambda v, w: 1 << (4 * v + w)
    # d0 went 0 -> 2 and d3 1 -> 2: each is reported only under its own bit
    for tr, pos, trans in ((bit(0, 2), [0], [2]), (bit(1, 2), [3], [6]), (GAINED, [0, 3], [2, 6]), (ANY, [0, 3], [2, 6]),
                           (bit(0, 3) | bit(0, 1) | LOST, [], []), (ANY & ~bit(0, 2), [3], [6])):
        out = _DOut(1, 4)
        rev, got = _recheck_list(e, mode, hdr, fixed, rids, _i64(LA[0]), tr, out)
        assert rev == 2 and got["pos"].tolist() == pos and got["trans"].tolist() == trans, hex(tr)
        assert got["ids"].tolist() == [int(rids[p]) for p in pos]
        assert got["n_errs"] == 1 and got["errs"] == [(2, 1)] and np.array_equal(got["words"], LB[0])
        # the cross form: one row
        out = _DOut(1, 4, rows=1)
        rev, got = _recheck_cross(e, mode, hdr, sids, rids, _i64(LA[0]), tr, out)
        assert rev == 2 and got["pos"].tolist() == pos and got["trans"].tolist() == trans, hex(tr)
        assert got["row_off"].tolist() == [0, len(pos)] and got["n_errs"] == 1
    e.close()


def test_refusals(nested_engine):
    e = nested_engine
    fam = _family("nested")
    res, sub = fam.shapes[SHAPE]
    hdr, sids, rids = _ids(e, SHAPE, sub[:3], res[:70])
    ds, dr = _u32(sids), _u32(rids)
    st = torch.cuda.current_stream().cuda_stream
    S, R, stride = 3, 70, 3
    n, words = 70, 3

    def refused(fn, *a, **kw):
        with pytest.raises(E.GckError) as ex:
            r = fn(*a, **kw)
            if hasattr(r, "wait"):
                r.wait()
        assert ex.value.code == E.GCK_E_INVALID_ARGUMENT, ex.value
        out.untouched()

    # the cross form: prev inside, at and one word before the new plane; the good neighbour passes
    out = _DOut(S * stride + 16, 8, rows=S)
    base = out.words.data_ptr()
    good = dict(out.args(), d_out_packed=base + 8 * 16, stream=st, now_us=NOW_US)
    head = (hdr, ds.data_ptr(), S, dr.data_ptr(), R)
    for fn in (e.recheck_cross_device, e.submit_recheck_cross_device):
        for prev in (base + 8 * 16, base + 8 * 17, base + 8 * (16 - S * stride + 1), base + 8 * (16 + S * stride - 1)):
            refused(fn, *head, prev, **good)
        refused(fn, *head, base + 4, **good)                                  # a plane that is not 8-byte aligned
        refused(fn, *head, 0, **dict(good, transitions=0))
        refused(fn, *head, 0, **dict(good, transitions=ANY | 1))
        refused(fn, *head, 0, **dict(good, d_out_packed=0))
        refused(fn, *head, 0, **dict(good, d_out_row_off=0))
        refused(fn, *head, 0, **dict(good, d_out_n=0))
        refused(fn, *head, 0, **dict(good, d_out_ids=0, d_out_col=0, d_out_trans=0))
        refused(fn, *head, 0, **dict(good, d_out_col=out.pos.data_ptr() + 2))
    # the list form likewise
    out = _DOut(words + 16, 8)
    base = out.words.data_ptr()
    good = dict(out.args(), d_out_packed=base + 8 * 16, d_ids=dr.data_ptr(), stream=st, now_us=NOW_US)
    head = (hdr, int(sids[0]), R_, n)
    for fn in (e.recheck_list_device, e.submit_recheck_list_device):
        for prev in (base + 8 * 16, base + 8 * 18, base + 8 * (16 - words + 1)):
            refused(fn, *head, prev, **good)
        refused(fn, *head, base + 4, **good)
        refused(fn, *head, 0, **dict(good, transitions=1 << 5))
        refused(fn, *head, 0, **dict(good, d_out_packed=0))
        refused(fn, *head, 0, **dict(good, d_out_n=0))
        refused(fn, *head, 0, **dict(good, d_out_ids=0, d_out_pos=0, d_out_trans=0))
        refused(fn, *head, 0, **dict(good, d_out_pos=out.pos.data_ptr() + 1))
        refused(fn, hdr, int(sids[0]), 3, n, 0, **good)                       # what the list call refuses: a bad vary
    # the plane-only calls
    refused(e.diff_planes_device, base, base, n, stream=st, **out.sel())
    refused(e.diff_planes_device, 0, 0, n, stream=st, **out.sel())
    refused(e.diff_cross_planes_device, base, base + 8, S, R, dr.data_ptr(), out.cnt.data_ptr(), out.cnt.data_ptr(), 8,
            d_out_ids=out.ids.data_ptr(), stream=st)
    # adjacent planes are no overlap: the good request runs
    rev = e.recheck_list_device(*head, base, **dict(good, d_out_packed=base + 8 * words))
    assert rev == e.revision


def test_stats_count_a_recheck_as_the_request_it_is(nested_engine):
    e = nested_engine
    fam = _family("nested")
    res, sub = fam.shapes[SHAPE]
    hdr, sids, rids = _ids(e, SHAPE, sub[:5], res[:40])
    before = sum(e.device_compact_stats())
    _cross(e, "sync", hdr, sids, rids)
    plain = sum(e.device_compact_stats()) - before
    out = _DOut(5 * 2, 200, rows=5)
    _recheck_cross(e, "sync", hdr, sids, rids, None, ANY, out)
    assert sum(e.device_compact_stats()) - before == 2 * plain and plain > 0
