"""Filter requests (include/gck.h gck_filter_list_device and its submit form): a list request over
device buffers whose survivors — ids, positions, Permissionships, and their number — are compacted
by a kernel into device arrays (torch tensors on cuda:0).

Bar, never the code under test: Engine.lookup_resources_among / lookup_subjects_among on the same
candidates (ids, perms, order under the lookup's rule), and a numpy selection from the unpacked plane
of Engine.check_list (positions, every mask, the error records); in test_family_parity the oracle's
answers too. Every output starts poisoned — ids, pos and perm with a sentinel and two entries beyond
cap, the plane with a word beyond it, the error list, both count words — and what the protocol
leaves untouched is asserted untouched."""
import itertools

import numpy as np
import pytest
import torch

from gochugaru_amd import consistency
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client
from tests.test_gpu_device_compact import (FAMS, MODES, NOW_US, POISON, SENT, R, S, _dev, _family, _plain, _records,
                                           _u32)

pytestmark = pytest.mark.gpu
SENT8 = 0xA5
LOOKUP, HAS, NO, COND = E.SELECT_LOOKUP, E.SELECT_HAS, E.SELECT_NO, E.SELECT_CONDITIONAL
ALL3 = ("ids", "pos", "perm")


class _FOut:
    """The device outputs of one filter request, poisoned: cap + 2 entries per wanted array, both
    count words, err_cap + 2 records, and (plane=True) n_words + 1 words."""

    def __init__(self, n, cap, which=ALL3, err_cap=4, plane=True):
        self.n, self.cap, self.which, self.err_cap = n, cap, tuple(which), err_cap
        self.nw = (n + 31) // 32
        self.ids = torch.full((cap + 2,), SENT, dtype=torch.int32, device=_dev()) if "ids" in which else None
        self.pos = torch.full((cap + 2,), SENT, dtype=torch.int32, device=_dev()) if "pos" in which else None
        self.perm = torch.full((cap + 2,), SENT8, dtype=torch.uint8, device=_dev()) if "perm" in which else None
        self.cnt = torch.full((2,), SENT, dtype=torch.int32, device=_dev())  # [survivors, errors]
        self.errs = torch.full((err_cap + 2, 2), SENT, dtype=torch.int32, device=_dev())
        self.words = torch.full((self.nw + 1,), -1, dtype=torch.int64, device=_dev()) if plane else None

    def args(self):
        p = lambda t: t.data_ptr() if t is not None else 0
        return dict(d_out_n=self.cnt.data_ptr(), cap=self.cap, d_out_ids=p(self.ids), d_out_pos=p(self.pos),
                    d_out_perm=p(self.perm), d_out_packed=p(self.words), d_out_errs=self.errs.data_ptr() if self.err_cap else 0,
                    err_cap=self.err_cap, d_out_n_errs=self.cnt.data_ptr() + 4)

    def read(self):
        """What was written, the poison beyond it asserted: total, ids / pos / perm (the first
        min(total, cap); None when not asked for), the records, the error count, the plane."""
        torch.cuda.synchronize()
        total, n_errs = (int(x) for x in self.cnt.cpu().numpy().view(np.uint32))
        assert total != SENT and n_errs != SENT, "a count word was not written"
        m = min(total, self.cap)
        got = {"total": total, "n_errs": n_errs}
        for name, t, sent in (("ids", self.ids, SENT), ("pos", self.pos, SENT), ("perm", self.perm, SENT8)):
            if t is None:
                got[name] = None
                continue
            a = t.cpu().numpy()
            a = a.view(np.uint32) if a.dtype == np.int32 else a
            assert (a[m:] == sent).all(), f"{name}: entries beyond min(total, cap) were written"
            got[name] = a[:m].copy()
        errs = self.errs.cpu().numpy()
        k = min(n_errs, self.err_cap)
        assert (errs[k:] == SENT).all(), "records beyond min(count, err_cap) were written"
        got["errs"] = [(int(np.uint32(i)), int(c)) for i, c in errs[:k]]
        if self.words is not None:
            w = self.words.cpu().numpy().view(np.uint64)
            assert int(w[self.nw]) == POISON, "the word after the plane was written"
            got["words"] = w[:self.nw].copy()
        return got


def _filter(e, mode, hdr, fixed, vary, n, out, ids=None, first=0, select=LOOKUP, contexts=None):
    d = _u32(ids) if ids is not None else None
    kw = dict(out.args(), select=select, d_ids=d.data_ptr() if d is not None and n else 0, first_id=first,
              now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    if mode == "sync":
        rev = e.filter_list_device(hdr, fixed, vary, n, stream=st, **kw)
    else:
        rev = e.submit_filter_list_device(hdr, fixed, vary, n, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read()


class _Yard:
    """The host yardstick of one list request: check_list's plane unpacked, its error records, the
    varying ids; select(mask) is the numpy selection."""

    def __init__(self, e, hdr, fixed, vary, ids=None, first=0, n=None, contexts=None):
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
            n = len(ids)
            words, errs, _ = e.check_list(hdr, fixed, vary, ids, now_us=NOW_US, contexts=contexts)
        else:
            words, errs, _ = e.check_list(hdr, fixed, vary, None, first, n, now_us=NOW_US, contexts=contexts)
        self.n = n
        self.words = np.asarray(words).copy()
        self.values = E.unpack_results(self.words, n)
        self.records = _records(errs)
        self.vids = ids if ids is not None else (first + np.arange(n)).astype(np.uint32)
        assert all(self.values[k] == 0 for k, _ in self.records)  # (an errored check is UNSPECIFIED in the plane)

    def select(self, mask):
        pos = np.flatnonzero((mask >> self.values.astype(np.uint32)) & 1).astype(np.uint32)
        return pos, self.vids[pos], self.values[pos]


def _agree(got, yard, mask, out, what=None):
    """A filter request's outputs against the yardstick's selection, under the cap protocol."""
    pos, ids, perm = yard.select(mask)
    assert got["total"] == len(pos), (what, got["total"], len(pos))
    m = min(len(pos), out.cap)
    for name, want in (("ids", ids), ("pos", pos), ("perm", perm)):
        if name in out.which:
            assert len(got[name]) == m and np.array_equal(got[name], want[:m]), (what, name, got[name][:8], want[:8])
        else:
            assert got[name] is None
    assert got["n_errs"] == len(yard.records), (what, got["n_errs"], yard.records[:4])
    assert got["errs"] == yard.records[:out.err_cap], (what, got["errs"], yard.records[:4])
    if "words" in got:
        assert np.array_equal(got["words"], yard.words), what


def _lookup(e, hdr, fixed, vary, vids):
    """The host lookup among the same candidates: (ids, perms), or the GckError it fails with."""
    try:
        if vary == R:
            return e.lookup_resources_among(hdr[0], hdr[1], hdr[2], hdr[3], fixed, vids, now_us=NOW_US)
        return e.lookup_subjects_among(hdr[0], fixed, hdr[1], hdr[2], vids, hdr[3], now_us=NOW_US)
    except E.GckError as ex:
        return ex


def _agree_lookup(got, e, hdr, fixed, vary, yard, what=None):
    """Under the lookup's rule: the host lookup's ids, perms and order — or, when a candidate has a
    per-item error, its failure (the device form reports the record and goes on)."""
    want = _lookup(e, hdr, fixed, vary, yard.vids)
    if yard.records:
        assert isinstance(want, E.GckError), what
        return
    assert np.array_equal(got["ids"], want[0]) and np.array_equal(got["perm"], want[1]), (what, got["ids"][:8], want[0][:8])


def _repeat(a, n):
    return np.concatenate([a] * (n // len(a) + 1))[:n].astype(np.uint32)


def _mix(e, hdr, p):
    """Of the subjects of the pairs p, the one the host yardstick gives the most even split of the
    pairs' resources: (its id, the resources it may see, those it may not)."""
    best = None
    for f in np.unique(p[:, 1]):
        y = _Yard(e, hdr, int(f), R, ids=np.unique(p[:, 0]))
        yes, no = y.vids[y.values >= E.PERM_HAS], y.vids[y.values == E.PERM_NO]
        if best is None or min(len(yes), len(no)) > min(len(best[1]), len(best[2])):
            best = (int(f), yes, no)
    assert len(best[1]) and len(best[2]), "no subject sees some of the resources and not others"
    return best


def _mixed(yes, no, n):
    """n candidates that repeat the ids: every third one of `yes`, the others of `no`."""
    return np.where(np.arange(n) % 3 == 0, _repeat(yes, n), _repeat(no, n)).astype(np.uint32)


# ---- 1. parity per family -------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMS)
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    # the shape of a check the oracle answers with an error where there is one, else the commonest
    bad = [k for k, (_, x) in enumerate(fam.want) if x]
    if family == "near_budget":
        assert bad, "near_budget has no per-item error at seed 2"
    k0 = bad[0] if bad else int(np.flatnonzero(shape_of == int(np.argmax(np.bincount(shape_of))))[0])
    j = int(shape_of[k0])
    hdr, at = shapes[j], np.flatnonzero(shape_of == j)
    res, sub = pairs[at, 0].copy(), pairs[at, 1].copy()
    r0, s0 = int(pairs[k0, 0]), int(pairs[k0, 1])
    oracle = {(int(pairs[k, 0]), int(pairs[k, 1])): fam.want[k] for k in at}
    m = min(e.object_count(hdr[0]), 45)
    lists = [("list R", s0, R, dict(ids=res)), ("list S", r0, S, dict(ids=sub)), ("range", s0, R, dict(first=0, n=m))]
    calls = 0
    n_errs = 0
    for what, fixed, vary, kw in lists:
        yard = _Yard(e, hdr, fixed, vary, **kw)
        n_errs += len(yard.records)
        for mask in (LOOKUP, HAS, NO):
            for mode in MODES:
                out = _FOut(yard.n, yard.n, err_cap=yard.n)
                got = _filter(e, mode, hdr, fixed, vary, yard.n, out, ids=kw.get("ids"), first=kw.get("first", 0),
                              select=mask)
                _agree(got, yard, mask, out, (family, what, mask, mode))
                calls += 1
                if mask == LOOKUP:
                    _agree_lookup(got, e, hdr, fixed, vary, yard, (family, what, mode))
                # the oracle, directly, where the list's check is one of the family's
                surv = set(int(p) for p in got["pos"])
                for i, v in enumerate(yard.vids):
                    key = (int(v), fixed) if vary == R else (fixed, int(v))
                    if key in oracle:
                        p, x = oracle[key]
                        assert (i in surv) == (not x and bool((mask >> p) & 1)), (family, what, mask, mode, i, p, x)
                for i, _ in yard.records:
                    assert i not in surv
    if family == "near_budget":
        assert n_errs >= 1, "no per-item error on the host yardstick"
    e.close()


# ---- 2. edges -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nested():
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shapes, shape_of, pairs = fam.request(e)
    yield fam, e, shapes, shape_of, pairs
    e.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193])
def test_edges(nested, n):
    """Word edges, and one block's tile of 256 words +- 1: the smallest size at which a second
    block's recount of the words before its tile can be wrong."""
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    fixed, yes, no = _mix(e, shapes[j], p)
    ids = _mixed(yes, no, n)
    yard = _Yard(e, shapes[j], fixed, R, ids=ids)
    assert len(yard.select(LOOKUP)[0]) == (n + 2) // 3
    s0 = e.device_compact_stats()
    for mode in ("engine", "sync"):
        out = _FOut(n, n)
        got = _filter(e, mode, shapes[j], fixed, R, n, out, ids=ids)
        _agree(got, yard, LOOKUP, out, (n, mode))
        _agree_lookup(got, e, shapes[j], fixed, R, yard, (n, mode))
    assert e.device_compact_stats() == (s0[0] + 2, s0[1])  # every chunk in place


# ---- 3. the cap protocol --------------------------------------------------------------------------

def test_cap_protocol(nested):
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    n = 200
    fixed, yes, no = _mix(e, shapes[j], p)
    ids = _mixed(yes, no, n)
    yard = _Yard(e, shapes[j], fixed, R, ids=ids)
    total = len(yard.select(LOOKUP)[0])
    assert 2 <= total < n
    subsets = [c for k in (1, 2, 3) for c in itertools.combinations(ALL3, k)]
    for k, cap in enumerate((0, 1, total - 1, total, total + 5)):
        for which in subsets + ([()] if cap == 0 else []):
            out = _FOut(n, cap, which, plane=bool(k % 2))  # (with and without a plane of the caller's)
            got = _filter(e, MODES[(k + len(which)) % 3], shapes[j], fixed, R, n, out, ids=ids)
            _agree(got, yard, LOOKUP, out, (cap, which))
            assert got["total"] == total
    # no survivors: candidates the yardstick answers NO, under HAS
    none = _repeat(no, 70)
    y0 = _Yard(e, shapes[j], fixed, R, ids=none)
    assert len(y0.select(HAS)[0]) == 0
    for mode in MODES:
        out = _FOut(70, 8)
        got = _filter(e, mode, shapes[j], fixed, R, 70, out, ids=none, select=HAS)
        _agree(got, y0, HAS, out, ("none", mode))
        assert got["total"] == 0
        # n == 0: both counts are written as 0, nothing else
        out = _FOut(0, 3, plane=False)
        got = _filter(e, mode, shapes[j], fixed, R, 0, out, ids=np.zeros(0, dtype=np.uint32))
        assert got["total"] == 0 and got["n_errs"] == 0 and len(got["ids"]) == 0


# ---- 4. chunks in order ---------------------------------------------------------------------------

@pytest.mark.parametrize("workspaces", [0, 1], ids=["two-workspaces", "one-workspace"])
def test_chunks_in_order(workspaces):
    fam = _family("nested")
    e = fam.engine(max_batch=64, workspaces=workspaces)
    shapes, shape_of, pairs = fam.request(e)
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    fixed, yes, no = _mix(e, shapes[j], p)
    n = 64 * 4 + 40  # five chunks: the running total crosses both workspaces and both parities
    mixed = lambda k: _mixed(yes, no, k)
    # survivors from the first and the last chunk and from no middle one
    ends = np.concatenate([mixed(64), _repeat(no, 192), mixed(40)])
    # ... and from every chunk
    every = mixed(n)
    s0 = e.device_compact_stats()
    runs = 0
    for what, ids in (("ends", ends), ("every", every)):
        yard = _Yard(e, shapes[j], fixed, R, ids=ids)
        pos = yard.select(LOOKUP)[0]
        total = len(pos)
        per_chunk = [int(np.count_nonzero(pos // 64 == c)) for c in range(5)]
        if what == "ends":
            assert per_chunk[0] and per_chunk[4] and per_chunk[1:4] == [0, 0, 0]
            caps = (total, total - 2, per_chunk[0])  # whole; cut inside the last chunk; exactly the first chunk's
        else:
            assert all(per_chunk)
            caps = (total, per_chunk[0] + per_chunk[1] + per_chunk[2] // 2, 0)  # ... a cap that falls inside the third chunk
        for cap in caps:
            out = _FOut(n, cap)
            got = _filter(e, "sync", shapes[j], fixed, R, n, out, ids=ids)
            _agree(got, yard, LOOKUP, out, (what, cap))
            runs += 1
        out = _FOut(n, total)
        _agree_lookup(_filter(e, "sync", shapes[j], fixed, R, n, out, ids=ids), e, shapes[j], fixed, R, yard, what)
        runs += 1
    assert e.device_compact_stats() == (s0[0] + 5 * runs, s0[1])
    # a range across chunks, without a plane of the caller's
    m = min(e.object_count(shapes[j][0]), n)
    assert m > 64
    yard = _Yard(e, shapes[j], fixed, R, first=0, n=m)
    out = _FOut(m, m, plane=False)
    _agree(_filter(e, "sync", shapes[j], fixed, R, m, out, first=0), yard, LOOKUP, out, "range")
    e.close()


# ---- 5. deferred checks before the select ---------------------------------------------------------

def test_deferred_checks_before_the_select():
    """The userset-subject shape of test_deferred_checks_share_a_word as a vary-resource list of 40
    with the userset as the fixed subject: the join leaves checks to the bundle stages, k_dc_patch
    puts their answers into the plane, and the select must run after it. (The vary-resource shape,
    not its mirror.) More survivors than checks the join decided: one of them was a left check."""
    fam = _family("gdocs")
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    userset = [j for j, s in enumerate(shapes) if s[3] != E.ELLIPSIS]
    assert userset
    j = userset[0]
    p = pairs[np.flatnonzero(shape_of == j)]
    yards = [(int(f), _Yard(e, shapes[j], int(f), R, ids=_repeat(p[:, 0], 40))) for f in np.unique(p[:, 1])]
    fixed, yard = max(yards, key=lambda fy: len(fy[1].select(LOOKUP)[0]))
    total = len(yard.select(LOOKUP)[0])
    for mode in MODES:
        e.reset_stats()
        s0 = e.device_compact_stats()
        out = _FOut(40, 40)
        got = _filter(e, mode, shapes[j], fixed, R, 40, out, ids=yard.vids)
        st = e.stats()
        left = st["queries"] - st["closure_checks"]
        print(f"{mode}: {left} of {st['queries']} checks left by the join, {total} survivors")
        assert e.device_compact_stats() == (s0[0] + 1, s0[1]), "not in place"
        assert st["queries"] == 40 and left >= 3
        assert total > 40 - left, "no survivor is certain to be among the checks the join left"
        _agree(got, yard, LOOKUP, out, mode)
        _agree_lookup(got, e, shapes[j], fixed, R, yard, mode)
    e.close()


# ---- 6. expanded paths ----------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"labels": False}, {"closure": False, "labels": False}, {"wide_only": True},
                                {"profile": True}], ids=["no-labels", "no-join", "wide-only", "profiling"])
def test_every_engine_path(kw):
    fam = _family("gdocs")
    e = fam.engine(**kw)
    shapes, shape_of, pairs = fam.request(e)
    j = int(np.argmax(np.bincount(shape_of)))
    p = pairs[np.flatnonzero(shape_of == j)]
    fixed, ids = int(p[0, 1]), p[:, 0].copy()
    yard = _Yard(e, shapes[j], fixed, R, ids=ids)
    s0 = e.device_compact_stats()
    for k, mode in enumerate(MODES):
        out = _FOut(len(ids), len(ids), plane=bool(k % 2))
        got = _filter(e, mode, shapes[j], fixed, R, len(ids), out, ids=ids)
        _agree(got, yard, LOOKUP, out, (kw, mode))
        _agree_lookup(got, e, shapes[j], fixed, R, yard, (kw, mode))
    m = min(e.object_count(shapes[j][0]), 40)
    yr = _Yard(e, shapes[j], fixed, R, first=0, n=m)
    out = _FOut(m, m)
    _agree(_filter(e, "sync", shapes[j], fixed, R, m, out, first=0, select=NO), yr, NO, out, (kw, "range"))
    s1 = e.device_compact_stats()
    if kw == {"labels": False}:
        assert sum(s1) == sum(s0) + 4
    else:
        assert s1 == (s0[0], s0[1] + 4)  # expanded on the device: k_dc_pack wrote the plane the select read
    e.close()


def test_check_contexts():
    """Check contexts run expanded. A header at slot 0 leaves the caveats' parameters open:
    CONDITIONAL survivors appear under LOOKUP and not under HAS."""
    fam = _family("caveated")
    e = fam.engine()
    ctxs = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]
    shapes, shape_of, pairs = fam.request(e)
    # the shape and the subjects of checks the oracle answers CONDITIONAL without a context
    open_k = [k for k, (v, x) in enumerate(fam.want) if v == E.PERM_CONDITIONAL and not x]
    assert open_k
    j = int(shape_of[open_k[0]])
    p = pairs[np.flatnonzero(shape_of == j)]
    ids = p[:, 0].copy()
    subjects = np.unique([pairs[k, 1] for k in open_k if shape_of[k] == j])[:3]
    seen_cond = False
    s0 = e.device_compact_stats()
    calls = 0
    for slot in (0, 1, 2):
        hdr = shapes[j][:4] + (slot,)
        for fixed in subjects:
            yard = _Yard(e, hdr, int(fixed), R, ids=ids, contexts=ctxs)
            cond = set(np.flatnonzero(yard.values == E.PERM_CONDITIONAL).tolist())
            seen_cond = seen_cond or bool(cond)
            for mask, mode in ((LOOKUP, "sync"), (HAS, "engine"), (COND, "stream")):
                out = _FOut(len(ids), len(ids))
                got = _filter(e, mode, hdr, int(fixed), R, len(ids), out, ids=ids, select=mask, contexts=ctxs)
                _agree(got, yard, mask, out, (slot, mask))
                calls += 1
                surv = set(int(x) for x in got["pos"])
                assert cond <= surv if mask != HAS else not (cond & surv)
    assert seen_cond, "no CONDITIONAL answer on the host yardstick"
    assert e.device_compact_stats() == (s0[0], s0[1] + calls)
    e.close()


# ---- 7. refusals before any launch ----------------------------------------------------------------

def test_refusals(nested):
    fam, e, shapes, shape_of, pairs = nested
    hdr = shapes[_plain(shapes, shape_of)]
    n = 64
    big = torch.zeros(4 * n + 8, dtype=torch.int32, device=_dev())
    outs = torch.zeros(4 * n + 8, dtype=torch.int32, device=_dev())
    words = torch.zeros(n, dtype=torch.int64, device=_dev())
    errs = torch.zeros((n + 1, 2), dtype=torch.int32, device=_dev())
    cnt = torch.zeros(4, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    P, O, W, X, N = big.data_ptr(), outs.data_ptr(), words.data_ptr(), errs.data_ptr(), cnt.data_ptr()
    s0 = e.device_compact_stats()
    b0 = e.stats()["batches"]
    lib = e._lib

    def refused(fn, *a, **k):
        with pytest.raises(E.GckError) as ei:
            r = fn(*a, **k)
            if hasattr(r, "wait"):
                r.wait()
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        return ei.value.message

    good = dict(d_out_n=N, cap=n, d_out_ids=O, d_ids=P, d_out_packed=W, d_out_errs=X, err_cap=n, d_out_n_errs=N + 4)
    for fn in (e.filter_list_device, e.submit_filter_list_device):
        call = lambda vary=R, fixed=0, h=hdr, **k: refused(fn, h, fixed, vary, n, **{**good, **k})
        for mask in (0, 1, 3, 5, 0xF, 0x10, 0x1E):  # 0, GCK_PERM_UNSPECIFIED selected, above 0xE
            assert "mask" in call(select=mask)
        assert "d_out_n" in call(d_out_n=0)
        assert "cap" in call(d_out_ids=0)                                  # cap > 0 with all three arrays NULL
        call(d_out_ids=O + 2)                                              # misaligned ids / pos / count
        call(d_out_ids=0, d_out_pos=O + 1)
        call(d_out_n=N + 2)
        # everything the list device call refuses
        call(vary=S, d_ids=0)                                              # a range with VARY_SUBJECT
        call(vary=3)                                                       # vary neither value
        call(d_ids=P + 2)                                                  # misaligned ids
        call(h=E.Uniform(*hdr[:4], 0, 7))                                  # reserved != 0
        call(fixed=0, d_ids=0, first_id=0xFFFFFFF0)                        # a range past 2^32
        call(d_out_packed=W + 4)                                           # misaligned plane
        call(d_out_errs=X + 2)
        call(d_out_n_errs=N + 6)
        call(d_out_errs=0)                                                 # err_cap without a list
        call(h=hdr[:4] + (1,))                                             # a slot beyond the contexts
    # sel == NULL and reserved != 0, through the C entry point itself
    cs = E._Consistency(E.CONSISTENCY_MIN_LATENCY, 0, 0)
    h = E._header(hdr)
    rev = E.C.c_uint64(0)
    for sel in (None, E.Select(LOOKUP, 1, O, None, None, n, N)):
        rc = lib.gck_filter_list_device(e._h, E.C.byref(cs), E.C.byref(h), 0, R, P, 0, n, None, None, 0, NOW_US,
                                        E.C.byref(sel) if sel is not None else None, W, X, n, N + 4, None, E.C.byref(rev))
        assert rc == E.GCK_E_INVALID_ARGUMENT
        b = E._P()
        rc = lib.gck_filter_submit_list_device(e._h, E.C.byref(cs), E.C.byref(h), 0, R, P, 0, n, None, None, 0, NOW_US,
                                               E.C.byref(sel) if sel is not None else None, W, X, n, N + 4, 0, None,
                                               E.C.byref(b))
        assert rc == E.GCK_E_INVALID_ARGUMENT and not b.value
    small = fam.engine(max_batch=32, workspaces=1)
    refused(small.submit_filter_list_device, hdr, 0, R, 33, **good)        # a submit above max_batch
    small.close()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran
    torch.cuda.synchronize()
    assert int(outs.abs().sum()) == 0 and int(cnt.abs().sum()) == 0 and int(words.abs().sum()) == 0  # nothing written


# ---- 8. in flight ---------------------------------------------------------------------------------

def test_eight_in_flight_waited_in_reverse(nested):
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    fixed, yes, no = _mix(e, shapes[j], p)
    subjects = [fixed] + [int(f) for f in np.unique(p[:, 1])[:3]]
    n = 300
    reqs = []
    for k in range(40):
        ids = np.roll(_mixed(yes, no, n), k // 4)[:n - k]  # (requests of different lengths and answers)
        reqs.append((subjects[k % 4], ids, _u32(ids)))
    yards = {}
    for fixed, ids, _ in reqs:  # (one yardstick per distinct request)
        key = (fixed, ids.tobytes())
        if key not in yards:
            yards[key] = _Yard(e, shapes[j], fixed, R, ids=ids)
    yard = lambda k: yards[(reqs[k][0], reqs[k][1].tobytes())]
    assert len({len(y.select(LOOKUP)[0]) for y in yards.values()}) > 1  # (the requests differ)
    outs = [_FOut(len(reqs[k][1]), n, plane=bool(k % 2)) for k in range(8)]
    torch.cuda.synchronize()
    s0 = e.device_compact_stats()
    bs = [e.submit_filter_list_device(shapes[j], reqs[k][0], R, len(reqs[k][1]), d_ids=reqs[k][2].data_ptr(), engine_stream=True,
                                      now_us=NOW_US, **outs[k].args()) for k in range(8)]
    for b in reversed(bs):
        assert b.wait() == e.revision
    for k, o in enumerate(outs):
        _agree(o.read(), yard(k), LOOKUP, o, k)
    assert e.device_compact_stats() == (s0[0] + 8, s0[1])
    # the compiled loop: 40 requests, 8 in flight, every request's survivors
    outs = [_FOut(len(r[1]), n, plane=False) for r in reqs]
    torch.cuda.synchronize()
    loop = e.prepare_filter_device([shapes[j]] * 40, [r[0] for r in reqs], R, [r[2].data_ptr() for r in reqs], [0] * 40,
                                   [len(r[1]) for r in reqs], [o.cnt.data_ptr() for o in outs], n, 8,
                                   out_ids=[o.ids.data_ptr() for o in outs], out_pos=[o.pos.data_ptr() for o in outs],
                                   out_perm=[o.perm.data_ptr() for o in outs],
                                   errs=[o.errs.data_ptr() for o in outs], err_cap=4,
                                   n_errs=[o.cnt.data_ptr() + 4 for o in outs], now_us=NOW_US)
    assert loop.run() > 0
    for k, o in enumerate(outs):
        _agree(o.read(), yard(k), LOOKUP, o, ("loop", k))


# ---- 9. the Python layers -------------------------------------------------------------------------

def test_filter_ids():
    fam = _family("near_budget")
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    bad = [k for k, (_, x) in enumerate(fam.want) if x]
    assert bad
    k0 = bad[0]
    j = int(shape_of[k0])
    at = np.flatnonzero(shape_of == j)
    res, fixed = pairs[at, 0].copy(), int(pairs[k0, 1])
    yard = _Yard(e, shapes[j], fixed, R, ids=res)
    assert yard.records
    with pytest.raises(E.GckError) as ei:
        e.filter_ids(shapes[j], fixed, R, _u32(res), now_us=NOW_US)
    want = _lookup(e, shapes[j], fixed, R, res)
    assert isinstance(want, E.GckError) and ei.value.message == want.message and ei.value.code == want.code
    # without the errored candidates: tensors equal to the yardstick, on the device
    ok = np.delete(res, [k for k, _ in yard.records])
    yard = _Yard(e, shapes[j], fixed, R, ids=ok)
    assert not yard.records
    for mask in (LOOKUP, NO):
        pos, ids, perm = yard.select(mask)
        for dtype in (torch.int32, torch.uint32):
            got = e.filter_ids(shapes[j], fixed, R, _u32(ok).view(dtype), select=mask, want_pos=True, want_perm=True,
                               now_us=NOW_US)
            assert all(t.is_cuda for t in got) and got[0].dtype == dtype
            assert np.array_equal(got[0].view(torch.int32).cpu().numpy().view(np.uint32), ids)
            assert np.array_equal(got[1].cpu().numpy().view(np.uint32), pos)
            assert np.array_equal(got[2].cpu().numpy(), perm)
    got = e.filter_ids(shapes[j], fixed, R, _u32(ok), now_us=NOW_US)
    assert isinstance(got, torch.Tensor) and np.array_equal(got.cpu().numpy().view(np.uint32), _lookup(e, shapes[j], fixed, R, ok)[0])
    # a range
    m = min(e.object_count(shapes[j][0]), 40)
    yr = _Yard(e, shapes[j], fixed, R, first=0, n=m)
    if not yr.records:
        got = e.filter_ids(shapes[j], fixed, R, None, first_id=0, n=m, now_us=NOW_US)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), yr.select(LOOKUP)[1])
    e.close()


def _names(e, type_name, ids):
    t = e.type_id(type_name)
    return [e.object_name(t, int(i)) for i in ids.view(torch.int32).cpu().numpy().view(np.uint32)]


def test_client_filters():
    # the README founders graph
    e = E.Engine(device=0)
    e.load_schema("definition user {}\ndefinition company { relation founder: user }")
    e.load_snapshot_text(1, "\n".join(f"company:authzed#founder@user:{u}" for u in ("jake", "joey", "jimmy")))
    c = Client(e)
    cs = consistency.MinLatency()
    users = ["jake", "nobody", "jimmy", "jake"]  # (an unknown name, a repeated id)
    cand = _u32(e.intern(e.type_id("user"), users))
    got, err = c.FilterSubjectsDevice(None, cs, "company:authzed", "founder", "user", cand)
    want = list(c.FilterSubjects(None, cs, "company:authzed", "founder", ["user:" + u for u in users]))
    assert err is None and all(x is None for _, x in want)
    assert _names(e, "user", got) == [n for n, _ in want] == ["jake", "jimmy", "jake"]
    comp = _u32(e.intern(e.type_id("company"), ["authzed", "authzed"]))
    got, err = c.FilterResourcesDevice(None, cs, "company#founder", "user:joey", comp)
    want = list(c.FilterResources(None, cs, "company#founder", "user:joey", ["company:authzed"] * 2))
    assert err is None and _names(e, "company", got) == [n for n, _ in want] == ["authzed", "authzed"]
    # an unknown permission is the error of both; an empty tensor is an empty answer
    got, err = c.FilterResourcesDevice(None, cs, "company#owner", "user:joey", comp)
    want = list(c.FilterResources(None, cs, "company#owner", "user:joey", ["company:authzed"]))
    assert got is None and isinstance(err, E.GckError) and isinstance(want[0][1], E.GckError)
    assert err.code == want[0][1].code == E.GCK_E_NOT_FOUND
    got, err = c.FilterSubjectsDevice(None, cs, "company:authzed", "founder", "user", cand[:0])
    assert err is None and got.numel() == 0
    got, err = c.FilterSubjectsDevice(None, cs, "company:authzed", "founder", "user", [1, 2])  # not a device tensor
    assert got is None and err is not None
    e.close()
    # one gdocs subject
    fam = _family("gdocs")
    e = fam.engine()
    c = Client(e)
    chk = next(k for k in fam.checks if k.startswith("doc:") and "#view@user:" in k and not k.endswith("*"))
    subject = chk.split("@", 1)[1]
    docs = sorted({k.split("#", 1)[0] for k in fam.checks if k.startswith("doc:")})
    docs = docs + docs[:3]
    cand = _u32(e.intern(e.type_id("doc"), [d.split(":", 1)[1] for d in docs]))
    got, err = c.FilterResourcesDevice(None, cs, "doc#view", subject, cand)
    want = list(c.FilterResources(None, cs, "doc#view", subject, docs))
    assert err is None and all(x is None for _, x in want)
    assert _names(e, "doc", got) == [n for n, _ in want]
    users = sorted({k.split("@user:", 1)[1] for k in fam.checks if "@user:" in k and not k.endswith("*")})
    cand = _u32(e.intern(e.type_id("user"), users))
    doc = chk.split("#", 1)[0]
    got, err = c.FilterSubjectsDevice(None, cs, doc, "view", "user", cand)
    want = list(c.FilterSubjects(None, cs, doc, "view", ["user:" + u for u in users]))
    assert err is None and _names(e, "user", got) == [n for n, _ in want]
    e.close()
