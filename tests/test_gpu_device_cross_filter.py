"""Cross filter requests (include/gck.h gck_filter_cross_device and its submit form): the cross device
request with each subject's survivors compacted by kernels into a CSR in device memory (torch tensors
on cuda:0).

Bar, never the code under test: the host cross call's plane on the same request, unpacked with
unpack_cross, then a numpy per-row selection (tests/test_select_rows.py expect) — and, in the family
test, the oracle's answer of every (subject, resource). The plane and the error records must equal the
plain cross device call's bit for bit. Every output starts poisoned — the records with two entries
beyond cap, row_off with an entry beyond S + 1, row_n with one beyond S, the plane with a word beyond
it, the error list and both count words — and whatever the protocol leaves untouched must stay so."""
import itertools

import numpy as np
import pytest
import torch

from gochugaru_amd import consistency
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client
from tests.helpers import load_golden
from tests.test_gpu_device_cross import (CTXS, MODES, NOW_US, SENT, _bad_permission, _cross, _dev, _family, _host, _ids,
                                         _nested_lists, _Out, _plane, _same, _u32)
from tests.test_select_rows import expect

pytestmark = pytest.mark.gpu
P8 = 0xA5
ALL = ("ids", "col", "perm")


class _Csr:
    """The device CSR outputs of one request, poisoned: S + 2 offsets, S + 1 row counts, cap + 2
    records per array, the count word."""

    def __init__(self, S, cap, arrays=ALL, row_n=True):
        i32 = lambda n: torch.full((n,), SENT, dtype=torch.int32, device=_dev())
        self.S, self.cap, self.arrays = S, cap, arrays
        self.row_off, self.n = i32(S + 2), i32(1)
        self.row_n = i32(S + 1) if row_n else None
        self.ids = i32(cap + 2) if "ids" in arrays else None
        self.col = i32(cap + 2) if "col" in arrays else None
        self.perm = torch.full((cap + 2,), P8, dtype=torch.uint8, device=_dev()) if "perm" in arrays else None

    def args(self):
        p = lambda t: 0 if t is None else t.data_ptr()
        return dict(d_out_row_off=self.row_off.data_ptr(), d_out_n=self.n.data_ptr(), cap=self.cap, d_out_ids=p(self.ids),
                    d_out_col=p(self.col), d_out_perm=p(self.perm), d_out_row_n=p(self.row_n))

    def _np(self, t):
        a = t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def untouched(self):
        torch.cuda.synchronize()
        for t in (self.row_off, self.n, self.row_n, self.ids, self.col):
            assert t is None or (self._np(t) == SENT).all()
        assert self.perm is None or (self._np(self.perm) == P8).all()

    def read(self):
        """{"row_off": S + 1, "row_n": S or None, "n", "ids" / "col" / "perm": the first min(n, cap) or
        None}; the poison beyond each is asserted here."""
        torch.cuda.synchronize()
        S, ro, n = self.S, self._np(self.row_off), int(self._np(self.n)[0])
        assert n != SENT, "the count word was not written"
        assert (ro[S + 1:] == SENT).all(), "row_off beyond S + 1 was written"
        out = {"row_off": ro[:S + 1].copy(), "n": n, "row_n": None}
        if self.row_n is not None:
            rn = self._np(self.row_n)
            assert (rn[S:] == SENT).all(), "row_n beyond S was written"
            out["row_n"] = rn[:S].copy()
        k = min(n, self.cap)
        for name, poison in (("ids", SENT), ("col", SENT), ("perm", P8)):
            t = getattr(self, name)
            out[name] = None
            if t is not None:
                a = self._np(t)
                assert (a[k:] == poison).all(), f"{name} beyond min(total, cap) was written"
                out[name] = a[:k].copy()
        return out


def _filter(e, mode, hdr, sids, rids, select=E.SELECT_LOOKUP, row_limit=0, cap=None, arrays=ALL, row_n=True,
            err_cap=None, count=True, contexts=None, block=False):
    """One cross filter request: ((words, records written, count or None), the CSR read back)."""
    S, R = len(sids), len(rids)
    if block:
        keep, ds, dr = E.cross_id_block(_u32(sids), _u32(rids))
    else:
        ds, dr = _u32(sids), _u32(rids)
    out = _Out(S, R, S * R if err_cap is None else err_cap, count)
    csr = _Csr(S, S * R if cap is None else cap, arrays, row_n)
    kw = dict(out.args(), **csr.args(), select=select, row_limit=row_limit, now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, ds.data_ptr() if S * R else 0, S, dr.data_ptr() if S * R else 0, R)
    if mode == "sync":
        rev = e.filter_cross_device(*head, stream=st, **kw)
    else:
        rev = e.submit_filter_cross_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read(), csr.read()


def _yard(e, hdr, sids, rids, contexts=None):
    """The host cross call on the request: ((words, records, count), perm[S, R] with 0 for an error)."""
    host = _host(e, hdr, sids, rids, contexts=contexts)
    return host, E.unpack_cross(host[0], len(sids), len(rids))


def _check(csr, perm, rids, select, row_limit, cap, what=None):
    """The CSR read back against the numpy selection over the yardstick's perm[S, R]."""
    row_off, row_n, ids, col, pm = expect(perm, np.asarray(rids, dtype=np.uint32), select, row_limit)
    total = int(row_off[-1])
    assert csr["n"] == total, (what, csr["n"], total)
    assert np.array_equal(csr["row_off"], row_off), (what, csr["row_off"][:8], row_off[:8])
    if csr["row_n"] is not None:
        assert np.array_equal(csr["row_n"], row_n), (what, csr["row_n"][:8], row_n[:8])  # unclipped
    k = min(total, cap)
    for name, full in (("ids", ids), ("col", col), ("perm", pm)):
        if csr[name] is not None:
            assert len(csr[name]) == k and np.array_equal(csr[name], full[:k]), (what, name, csr[name][:8], full[:8])
    return total


# ---- 1. every family, against the host call, the cross device call and the oracle -----------------

@pytest.mark.parametrize("family", ["nested", "gdocs", "caveated", "near_budget"])
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    n_records = n_rows_looked_up = 0
    for j, (shape, (res, sub)) in enumerate(fam.shapes.items()):
        hdr, sids, rids = _ids(e, shape, sub, res)
        S, R = len(sids), len(rids)
        host, perm = _yard(e, hdr, sids, rids)
        wp, we = fam.want(shape, sub, res)
        assert np.array_equal(perm, wp) and host[1] == we, (family, shape)  # the yardstick itself
        for mode in (MODES if j == 0 else [MODES[j % 3]]):
            plain = _cross(e, mode, hdr, sids, rids)
            for select in (E.SELECT_LOOKUP, E.SELECT_NO):
                got, csr = _filter(e, mode, hdr, sids, rids, select=select)
                # the plane and the error records: the cross device call's, bit for bit
                assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and got[2] == plain[2]
                _same(got, host, (family, shape, mode))
                _check(csr, perm, rids, select, 0, S * R, (family, shape, mode, select))
                for idx, _ in got[1]:  # no errored check survives
                    s, r = divmod(idx, R)
                    assert r not in csr["col"][csr["row_off"][s]:csr["row_off"][s + 1]].tolist(), (family, shape, idx)
            n_records += len(plain[1])
        # one row per request: the row's ids are lookup_resources_among's over the same candidates
        got, csr = _filter(e, MODES[j % 3], hdr, sids[:1], rids)
        try:
            want_ids, want_perm = e.lookup_resources_among(*hdr, int(sids[0]), rids, now_us=NOW_US)
        except E.GckError:  # (a per-item error fails that call)
            assert got[2] > 0
        else:
            assert np.array_equal(csr["ids"], want_ids) and np.array_equal(csr["perm"], want_perm), (family, shape)
            assert csr["row_off"].tolist() == [0, len(want_ids)]
            n_rows_looked_up += 1
    print(family, "error records", n_records, "rows compared with lookup_resources_among", n_rows_looked_up)
    if family == "near_budget":
        assert n_records > 0, "near_budget gave no error record"
    else:
        assert n_rows_looked_up > 0
    e.close()


# ---- 2. the lane mapping: every group width, ragged waves, the block layout -----------------------

def test_lane_mapping_edges():
    """R = 1 .. 200 gives L = 1, 1, 1, 2, 4 and 8 lanes per row; 9 rows at L = 8 make a ragged second
    wave, 5 rows at L = 1 .. 4 a wave with idle groups."""
    fam = _family("nested")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    k = 0
    partial = differ = False
    for R in (1, 31, 32, 33, 65, 200):
        for S in (1, 2, 5, 9):
            # (the first subject of the family sees nothing: the lists begin at the second)
            sub = [sub_all[(1 + j) % len(sub_all)] for j in range(S)]
            res = [res_all[j % len(res_all)] for j in range(R)]
            hdr, sids, rids = _ids(e, shape, sub, res)
            host, perm = _yard(e, hdr, sids, rids)
            assert np.array_equal(perm, fam.want(shape, sub, res)[0])
            surv = ((E.SELECT_LOOKUP >> perm) & 1).sum(axis=1)
            if R >= 31:  # the yardstick is not degenerate: a row partly kept, and rows that differ
                assert ((surv > 0) & (surv < R)).any(), (S, R, surv)
                partial = True
            if S >= 2 and R >= 31:
                assert len(set(surv.tolist())) > 1, (S, R, surv)
                differ = True
            for block in (False, True):
                mode = MODES[k % 3]
                k += 1
                select = (E.SELECT_LOOKUP, E.SELECT_NO, E.SELECT_HAS | E.SELECT_NO)[k % 3]
                got, csr = _filter(e, mode, hdr, sids, rids, select=select, block=block)
                _same(got, host, (S, R, mode, block))
                _check(csr, perm, rids, select, 0, S * R, (S, R, mode, block, select))
    assert partial and differ
    assert e.device_compact_stats() == (k, 0)  # every request ran in place
    e.close()


# ---- 3. row_limit and cap -------------------------------------------------------------------------

def test_row_limit_and_cap():
    fam = _family("nested")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    sub = [sub_all[(1 + j) % len(sub_all)] for j in range(5)]
    res = [res_all[j % len(res_all)] for j in range(65)]
    hdr, sids, rids = _ids(e, shape, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    surv = ((E.SELECT_LOOKUP >> perm) & 1).sum(axis=1)
    assert surv.max() > 3 and len(set(surv.tolist())) > 1, surv  # a limit of 3 clips some row
    k = 0
    for row_limit in (0, 1, 3, 65):
        total = int(expect(perm, rids, E.SELECT_LOOKUP, row_limit)[0][-1])
        assert total > 1
        for cap, arrays in itertools.product((0, total - 1, total, total + 5), (ALL, ("ids",), ("col", "perm"))):
            mode = MODES[k % 3]
            k += 1
            got, csr = _filter(e, mode, hdr, sids, rids, row_limit=row_limit, cap=cap, arrays=arrays)
            _same(got, host, (row_limit, cap, arrays, mode))
            assert _check(csr, perm, rids, E.SELECT_LOOKUP, row_limit, cap, (row_limit, cap, arrays, mode)) == total
            assert np.array_equal(csr["row_n"], surv)  # unclipped, while row_off follows the limit
            if row_limit:
                assert (np.diff(csr["row_off"].astype(np.int64)) == np.minimum(surv, row_limit)).all()
    # without row_n
    got, csr = _filter(e, "sync", hdr, sids, rids, row_limit=3, row_n=False)
    _check(csr, perm, rids, E.SELECT_LOOKUP, 3, 5 * 65)
    e.close()


# ---- 4. several bands -----------------------------------------------------------------------------

@pytest.mark.parametrize("workspaces", [0, 1], ids=["two-workspaces", "one-workspace"])
def test_bands(workspaces):
    """max_batch = 256 cuts S x 100 into 2-row tiles: 10 x 100 is five bands, 9 x 100 five with a
    ragged last one; the selection runs once, behind the last band, and row_off ascends across them."""
    fam = _family("nested")
    assert E.cross_tile_device(10, 100, 256) == 2
    e = fam.engine(max_batch=256, workspaces=workspaces)
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    for S in (10, 9):
        sub = [sub_all[(1 + j) % len(sub_all)] for j in range(S)]
        res = [res_all[j % len(res_all)] for j in range(100)]
        hdr, sids, rids = _ids(e, shape, sub, res)
        host, perm = _yard(e, hdr, sids, rids)
        for row_limit, block in ((0, False), (7, False), (0, True)):
            s0 = e.device_compact_stats()
            got, csr = _filter(e, "sync", hdr, sids, rids, row_limit=row_limit, block=block)
            assert e.device_compact_stats() == (s0[0] + 5, s0[1])
            _same(got, host, (S, row_limit, block))
            total = _check(csr, perm, rids, E.SELECT_LOOKUP, row_limit, S * 100, (S, row_limit, block))
            ro = csr["row_off"].astype(np.int64)
            assert (np.diff(ro) >= 0).all() and ro[2] > 0 and ro[-1] == total and ro[-1] > ro[4]  # across bands
        # a submitted request must be one tile
        for mode in MODES[1:]:
            with pytest.raises(E.GckError) as ei:
                _filter(e, mode, hdr, sids, rids)
            assert ei.value.code == E.GCK_E_INVALID_ARGUMENT and "one tile" in ei.value.message
    e.close()


# ---- 5. expanded on the device --------------------------------------------------------------------

def test_expanded_check_contexts():
    """Check contexts force the expansion. Without a slot the caveated grants stay CONDITIONAL: they
    survive SELECT_LOOKUP, and SELECT_CONDITIONAL alone picks exactly those."""
    fam = _family("caveated")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    sub, res = sub[:12], res[:35]
    hdr, sids, rids = _ids(e, shape, sub, res)
    k = 0
    for slot in (0, 1, 2):
        ctx = CTXS[slot - 1] if slot else None
        host, perm = _yard(e, hdr + (slot,), sids, rids, contexts=CTXS)
        assert np.array_equal(perm, fam.want(shape, sub, res, ctx)[0])
        if slot == 0:
            assert (perm == E.PERM_CONDITIONAL).any() and (perm == E.PERM_HAS).any()
        for select in (E.SELECT_LOOKUP, E.SELECT_CONDITIONAL, E.SELECT_HAS):
            s0 = e.device_compact_stats()
            mode = MODES[k % 3]
            k += 1
            got, csr = _filter(e, mode, hdr + (slot,), sids, rids, select=select, contexts=CTXS)
            assert e.device_compact_stats() == (s0[0], s0[1] + 1), "not expanded"
            _same(got, host, (slot, select, mode))
            _check(csr, perm, rids, select, 0, len(sids) * len(rids), (slot, select, mode))
            if select == E.SELECT_CONDITIONAL:
                assert csr["n"] == int((perm == E.PERM_CONDITIONAL).sum())
                assert (csr["perm"] == E.PERM_CONDITIONAL).all()
    e.close()


def test_expanded_long_rows():
    """2 x 2081: R >= GCK_CROSS_IDS, so the request is expanded, and a row is 66 words — the whole
    wave, a full piece of 64 words and a ragged one of 2 with a carried rank."""
    fam = _family("nested")
    e = fam.engine()
    assert E.cross_tile_device(2, 2081) == 0 and 2081 >= E.CROSS_IDS
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    sub = [sub_all[1], sub_all[2]]
    res = [res_all[j % len(res_all)] for j in range(2081)]
    hdr, sids, rids = _ids(e, shape, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    surv = ((E.SELECT_LOOKUP >> perm) & 1)
    assert surv[:, 2048:].any() and surv[:, :2048].any() and surv.sum(axis=1)[0] != surv.sum(axis=1)[1]
    for row_limit, cap in ((0, 2 * 2081), (3, 2 * 2081), (1100, 2 * 2081), (0, 1500)):
        s0 = e.device_compact_stats()
        got, csr = _filter(e, "sync", hdr, sids, rids, row_limit=row_limit, cap=cap)
        assert e.device_compact_stats() == (s0[0], s0[1] + 1), "not expanded"
        _same(got, host, (row_limit, cap))
        _check(csr, perm, rids, E.SELECT_LOOKUP, row_limit, cap, (row_limit, cap))
    e.close()


def test_expanded_chunks_end_inside_rows():
    """max_batch = 64: 1 x 500 runs as eight chunks of 64 checks, 60 x 3 (thin) as three whose
    boundaries fall inside rows and inside plane words; the selection follows the last chunk."""
    fam = _family("nested")
    shape = ("doc", "view", "user", "")
    res_all, sub_all = fam.shapes[shape]
    for workspaces in (0, 1):
        e = fam.engine(max_batch=64, workspaces=workspaces)
        for (S, R), chunks in (((1, 500), 8), ((60, 3), 3)):
            assert E.cross_tile_device(S, R, 64) == 0
            sub = [sub_all[(1 + j) % len(sub_all)] for j in range(S)]
            res = [res_all[(3 * j) % len(res_all)] for j in range(R)]
            hdr, sids, rids = _ids(e, shape, sub, res)
            host, perm = _yard(e, hdr, sids, rids)
            assert ((E.SELECT_LOOKUP >> perm) & 1).any()
            for row_limit in (0, 2):
                s0 = e.device_compact_stats()
                got, csr = _filter(e, "sync", hdr, sids, rids, row_limit=row_limit)
                assert e.device_compact_stats() == (s0[0], s0[1] + chunks), (S, R)  # counted as expanded
                _same(got, host, (S, R))
                _check(csr, perm, rids, E.SELECT_LOOKUP, row_limit, S * R, (S, R, row_limit))
        e.close()


# ---- 6. all errors and empties --------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_all_errors_and_empties(mode):
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 3, 37))
    bad = _bad_permission(e, hdr)
    host, perm = _yard(e, bad, sids, rids)
    assert host[2] == 111 and not perm.any()
    for select in (E.SELECT_LOOKUP, E.SELECT_NO | E.SELECT_LOOKUP):
        got, csr = _filter(e, mode, bad, sids, rids, select=select)
        _same(got, host, mode)
        assert got[2] == 111 and len(got[1]) == 111
        assert csr["n"] == 0 and csr["row_off"].tolist() == [0, 0, 0, 0] and csr["row_n"].tolist() == [0, 0, 0]
        assert len(csr["ids"]) == 0
    # an error-free request after them: the error count is written as 0
    host, perm = _yard(e, hdr, sids, rids)
    got, csr = _filter(e, mode, hdr, sids, rids, err_cap=4)
    assert got[2] == 0 and got[1] == []
    _same(got, host)
    _check(csr, perm, rids, E.SELECT_LOOKUP, 0, 111)
    # S == 0: row_off[0] and the two count words alone; R == 0: S + 1 zero offsets
    s0 = e.device_compact_stats()
    for s, r in ((sids[:0], rids), (sids, rids[:0]), (sids[:0], rids[:0])):
        got, csr = _filter(e, mode, hdr, s, r, cap=4, err_cap=2)
        assert got[2] == 0 and got[1] == [] and csr["n"] == 0
        assert csr["row_off"].tolist() == [0] * (len(s) + 1) and csr["row_n"].tolist() == [0] * len(s)
        assert len(csr["ids"]) == 0 and len(csr["col"]) == 0 and len(csr["perm"]) == 0
    assert e.device_compact_stats() == s0
    e.close()


# ---- 7. refusals before any launch ----------------------------------------------------------------

def test_argument_errors():
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 4, 40))
    ds, dr = _u32(np.concatenate([sids, sids])), _u32(np.concatenate([rids, rids]))
    out, csr = _Out(4, 40, 8), _Csr(4, 16)
    torch.cuda.synchronize()
    good = dict(out.args(), **csr.args())
    s0, b0 = e.device_compact_stats(), e.stats()["batches"]

    def refused(fn, hdr=hdr, S=4, R=40, d_s=ds.data_ptr(), d_r=dr.data_ptr(), **changes):
        with pytest.raises(E.GckError) as ei:
            r = fn(hdr, d_s, S, d_r, R, **dict(good, **changes))
            if hasattr(r, "wait"):
                r.wait()
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        return ei.value.message

    for fn in (e.filter_cross_device, e.submit_filter_cross_device):
        for mask in (0, 1, 3, 15, 16, 0x12):
            assert "mask" in refused(fn, select=mask)
        assert "d_out_row_off" in refused(fn, d_out_row_off=0)
        assert "d_out_n" in refused(fn, d_out_n=0)
        assert "d_out_packed" in refused(fn, d_out_packed=0)
        assert "cap" in refused(fn, d_out_ids=0, d_out_col=0, d_out_perm=0)
        for name in ("d_out_row_off", "d_out_row_n", "d_out_ids", "d_out_col", "d_out_n"):
            assert "aligned" in refused(fn, **{name: good[name] + 2}), name
        # everything the cross device call refuses
        assert "d_out_packed" in refused(fn, d_out_packed=good["d_out_packed"] + 4)
        assert "2^32" in refused(fn, S=65536, R=65536)
        assert "reserved" in refused(fn, hdr=E.Uniform(*hdr[:4], 0, 7))
        assert "d_subjects" in refused(fn, d_s=ds.data_ptr() + 2)
        assert "d_resources" in refused(fn, d_r=dr.data_ptr() + 1)
        refused(fn, d_out_errs=good["d_out_errs"] + 2)
        refused(fn, d_out_n_errs=good["d_out_n_errs"] + 2)
        refused(fn, d_s=0)
        refused(fn, d_r=0)
        refused(fn, d_out_errs=0)
        refused(fn, hdr=hdr + (1,))
    # a null gck_select_rows
    cs, tail = e._device_tail(E.CONSISTENCY_MIN_LATENCY, 0, NOW_US, None, good["d_out_packed"], good["d_out_errs"], 8,
                              good["d_out_n_errs"])
    rev = E.C.c_uint64(0)
    rc = e._lib.gck_filter_cross_device(e._h, E.C.byref(cs), E.C.byref(E._header(hdr)), ds.data_ptr(), 4, dr.data_ptr(),
                                        40, *tail[:4], None, *tail[4:], None, E.C.byref(rev))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    out.untouched(), csr.untouched()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran
    host, perm = _yard(e, hdr, sids, rids)
    got, c = _filter(e, "engine", hdr, sids, rids)
    _same(got, host, "after refusals")
    _check(c, perm, rids, E.SELECT_LOOKUP, 0, 160)
    e.close()


# ---- 8. the torch and client surface --------------------------------------------------------------

def test_filter_cross_ids_and_client():
    fam = _family("gdocs")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    sub, res = sub[:9], res + res[:7]  # (repeated ids are reported as often as the list repeats them)
    hdr, sids, rids = _ids(e, shape, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    assert host[2] == 0 and ((E.SELECT_LOOKUP >> perm) & 1).sum() > 9
    S, R = len(sids), len(rids)
    for dtype, limit in itertools.product((torch.int32, torch.uint32), (0, 2)):
        ts, tr = _u32(sids).view(dtype), _u32(rids).view(dtype)
        row_off, ids, col, pm = e.filter_cross_ids(hdr, ts, tr, row_limit=limit, want_col=True, want_perm=True,
                                                   now_us=NOW_US)
        assert row_off.is_cuda and row_off.dtype == torch.int32 and ids.dtype == dtype and pm.dtype == torch.uint8
        csr = {"row_off": row_off.cpu().numpy().view(np.uint32), "n": int(row_off[-1]), "row_n": None,
               "ids": ids.view(torch.int32).cpu().numpy().view(np.uint32), "col": col.cpu().numpy().view(np.uint32),
               "perm": pm.cpu().numpy()}
        _check(csr, perm, rids, E.SELECT_LOOKUP, limit, S * R, (dtype, limit))
        two = e.filter_cross_ids(hdr, ts, tr, select=E.SELECT_NO, row_limit=limit, now_us=NOW_US)
        assert len(two) == 2
        want = expect(perm, rids, E.SELECT_NO, limit)
        assert np.array_equal(two[0].cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(two[1].view(torch.int32).cpu().numpy().view(np.uint32), want[2])
    empty = e.filter_cross_ids(hdr, _u32(sids), _u32(rids[:0]))
    assert empty[0].tolist() == [0] * (S + 1) and empty[1].numel() == 0
    with pytest.raises(E.GckError):  # a per-item error: raised, as filter_ids raises it
        e.filter_cross_ids(_bad_permission(e, hdr), _u32(sids), _u32(rids))
    with pytest.raises(E.GckError):
        e.filter_cross_ids(hdr, _u32(sids).cpu(), _u32(rids))
    e.close()

    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(1, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jake", "user:joey", "user:jimmy", "user:nobody_of_that_name"]
    resources = ["company:authzed", "company:no_such_company", "company:authzed"]
    rows, err = c.CheckCross(None, cs, "founder", resources, subjects)
    assert err is None and rows[0] == [True, False, True]
    user, company = e.type_id("user"), e.type_id("company")
    sids = _u32(e.intern(user, [s.split(":")[1] for s in subjects]))
    rids = _u32(e.intern(company, [r.split(":")[1] for r in resources]))
    for limit in (0, 1):
        (row_off, ids), err = c.FilterCrossDevice(None, cs, "company#founder", rids, "user", sids, limit=limit)
        assert err is None and ids.is_cuda
        want_off, want_ids = [0], []
        for row in rows:
            kept = [int(rids[r]) for r, ok in enumerate(row) if ok][:limit or None]
            want_ids += kept
            want_off.append(len(want_ids))
        assert row_off.tolist() == want_off and ids.tolist() == want_ids, limit
    # the same refusals and errors as CheckCrossDevice's
    out, err = c.FilterCrossDevice(None, cs, "company#founder", rids.cpu(), "user", sids)
    assert out is None and err is not None
    out, err = c.FilterCrossDevice(None, cs, "company#no_such_permission", rids, "user", sids)
    assert out is None and isinstance(err, E.GckError)
    # a per-item error becomes err: near_budget's checks run out of depth
    e.close()
    fam = _family("near_budget")
    e = fam.engine()
    shape = ("doc", "view", "user", "")
    res, sub = fam.shapes[shape]
    assert fam.want(shape, sub, res)[1]
    hdr, sids, rids = _ids(e, shape, sub, res)
    out, err = Client(e).FilterCrossDevice(None, cs, "doc#view", _u32(rids), "user", _u32(sids))
    assert out is None and isinstance(err, E.GckError)
    e.close()
