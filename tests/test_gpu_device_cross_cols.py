"""Cross filter requests by resource (include/gck.h gck_filter_cross_cols_device and its submit form):
the cross device request with each resource's surviving subjects compacted by kernels into a CSR by
resource in device memory (torch tensors on cuda:0).

Bar, never the code under test: the host cross call's plane on the same request (_yard of
tests/test_gpu_device_cross_filter.py), unpacked, then the numpy selection of tests/test_select_rows.py
(expect) applied to the TRANSPOSED matrix with the subject ids as the source — and, in the family test,
the oracle's answer of every (subject, resource). The plane and the error records must equal the plain
cross device call's bit for bit. Every output starts poisoned — the records with two entries beyond
cap, col_off with an entry beyond R + 1, col_n with one beyond R, the plane with a word beyond it, the
error list and both count words — and whatever the protocol leaves untouched must stay so."""
import itertools

import numpy as np
import pytest
import torch

from gochugaru_amd import consistency
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client, InvalidArgument
from tests.helpers import load_golden
from tests.test_gpu_device_cross import (CTXS, MODES, NOW_US, SENT, _bad_permission, _cross, _dev, _family, _ids,
                                         _nested_lists, _Out, _same, _u32)
from tests.test_gpu_device_cross_filter import _yard
from tests.test_select_rows import expect

pytestmark = pytest.mark.gpu
P8 = 0xA5
ALL = ("ids", "row", "perm")
SHAPE = ("doc", "view", "user", "")


class _Csr:
    """The device CSR outputs of one request, poisoned: R + 2 offsets, R + 1 column counts, cap + 2
    records per array, the count word."""

    def __init__(self, R, cap, arrays=ALL, col_n=True):
        i32 = lambda n: torch.full((n,), SENT, dtype=torch.int32, device=_dev())
        self.R, self.cap, self.arrays = R, cap, arrays
        self.col_off, self.n = i32(R + 2), i32(1)
        self.col_n = i32(R + 1) if col_n else None
        self.ids = i32(cap + 2) if "ids" in arrays else None
        self.row = i32(cap + 2) if "row" in arrays else None
        self.perm = torch.full((cap + 2,), P8, dtype=torch.uint8, device=_dev()) if "perm" in arrays else None

    def args(self):
        p = lambda t: 0 if t is None else t.data_ptr()
        return dict(d_out_col_off=self.col_off.data_ptr(), d_out_n=self.n.data_ptr(), cap=self.cap, d_out_ids=p(self.ids),
                    d_out_row=p(self.row), d_out_perm=p(self.perm), d_out_col_n=p(self.col_n))

    def _np(self, t):
        a = t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def untouched(self):
        torch.cuda.synchronize()
        for t in (self.col_off, self.n, self.col_n, self.ids, self.row):
            assert t is None or (self._np(t) == SENT).all()
        assert self.perm is None or (self._np(self.perm) == P8).all()

    def read(self):
        """{"col_off": R + 1, "col_n": R or None, "n", "ids" / "row" / "perm": the first min(n, cap) or
        None}; the poison beyond each is asserted here."""
        torch.cuda.synchronize()
        R, co, n = self.R, self._np(self.col_off), int(self._np(self.n)[0])
        assert n != SENT, "the count word was not written"
        assert (co[R + 1:] == SENT).all(), "col_off beyond R + 1 was written"
        out = {"col_off": co[:R + 1].copy(), "n": n, "col_n": None}
        if self.col_n is not None:
            cn = self._np(self.col_n)
            assert (cn[R:] == SENT).all(), "col_n beyond R was written"
            out["col_n"] = cn[:R].copy()
        k = min(n, self.cap)
        for name, poison in (("ids", SENT), ("row", SENT), ("perm", P8)):
            t = getattr(self, name)
            out[name] = None
            if t is not None:
                a = self._np(t)
                assert (a[k:] == poison).all(), f"{name} beyond min(total, cap) was written"
                out[name] = a[:k].copy()
        return out


def _filter(e, mode, hdr, sids, rids, select=E.SELECT_LOOKUP, col_limit=0, cap=None, arrays=ALL, col_n=True,
            err_cap=None, count=True, contexts=None, block=False):
    """One cross filter request by resource: ((words, records written, count or None), the CSR read back)."""
    S, R = len(sids), len(rids)
    if block:
        keep, ds, dr = E.cross_id_block(_u32(sids), _u32(rids))
    else:
        ds, dr = _u32(sids), _u32(rids)
    out = _Out(S, R, S * R if err_cap is None else err_cap, count)
    csr = _Csr(R, S * R if cap is None else cap, arrays, col_n)
    kw = dict(out.args(), **csr.args(), select=select, col_limit=col_limit, now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, ds.data_ptr() if S * R else 0, S, dr.data_ptr() if S * R else 0, R)
    if mode == "sync":
        rev = e.filter_cross_cols_device(*head, stream=st, **kw)
    else:
        rev = e.submit_filter_cross_cols_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read(), csr.read()


def _expect(perm, sids, select, col_limit):
    """The expected CSR by resource: the numpy row selection over the transposed matrix."""
    return expect(np.ascontiguousarray(perm.T), np.asarray(sids, dtype=np.uint32), select, col_limit)


def _check(csr, perm, sids, select, col_limit, cap, what=None):
    """The CSR read back against the numpy selection over the yardstick's perm[S, R], transposed."""
    col_off, col_n, ids, row, pm = _expect(perm, sids, select, col_limit)
    total = int(col_off[-1])
    assert csr["n"] == total, (what, csr["n"], total)
    assert np.array_equal(csr["col_off"], col_off), (what, csr["col_off"][:8], col_off[:8])
    if csr["col_n"] is not None:
        assert np.array_equal(csr["col_n"], col_n), (what, csr["col_n"][:8], col_n[:8])  # unclipped
    k = min(total, cap)
    for name, full in (("ids", ids), ("row", row), ("perm", pm)):
        if csr[name] is not None:
            assert len(csr[name]) == k and np.array_equal(csr[name], full[:k]), (what, name, csr[name][:8], full[:8])
    return total


def edge_lists(fam, S, R, first=30):
    """The lists of the mapping tests: nested's subjects from the 31st on and its resources from the
    second on, each repeated in a cycle — so that the first subject and the 65th (the 15th of the
    family) both see the first resource, and rows 0 .. 4 differ (asserted where it matters). first = 28
    puts subjects that see much into rows 0, 2, 8 and 9 (the bands test)."""
    res_all, sub_all = fam.shapes[SHAPE]
    return ([sub_all[(first + j) % len(sub_all)] for j in range(S)], [res_all[(1 + j) % len(res_all)] for j in range(R)])


# ---- 1. every family, against the host call, the cross device call and the oracle -----------------

@pytest.mark.parametrize("family", ["nested", "gdocs", "caveated", "near_budget"])
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    n_records = n_cols_looked_up = 0
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
                _check(csr, perm, sids, select, 0, S * R, (family, shape, mode, select))
                for idx, _ in got[1]:  # no errored check is in any column's records
                    s, r = divmod(idx, R)
                    assert s not in csr["row"][csr["col_off"][r]:csr["col_off"][r + 1]].tolist(), (family, shape, idx)
            n_records += len(plain[1])
        # one column per request: its ids are lookup_subjects_among's over the same candidates
        got, csr = _filter(e, MODES[j % 3], hdr, sids, rids[:1])
        try:
            want_ids, want_perm = e.lookup_subjects_among(hdr[0], int(rids[0]), hdr[1], hdr[2], sids,
                                                          subject_relation=hdr[3], now_us=NOW_US)
        except E.GckError:  # (a per-item error fails that call)
            assert got[2] > 0
        else:
            assert np.array_equal(csr["ids"], want_ids) and np.array_equal(csr["perm"], want_perm), (family, shape)
            assert csr["col_off"].tolist() == [0, len(want_ids)]
            n_cols_looked_up += 1
    print(family, "error records", n_records, "columns compared with lookup_subjects_among", n_cols_looked_up)
    if family == "near_budget":
        assert n_records > 0, "near_budget gave no error record"
    else:
        assert n_cols_looked_up > 0
    e.close()


# ---- 2. the thread mapping: column blocks, row chunks, the block layout ---------------------------

def test_lane_mapping_edges():
    """R = 1 .. 200: a column block of one lane, of half a wave on both sides, of a wave and one lane,
    four blocks; S = 1 .. 130: chunks of one row with idle waves, of 4, 5 and 9 rows (more than a batch
    of 8 words) and a ragged last chunk. All one-tile requests, in place."""
    fam = _family("nested")
    e = fam.engine()
    k = 0
    partial = differ = deep = False
    for R in (1, 31, 32, 33, 65, 200):
        for S in (1, 5, 9, 63, 64, 65, 130):
            assert E.cross_tile_device(S, R) == S  # one tile at the default max_batch
            sub, res = edge_lists(fam, S, R)
            hdr, sids, rids = _ids(e, SHAPE, sub, res)
            host, perm = _yard(e, hdr, sids, rids)
            assert np.array_equal(perm, fam.want(SHAPE, sub, res)[0])
            lives = ((E.SELECT_LOOKUP >> perm) & 1).astype(bool)
            surv = lives.sum(axis=0)
            if S >= 5 and R >= 31:  # the yardstick is not degenerate: a column partly kept, columns that differ
                assert ((surv > 0) & (surv < S)).any(), (S, R, surv)
                assert len(set(surv.tolist())) > 1, (S, R, surv)
                partial = differ = True
            if S >= 65:
                assert lives[64:].any(), (S, R)  # a survivor in a row >= 64
                deep = True
            for block in (False, True):
                mode = MODES[k % 3]
                k += 1
                select = (E.SELECT_LOOKUP, E.SELECT_NO, E.SELECT_HAS | E.SELECT_NO)[k % 3]
                got, csr = _filter(e, mode, hdr, sids, rids, select=select, block=block)
                _same(got, host, (S, R, mode, block))
                _check(csr, perm, sids, select, 0, S * R, (S, R, mode, block, select))
    assert partial and differ and deep
    assert e.device_compact_stats() == (k, 0)  # every request ran in place
    e.close()


# ---- 3. col_limit and cap -------------------------------------------------------------------------

def test_col_limit_and_cap():
    fam = _family("nested")
    e = fam.engine()
    sub, res = edge_lists(fam, 65, 5)
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    surv = ((E.SELECT_LOOKUP >> perm) & 1).sum(axis=0)
    assert surv.max() > 3 and len(set(surv.tolist())) > 1, surv  # a limit of 3 clips some column
    k = 0
    for col_limit in (0, 1, 3, 65):
        total = int(_expect(perm, sids, E.SELECT_LOOKUP, col_limit)[0][-1])
        assert total > 1
        for cap, arrays, col_n in itertools.product((0, total - 1, total, total + 5), (ALL, ("ids",), ("row", "perm")),
                                                    (True, False)):
            mode = MODES[k % 3]
            k += 1
            got, csr = _filter(e, mode, hdr, sids, rids, col_limit=col_limit, cap=cap, arrays=arrays, col_n=col_n)
            what = (col_limit, cap, arrays, col_n, mode)
            _same(got, host, what)
            assert _check(csr, perm, sids, E.SELECT_LOOKUP, col_limit, cap, what) == total
            if col_n:
                assert np.array_equal(csr["col_n"], surv)  # unclipped, while col_off follows the limit
            if col_limit:
                assert (np.diff(csr["col_off"].astype(np.int64)) == np.minimum(surv, col_limit)).all()
    e.close()


# ---- 4. several bands -----------------------------------------------------------------------------

@pytest.mark.parametrize("workspaces", [0, 1], ids=["two-workspaces", "one-workspace"])
def test_bands(workspaces):
    """max_batch = 256 cuts S x 100 into 2-row tiles: 10 x 100 is five bands, 9 x 100 five with a
    ragged last one; the selection runs once, behind the last band, and a column's survivors span the
    bands with ascending rows."""
    fam = _family("nested")
    assert E.cross_tile_device(10, 100, 256) == 2
    e = fam.engine(max_batch=256, workspaces=workspaces)
    for S in (10, 9):
        sub, res = edge_lists(fam, S, 100, first=28)
        hdr, sids, rids = _ids(e, SHAPE, sub, res)
        host, perm = _yard(e, hdr, sids, rids)
        lives = ((E.SELECT_LOOKUP >> perm) & 1).astype(bool)
        assert (lives[:2].any(axis=0) & lives[8:].any(axis=0)).any()  # a column with survivors in the first and the last band
        for col_limit, block in ((0, False), (4, False), (0, True)):
            s0 = e.device_compact_stats()
            got, csr = _filter(e, "sync", hdr, sids, rids, col_limit=col_limit, block=block)
            assert e.device_compact_stats() == (s0[0] + 5, s0[1])
            _same(got, host, (S, col_limit, block))
            total = _check(csr, perm, sids, E.SELECT_LOOKUP, col_limit, S * 100, (S, col_limit, block))
            co = csr["col_off"].astype(np.int64)
            assert (np.diff(co) >= 0).all() and co[-1] == total
            spans = 0
            for r in range(100):  # ranks ascend with the row, across the bands
                rows = csr["row"][co[r]:co[r + 1]].astype(np.int64)
                assert (np.diff(rows) > 0).all(), (S, r, rows)
                spans += len(rows) > 1 and rows[0] < 2 and rows[-1] >= 2
            assert spans > 0
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
    res, sub = fam.shapes[SHAPE]
    sub, res = sub[:12], res[:35]
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    k = 0
    for slot in (0, 1, 2):
        ctx = CTXS[slot - 1] if slot else None
        host, perm = _yard(e, hdr + (slot,), sids, rids, contexts=CTXS)
        assert np.array_equal(perm, fam.want(SHAPE, sub, res, ctx)[0])
        if slot == 0:
            assert (perm == E.PERM_CONDITIONAL).any() and (perm == E.PERM_HAS).any()
        for select in (E.SELECT_LOOKUP, E.SELECT_CONDITIONAL, E.SELECT_HAS):
            s0 = e.device_compact_stats()
            mode = MODES[k % 3]
            k += 1
            got, csr = _filter(e, mode, hdr + (slot,), sids, rids, select=select, contexts=CTXS)
            assert e.device_compact_stats() == (s0[0], s0[1] + 1), "not expanded"
            _same(got, host, (slot, select, mode))
            _check(csr, perm, sids, select, 0, len(sids) * len(rids), (slot, select, mode))
            if select == E.SELECT_CONDITIONAL:
                assert csr["n"] == int((perm == E.PERM_CONDITIONAL).sum())
                assert (csr["perm"] == E.PERM_CONDITIONAL).all()
    e.close()


@pytest.mark.parametrize("S", [2, 70])
def test_expanded_wide_planes(S):
    """S x 2081: R >= GCK_CROSS_IDS, so the request is expanded; the plane is 66 words wide — 33 column
    blocks, the last of 33 columns, the last word of a row with one column and 31 of padding."""
    fam = _family("nested")
    e = fam.engine()
    assert E.cross_tile_device(S, 2081) == 0 and 2081 >= E.CROSS_IDS
    sub, res = edge_lists(fam, S, 2081)
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    surv = ((E.SELECT_LOOKUP >> perm) & 1).sum(axis=0)
    assert surv[2048:].any() and surv[:2048].any() and len(set(surv.tolist())) > 1
    chunks = -(-S * 2081 // 65536)
    for col_limit, cap in ((0, S * 2081), (1, S * 2081), (0, 1500)):
        s0 = e.device_compact_stats()
        got, csr = _filter(e, "sync", hdr, sids, rids, col_limit=col_limit, cap=cap)
        assert e.device_compact_stats() == (s0[0], s0[1] + chunks), "not expanded"
        _same(got, host, (col_limit, cap))
        _check(csr, perm, sids, E.SELECT_LOOKUP, col_limit, cap, (col_limit, cap))
    e.close()


@pytest.mark.parametrize("S,R,in_place", [(2100, 3, False), (2052, 40, True), (4100, 33, True)])
def test_more_rows_than_a_tile(S, R, in_place):
    """The selection kernels take the rows in tiles of 2,048: a thin expanded request of 2,100 rows, and
    in-place requests of several bands whose finished plane is two tiles and four rows, and three tiles —
    a column's rank is carried from tile to tile."""
    fam = _family("nested")
    e = fam.engine()
    assert (E.cross_tile_device(S, R) != 0) == in_place and E.cross_tile_device(S, R) < S
    sub, res = edge_lists(fam, S, R)
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    lives = ((E.SELECT_LOOKUP >> perm) & 1).astype(bool)
    assert (lives[:2048].any(axis=0) & lives[2048:].any(axis=0)).any()  # a column with survivors in two tiles
    for col_limit, cap in ((0, S * R), (S // 3, S * R), (0, 1000)):
        s0 = e.device_compact_stats()
        got, csr = _filter(e, "sync", hdr, sids, rids, col_limit=col_limit, cap=cap, err_cap=8)
        s1 = e.device_compact_stats()
        assert (s1[0] > s0[0] and s1[1] == s0[1]) if in_place else (s1[0] == s0[0] and s1[1] > s0[1])
        _same(got, host, (col_limit, cap))
        _check(csr, perm, sids, E.SELECT_LOOKUP, col_limit, cap, (col_limit, cap))
    e.close()


def test_expanded_chunks_end_inside_rows():
    """max_batch = 64: 1 x 500 runs as eight chunks of 64 checks, 130 x 3 (thin) as seven whose
    boundaries fall inside rows and inside plane words; the selection follows the last chunk."""
    fam = _family("nested")
    res_all, sub_all = fam.shapes[SHAPE]
    for workspaces in (0, 1):
        e = fam.engine(max_batch=64, workspaces=workspaces)
        for (S, R), chunks in (((1, 500), 8), ((130, 3), 7)):
            assert E.cross_tile_device(S, R, 64) == 0
            sub = [sub_all[(1 + j) % len(sub_all)] for j in range(S)]
            res = [res_all[(3 * j) % len(res_all)] for j in range(R)]
            hdr, sids, rids = _ids(e, SHAPE, sub, res)
            host, perm = _yard(e, hdr, sids, rids)
            assert ((E.SELECT_LOOKUP >> perm) & 1).any()
            for col_limit in (0, 2):
                s0 = e.device_compact_stats()
                got, csr = _filter(e, "sync", hdr, sids, rids, col_limit=col_limit)
                assert e.device_compact_stats() == (s0[0], s0[1] + chunks), (S, R)  # counted as expanded
                _same(got, host, (S, R))
                _check(csr, perm, sids, E.SELECT_LOOKUP, col_limit, S * R, (S, R, col_limit))
        e.close()


# ---- 6. all errors and empties --------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_all_errors_and_empties(mode):
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 37, 3))
    bad = _bad_permission(e, hdr)
    host, perm = _yard(e, bad, sids, rids)
    assert host[2] == 111 and not perm.any()
    for select in (E.SELECT_LOOKUP, E.SELECT_NO | E.SELECT_LOOKUP):
        got, csr = _filter(e, mode, bad, sids, rids, select=select)
        _same(got, host, mode)
        assert got[2] == 111 and len(got[1]) == 111
        assert csr["n"] == 0 and csr["col_off"].tolist() == [0, 0, 0, 0] and csr["col_n"].tolist() == [0, 0, 0]
        assert len(csr["ids"]) == 0
    # an error-free request after them: the error count is written as 0
    host, perm = _yard(e, hdr, sids, rids)
    got, csr = _filter(e, mode, hdr, sids, rids, err_cap=4)
    assert got[2] == 0 and got[1] == []
    _same(got, host)
    _check(csr, perm, sids, E.SELECT_LOOKUP, 0, 111)
    # R == 0: col_off[0] and the two count words alone; S == 0: R + 1 zero offsets and R zero counts
    s0 = e.device_compact_stats()
    for s, r in ((sids[:0], rids), (sids, rids[:0]), (sids[:0], rids[:0])):
        got, csr = _filter(e, mode, hdr, s, r, cap=4, err_cap=2)
        assert got[2] == 0 and got[1] == [] and csr["n"] == 0
        assert csr["col_off"].tolist() == [0] * (len(r) + 1) and csr["col_n"].tolist() == [0] * len(r)
        assert len(csr["ids"]) == 0 and len(csr["row"]) == 0 and len(csr["perm"]) == 0
    assert e.device_compact_stats() == s0
    e.close()


# ---- 7. refusals before any launch ----------------------------------------------------------------

def test_argument_errors():
    fam = _family("nested")
    e = fam.engine()
    hdr, sids, rids = _ids(e, *_nested_lists(fam, 4, 40))
    ds, dr = _u32(np.concatenate([sids, sids])), _u32(np.concatenate([rids, rids]))
    out, csr = _Out(4, 40, 8), _Csr(40, 16)
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

    for fn in (e.filter_cross_cols_device, e.submit_filter_cross_cols_device):
        for mask in (0, 1, 3, 15, 16, 0x12):
            assert "mask" in refused(fn, select=mask)
        assert "d_out_col_off" in refused(fn, d_out_col_off=0)
        assert "d_out_n" in refused(fn, d_out_n=0)
        assert "d_out_packed" in refused(fn, d_out_packed=0)
        assert "cap" in refused(fn, d_out_ids=0, d_out_row=0, d_out_perm=0)
        for name in ("d_out_col_off", "d_out_col_n", "d_out_ids", "d_out_row", "d_out_n"):
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
    # a null gck_select_cols
    cs, tail = e._device_tail(E.CONSISTENCY_MIN_LATENCY, 0, NOW_US, None, good["d_out_packed"], good["d_out_errs"], 8,
                              good["d_out_n_errs"])
    rev = E.C.c_uint64(0)
    rc = e._lib.gck_filter_cross_cols_device(e._h, E.C.byref(cs), E.C.byref(E._header(hdr)), ds.data_ptr(), 4,
                                             dr.data_ptr(), 40, *tail[:4], None, *tail[4:], None, E.C.byref(rev))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    out.untouched(), csr.untouched()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran
    host, perm = _yard(e, hdr, sids, rids)
    got, c = _filter(e, "engine", hdr, sids, rids)
    _same(got, host, "after refusals")
    _check(c, perm, sids, E.SELECT_LOOKUP, 0, 160)
    e.close()


# ---- 8. the torch and client surface --------------------------------------------------------------

def test_filter_cross_cols_ids_and_client():
    fam = _family("gdocs")
    e = fam.engine()
    res, sub = fam.shapes[SHAPE]
    sub, res = (sub + sub[:7])[:40], res[:9]  # (repeated ids are reported as often as the list repeats them)
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    host, perm = _yard(e, hdr, sids, rids)
    assert host[2] == 0 and ((E.SELECT_LOOKUP >> perm) & 1).sum() > 9
    S, R = len(sids), len(rids)
    for dtype, limit in itertools.product((torch.int32, torch.uint32), (0, 2)):
        ts, tr = _u32(sids).view(dtype), _u32(rids).view(dtype)
        col_off, ids, row, pm = e.filter_cross_cols_ids(hdr, ts, tr, col_limit=limit, want_row=True, want_perm=True,
                                                        now_us=NOW_US)
        assert col_off.is_cuda and col_off.dtype == torch.int32 and ids.dtype == dtype and pm.dtype == torch.uint8
        csr = {"col_off": col_off.cpu().numpy().view(np.uint32), "n": int(col_off[-1]), "col_n": None,
               "ids": ids.view(torch.int32).cpu().numpy().view(np.uint32), "row": row.cpu().numpy().view(np.uint32),
               "perm": pm.cpu().numpy()}
        _check(csr, perm, sids, E.SELECT_LOOKUP, limit, S * R, (dtype, limit))
        two = e.filter_cross_cols_ids(hdr, ts, tr, select=E.SELECT_NO, col_limit=limit, now_us=NOW_US)
        assert len(two) == 2
        want = _expect(perm, sids, E.SELECT_NO, limit)
        assert np.array_equal(two[0].cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(two[1].view(torch.int32).cpu().numpy().view(np.uint32), want[2])
    empty = e.filter_cross_cols_ids(hdr, _u32(sids[:0]), _u32(rids))
    assert empty[0].tolist() == [0] * (R + 1) and empty[1].numel() == 0
    with pytest.raises(E.GckError):  # a per-item error: raised, as filter_cross_ids raises it
        e.filter_cross_cols_ids(_bad_permission(e, hdr), _u32(sids), _u32(rids))
    with pytest.raises(E.GckError):
        e.filter_cross_cols_ids(hdr, _u32(sids).cpu(), _u32(rids))
    with pytest.raises(E.GckError):
        e.filter_cross_cols_ids(hdr, sids.tolist(), _u32(rids))
    e.close()

    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(1, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jake", "user:joey", "user:nobody_of_that_name", "user:jimmy", "user:jake"]
    resources = ["company:authzed", "company:no_such_company", "company:authzed"]
    user, company = e.type_id("user"), e.type_id("company")
    sids = _u32(e.intern(user, [s.split(":")[1] for s in subjects]))
    rids = _u32(e.intern(company, [r.split(":")[1] for r in resources]))
    # each resource's ids: Client.FilterSubjects over the same candidates
    want = []
    for r in resources:
        names = []
        for name, err in c.FilterSubjects(None, cs, r, "founder", subjects):
            assert err is None
            names.append(name)
        want.append([int(x) for x in e.intern(user, names)])
    assert len(want[0]) == 4 and want[1] == []
    for limit in (0, 1, 3):
        (col_off, ids), err = c.FilterCrossSubjectsDevice(None, cs, "company#founder", rids, "user", sids, limit=limit)
        assert err is None and ids.is_cuda and col_off.is_cuda
        want_off, want_ids = [0], []
        for col in want:
            want_ids += col[:limit or None]  # `limit` clips
            want_off.append(len(want_ids))
        assert col_off.tolist() == want_off and ids.tolist() == want_ids, limit
    # a non-tensor argument is InvalidArgument; the other refusals and errors are FilterCrossDevice's
    for bad_r, bad_s in ((rids.tolist(), sids), (rids, sids.tolist()), (rids.cpu(), sids)):
        out, err = c.FilterCrossSubjectsDevice(None, cs, "company#founder", bad_r, "user", bad_s)
        assert out is None and isinstance(err, InvalidArgument)
    out, err = c.FilterCrossSubjectsDevice(None, cs, "company#founder", rids, "user", sids, limit=-1)
    assert out is None and isinstance(err, InvalidArgument)
    out, err = c.FilterCrossSubjectsDevice(None, cs, "company#no_such_permission", rids, "user", sids)
    assert out is None and isinstance(err, E.GckError)
    # a per-item error becomes err: near_budget's checks run out of depth
    e.close()
    fam = _family("near_budget")
    e = fam.engine()
    res, sub = fam.shapes[SHAPE]
    assert fam.want(SHAPE, sub, res)[1]
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    out, err = Client(e).FilterCrossSubjectsDevice(None, cs, "doc#view", _u32(rids), "user", _u32(sids))
    assert out is None and isinstance(err, E.GckError)
    e.close()
