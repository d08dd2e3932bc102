"""Group filter requests (include/gck.h gck_filter_groups_device and its submit form): S owners, a CSR
of candidates per owner, and each owner's survivors compacted by kernels into a CSR — all in device
memory (torch tensors on cuda:0).

Bar, never the code under test: the host uniform call (check_uniform) on the same pairs built with
numpy, unpacked, then the numpy per-group selection (tests/test_select_groups.py expect) — and, in the
family test, the oracle's answer of every pair. The plane and the error records must equal the uniform
device call's on the same pairs bit for bit. Every output starts poisoned with two entries beyond its
end — the records beyond cap, row_off beyond S + 1, row_n beyond S, the plane beyond its words, the
error list beyond err_cap — and both count words; whatever the protocol leaves untouched must stay so."""
import itertools

import numpy as np
import pytest
import torch

from gochugaru_amd import consistency
from gochugaru_amd import engine as E
from gochugaru_amd.client import Client
from tests.helpers import load_golden
from tests.test_gpu_device_cross import MODES, NOW_US, POISON, SENT, _bad_permission, _dev, _family, _ids, _Out, _records, _u32
from tests.test_gpu_device_cross_filter import P8
from tests.test_select_groups import expect, offsets

pytestmark = pytest.mark.gpu
ALL = ("ids", "pos", "perm")
VARIES = (E.VARY_RESOURCE, E.VARY_SUBJECT)
FAMILIES = ["nested", "gdocs", "caveated", "near_budget"]
SHAPE = ("doc", "view", "user", "")


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


class _Plane(_Out):
    """_Out over a dense plane of n checks, with a second guard word beyond it."""

    def __init__(self, n, cap, count=True):
        super().__init__(1, n, cap, count)
        self.words = torch.full((self.nw + 2,), -1, dtype=torch.int64, device=_dev())

    def guards(self):
        """The two entries beyond the plane and beyond the error list are still poison."""
        torch.cuda.synchronize()
        assert (self.words.cpu().numpy().view(np.uint64)[self.nw:] == POISON).all(), "words beyond the plane were written"
        assert (self.errs.cpu().numpy()[self.cap:] == SENT).all(), "records beyond err_cap were written"

    def read(self):
        self.guards()
        return super().read()


class _Csr:
    """The device CSR outputs of one request, poisoned: S + 3 offsets, S + 2 group counts, cap + 2
    records per array, the count word."""

    def __init__(self, S, cap, arrays=ALL, row_n=True):
        i32 = lambda n: torch.full((n,), SENT, dtype=torch.int32, device=_dev())
        self.S, self.cap = S, cap
        self.row_off, self.n = i32(S + 3), i32(1)
        self.row_n = i32(S + 2) if row_n else None
        self.ids = i32(cap + 2) if "ids" in arrays else None
        self.pos = i32(cap + 2) if "pos" in arrays else None
        self.perm = torch.full((cap + 2,), P8, dtype=torch.uint8, device=_dev()) if "perm" in arrays else None

    def args(self):
        p = lambda t: 0 if t is None else t.data_ptr()
        return dict(d_out_row_off=self.row_off.data_ptr(), d_out_n=self.n.data_ptr(), cap=self.cap, d_out_ids=p(self.ids),
                    d_out_pos=p(self.pos), d_out_perm=p(self.perm), d_out_row_n=p(self.row_n))

    def guards(self):
        """The two entries beyond every array are still poison."""
        torch.cuda.synchronize()
        assert (_np(self.row_off)[self.S + 1:] == SENT).all(), "row_off beyond S + 1 was written"
        assert self.row_n is None or (_np(self.row_n)[self.S:] == SENT).all(), "row_n beyond S was written"
        for t, poison in ((self.ids, SENT), (self.pos, SENT), (self.perm, P8)):
            assert t is None or (_np(t)[self.cap:] == poison).all(), "records beyond cap were written"

    def untouched(self):
        torch.cuda.synchronize()
        for t in (self.row_off, self.n, self.row_n, self.ids, self.pos):
            assert t is None or (_np(t) == SENT).all()
        assert self.perm is None or (_np(self.perm) == P8).all()

    def read(self):
        """{"row_off": S + 1, "row_n": S or None, "n", "ids" / "pos" / "perm": the first min(n, cap) or
        None}; the poison beyond each is asserted here."""
        self.guards()
        S, n = self.S, int(_np(self.n)[0])
        assert n != SENT, "the count word was not written"
        out = {"row_off": _np(self.row_off)[:S + 1].copy(), "n": n,
               "row_n": None if self.row_n is None else _np(self.row_n)[:S].copy()}
        k = min(n, self.cap)
        for name, poison in (("ids", SENT), ("pos", SENT), ("perm", P8)):
            t = getattr(self, name)
            out[name] = None
            if t is not None:
                a = _np(t)
                assert (a[k:] == poison).all(), f"{name} beyond min(total, cap) was written"
                out[name] = a[:k].copy()
        return out


def _pairs(vary, owners, off, cands):
    """The request's checks as (resource id, subject id) pairs, built with numpy."""
    own = np.repeat(np.asarray(owners, dtype=np.uint32), np.diff(off.astype(np.int64)))
    cands = np.asarray(cands, dtype=np.uint32)
    return np.stack([cands, own] if vary == E.VARY_RESOURCE else [own, cands], axis=1).astype(np.uint32)


def _yard(e, hdr, vary, owners, off, cands, contexts=None):
    """The host uniform call on the request's pairs: ((words, records, count), perm[n] with 0 for an error)."""
    n = len(cands)
    if n == 0:
        return (np.zeros(0, dtype=np.uint64), [], 0), np.zeros(0, dtype=np.uint8)
    words, errs, _ = e.check_uniform(hdr, _pairs(vary, owners, off, cands), now_us=NOW_US, contexts=contexts)
    rec = _records(errs)
    words = np.asarray(words).copy()
    return (words, rec, len(rec)), E.unpack_results(words, n)


def _uniform_device(e, hdr, vary, owners, off, cands, contexts=None):
    """gck_check_bulk_uniform_device on the same pairs: (words, records, count)."""
    n = len(cands)
    dp = _u32(_pairs(vary, owners, off, cands))
    out = _Plane(n, n)
    torch.cuda.synchronize()
    e.check_uniform_device(hdr, dp.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream, now_us=NOW_US,
                           contexts=contexts, **out.args())
    return out.read()


def _filter(e, mode, hdr, vary, owners, off, cands, select=E.SELECT_LOOKUP, group_limit=0, cap=None, arrays=ALL,
            row_n=True, err_cap=None, contexts=None, outs=None):
    """One group filter request: ((words, records written, count), the CSR read back). outs: a list that
    receives the two output holders before the call (what a failing call leaves is read from them)."""
    S, n = len(owners), len(cands)
    do, dg, dc = _u32(owners), _u32(off), _u32(cands)
    out = _Plane(n, n if err_cap is None else err_cap)
    csr = _Csr(S, n if cap is None else cap, arrays, row_n)
    if outs is not None:
        outs[:] = [out, csr]
    kw = dict(out.args(), **csr.args(), vary=vary, select=select, group_limit=group_limit, now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    head = (hdr, do.data_ptr() if n else 0, S, dg.data_ptr() if n else 0, dc.data_ptr() if n else 0, n)
    if mode == "sync":
        rev = e.filter_groups_device(*head, stream=st, **kw)
    else:
        rev = e.submit_filter_groups_device(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read(), csr.read()


def _same(got, want, what=None):
    """Device results against the yardstick's: words bit for bit, the records written, the count."""
    gw, gr, gc = got
    ww, wr, wc = want
    assert np.array_equal(gw, ww), (what, [(k, hex(int(a)), hex(int(b))) for k, (a, b) in enumerate(zip(gw, ww)) if a != b][:4])
    assert gr == wr[:len(gr)] and gr == sorted(gr), (what, gr[:6], wr[:6])
    assert gc == wc and len(gr) <= gc, (what, gc, wc)


def _check(csr, perm, off, cands, select, group_limit, cap, what=None):
    """The CSR read back against the numpy selection over the yardstick's perm[n]."""
    row_off, row_n, ids, pos, pm = expect(perm, off, np.asarray(cands, dtype=np.uint32), select, group_limit)
    total = int(row_off[-1])
    assert csr["n"] == total, (what, csr["n"], total)
    assert np.array_equal(csr["row_off"], row_off), (what, csr["row_off"][:8], row_off[:8])
    if csr["row_n"] is not None:
        assert np.array_equal(csr["row_n"], row_n), (what, csr["row_n"][:8], row_n[:8])  # unclipped
    k = min(total, cap)
    for name, full in (("ids", ids), ("pos", pos), ("perm", pm)):
        if csr[name] is not None:
            assert len(csr[name]) == k and np.array_equal(csr[name], full[:k]), (what, name, csr[name][:8], full[:8])
    return total


def _ragged(n_owners, n_pool, seed):
    """Group lengths and, per group, indices into a pool of n_pool candidates: a rotating window whose
    length cycles through 0 .. n_pool, so that every owner meets most of the pool across its groups."""
    rng = np.random.default_rng(seed)
    lengths = [int(x) for x in rng.integers(0, n_pool + 1, n_owners)]
    lengths[0] = n_pool  # (one group holds the whole pool)
    idx = [np.arange(s, s + m) % n_pool for s, m in enumerate(lengths)]
    return lengths, (np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64))


def _family_request(fam, shape, vary):
    """A request over one shape's id lists: owners, group lengths, the candidates' names, and the
    oracle's answer of every check (perm[n] with 0 for an error, [(k, code)])."""
    res, sub = fam.shapes[shape]
    own, pool = (sub, res) if vary == E.VARY_RESOURCE else (res, sub)
    lengths, idx = _ragged(len(own), len(pool), len(own) * 131 + len(pool))
    wp, _ = fam.want(shape, sub, res)
    codes = dict(fam.want(shape, sub, res)[1])
    owner_of = np.repeat(np.arange(len(own)), lengths)
    perm = np.zeros(len(idx), dtype=np.uint8)
    errs = []
    for k, (o, c) in enumerate(zip(owner_of, idx)):
        s, r = (o, c) if vary == E.VARY_RESOURCE else (c, o)
        if s * len(res) + r in codes:
            errs.append((k, codes[s * len(res) + r]))
        else:
            perm[k] = wp[s, r]
    return own, lengths, [pool[i] for i in idx], perm, errs


# ---- 1. every family, against the host call, the uniform device call and the oracle ---------------

@pytest.mark.parametrize("family", FAMILIES)
def test_family_groups_hold_survivors_and_non_survivors(family):
    """The oracle alone: over a family's requests some check survives SELECT_LOOKUP and some does not
    (what test_family_parity then demands of the engine is not a degenerate answer)."""
    fam = _family(family)
    surv = lost = 0
    for shape, vary in itertools.product(fam.shapes, VARIES):
        _, lengths, _, perm, errs = _family_request(fam, shape, vary)
        assert sum(lengths) == len(perm) > 0
        keep = (E.SELECT_LOOKUP >> perm.astype(np.uint32)) & 1
        surv += int(keep.sum())
        lost += int(len(keep) - keep.sum())
    assert surv > 0 and lost > 0, (family, surv, lost)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    n_records = surv = lost = 0
    for j, (shape, vary) in enumerate(itertools.product(fam.shapes, VARIES)):
        own, lengths, cand_names, wp, we = _family_request(fam, shape, vary)
        res, sub = (cand_names, own) if vary == E.VARY_RESOURCE else (own, cand_names)
        hdr, sids, rids = _ids(e, shape, sub, res)
        owners, cands = (sids, rids) if vary == E.VARY_RESOURCE else (rids, sids)
        off = offsets(lengths)
        n = len(cands)
        host, perm = _yard(e, hdr, vary, owners, off, cands)
        assert np.array_equal(perm, wp) and host[1] == we, (family, shape, vary)  # the yardstick itself
        keep = (E.SELECT_LOOKUP >> perm.astype(np.uint32)) & 1
        surv, lost = surv + int(keep.sum()), lost + int(n - keep.sum())
        plain = _uniform_device(e, hdr, vary, owners, off, cands)
        _same(plain, host, (family, shape, vary, "uniform device"))
        for mode in (MODES if j < 2 else [MODES[j % 3]]):
            for select in (E.SELECT_LOOKUP, E.SELECT_NO):
                got, csr = _filter(e, mode, hdr, vary, owners, off, cands, select=select)
                # the plane and the error records: the uniform device call's, bit for bit
                assert np.array_equal(got[0], plain[0]) and got[1] == plain[1] and got[2] == plain[2]
                _same(got, host, (family, shape, vary, mode))
                _check(csr, perm, off, cands, select, 0, n, (family, shape, vary, mode, select))
                bad = {k for k, _ in got[1]}
                assert not bad & set(csr["pos"].tolist()), (family, shape, vary)  # no errored check survives
        n_records += len(plain[1])
    print(family, "survivors", surv, "non-survivors", lost, "error records", n_records)
    assert surv > 0 and lost > 0
    if family == "near_budget":
        assert n_records > 0, "near_budget gave no error record"
    e.close()


# ---- 2. the shapes that can break the kernels -----------------------------------------------------

def _nested_request(fam, e, lengths, vary=E.VARY_RESOURCE):
    """Owners and candidates of nested's doc#view@user shape, names repeated in a cycle (ids are not
    deduplicated); the first subject of the family sees nothing, so the owners begin at the second."""
    res_all, sub_all = fam.shapes[SHAPE]
    own_all, pool = (sub_all, res_all) if vary == E.VARY_RESOURCE else (res_all, sub_all)
    own = [own_all[(1 + j) % len(own_all)] for j in range(len(lengths))]
    cand = [pool[(3 * k + k // 7) % len(pool)] for k in range(sum(lengths))]
    res, sub = (cand, own) if vary == E.VARY_RESOURCE else (own, cand)
    hdr, sids, rids = _ids(e, SHAPE, sub, res)
    owners, cands = (sids, rids) if vary == E.VARY_RESOURCE else (rids, sids)
    return hdr, owners, offsets(lengths), cands


KERNEL_SHAPES = {
    "around_a_word": [0, 1, 31, 32, 33, 0, 0, 65, 130],
    "S257_of_1_to_3": [1 + k % 3 for k in range(257)],
    "one_long_among_short": [3, 1, 2, 2100, 2, 0, 5],
}


@pytest.mark.parametrize("name", list(KERNEL_SHAPES))
def test_shapes(name):
    fam = _family("nested")
    e = fam.engine()
    lengths = KERNEL_SHAPES[name]
    k = 0
    for vary in VARIES:
        hdr, owners, off, cands = _nested_request(fam, e, lengths, vary)
        n = len(cands)
        host, perm = _yard(e, hdr, vary, owners, off, cands)
        row_n = expect(perm, off, cands, E.SELECT_LOOKUP, 0)[1]
        # the yardstick is not degenerate: a group partly kept, and the limits clip some group
        assert ((row_n > 0) & (row_n < np.asarray(lengths))).any() and row_n.max() > min(4, max(lengths) - 1), (name, vary, row_n[:12])
        for group_limit in (0, 1, 4):
            total = int(expect(perm, off, cands, E.SELECT_LOOKUP, group_limit)[0][-1])
            assert total > 1
            for cap in (0, total - 1, total):
                mode = MODES[k % 3]
                k += 1
                got, csr = _filter(e, mode, hdr, vary, owners, off, cands, group_limit=group_limit, cap=cap)
                _same(got, host, (name, vary, group_limit, cap, mode))
                assert _check(csr, perm, off, cands, E.SELECT_LOOKUP, group_limit, cap, (name, vary, group_limit, cap, mode)) == total
                assert np.array_equal(csr["row_n"], row_n)  # unclipped, while row_off follows the limit
    # each optional array absent, and without row_n
    for arrays in (("ids",), ("pos", "perm"), ("perm",)):
        got, csr = _filter(e, MODES[k % 3], hdr, vary, owners, off, cands, group_limit=4, arrays=arrays, row_n=False)
        k += 1
        _check(csr, perm, off, cands, E.SELECT_LOOKUP, 4, n, (name, arrays))
    assert e.device_compact_stats()[0] > 0  # the chunks ran in place
    e.close()


# ---- 3. chunking ----------------------------------------------------------------------------------

def test_chunking():
    """max_batch = 64 and n = 200: four chunks, and a group straddles each of the three boundaries
    (64, 128, 192); on one workspace and on two the results are the default engine's."""
    fam = _family("nested")
    lengths = [50, 30, 70, 0, 45, 5]  # [0, 50, 80, 150, 150, 195, 200]
    e = fam.engine()
    hdr, owners, off, cands = _nested_request(fam, e, lengths)
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    assert ((E.SELECT_LOOKUP >> perm.astype(np.uint32)) & 1).any()
    want = {}
    for vary, group_limit in itertools.product(VARIES, (0, 3)):
        hdr, owners, off, cands = _nested_request(fam, e, lengths, vary)
        s0 = e.device_compact_stats()
        want[vary, group_limit] = _filter(e, "sync", hdr, vary, owners, off, cands, group_limit=group_limit)
        assert sum(e.device_compact_stats()) == sum(s0) + 1  # one chunk
    e.close()
    for workspaces in (1, 2):
        e = fam.engine(max_batch=64, workspaces=workspaces)
        for vary, group_limit in itertools.product(VARIES, (0, 3)):
            hdr, owners, off, cands = _nested_request(fam, e, lengths, vary)
            host, perm = _yard(e, hdr, vary, owners, off, cands)
            s0 = e.device_compact_stats()
            got, csr = _filter(e, "sync", hdr, vary, owners, off, cands, group_limit=group_limit)
            assert sum(e.device_compact_stats()) == sum(s0) + 4, "not four chunks"
            _same(got, host, (workspaces, vary, group_limit))
            _check(csr, perm, off, cands, E.SELECT_LOOKUP, group_limit, 200, (workspaces, vary, group_limit))
            (ww, wr, wc), wcsr = want[vary, group_limit]
            assert np.array_equal(got[0], ww) and got[1] == wr and got[2] == wc
            for key in ("row_off", "row_n", "ids", "pos", "perm"):
                assert np.array_equal(csr[key], wcsr[key]), (workspaces, vary, group_limit, key)
        # the submit form takes n <= max_batch
        for mode in MODES[1:]:
            with pytest.raises(E.GckError) as ei:
                _filter(e, mode, hdr, vary, owners, off, cands)
            assert ei.value.code == E.GCK_E_INVALID_ARGUMENT and "max_batch" in ei.value.message
        # ... and a request of exactly max_batch checks is one
        hdr, owners, off, cands = _nested_request(fam, e, [20, 0, 44])
        host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
        for mode in MODES[1:]:
            got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, owners, off, cands)
            _same(got, host, mode)
            _check(csr, perm, off, cands, E.SELECT_LOOKUP, 0, 64, mode)
        e.close()


# ---- 4. empty forms -------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_empty_forms(mode):
    fam = _family("nested")
    e = fam.engine()
    hdr, owners, off, cands = _nested_request(fam, e, [4, 0, 9])
    s0 = e.device_compact_stats()
    none = np.zeros(0, dtype=np.uint32)
    # S == 0: row_off[0], the count and the error count word alone
    got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, none, np.zeros(1, dtype=np.uint32), none, cap=4, err_cap=2)
    assert got[2] == 0 and got[1] == [] and csr["n"] == 0 and csr["row_off"].tolist() == [0]
    assert len(csr["row_n"]) == 0 and len(csr["ids"]) == 0 and len(csr["pos"]) == 0 and len(csr["perm"]) == 0
    # n == 0 with S == 3: S + 1 zero offsets and S zero counts (the offsets are not read: the call gets none)
    got, csr = _filter(e, mode, hdr, E.VARY_SUBJECT, owners, np.zeros(4, dtype=np.uint32), none, cap=4, err_cap=2)
    assert got[2] == 0 and got[1] == [] and csr["n"] == 0 and csr["row_off"].tolist() == [0, 0, 0, 0]
    assert csr["row_n"].tolist() == [0, 0, 0] and len(csr["ids"]) == 0 and len(csr["pos"]) == 0
    assert e.device_compact_stats() == s0  # an empty request is no chunk
    # a request of empty groups around one candidate
    hdr, owners, off, cands = _nested_request(fam, e, [0, 0, 1, 0])
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, owners, off, cands, select=E.SELECT_LOOKUP | E.SELECT_NO)
    _same(got, host)
    _check(csr, perm, off, cands, E.SELECT_LOOKUP | E.SELECT_NO, 0, 1)
    assert csr["n"] == 1 and csr["row_off"].tolist() == [0, 0, 0, 1, 1]
    e.close()


# ---- 5. malformed offsets: refused by a kernel's verdict, never a fault ---------------------------

MALFORMED = {  # lengths [10, 20, 30, 40]: good offsets [0, 10, 30, 60, 100]
    "descending_pair": ([0, 10, 60, 30, 100], 2),
    "last_is_not_n": ([0, 10, 30, 60, 90], 4),
    "first_is_not_zero": ([5, 10, 30, 60, 100], 0),
}


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_offsets(name):
    """The clamps keep every kernel of the request inside its buffers whatever the offsets hold, so
    this is an argument error like any other: GCK_E_INVALID_ARGUMENT from the call or the wait, naming
    the smallest bad s; nothing beyond any output array written; the engine answers on."""
    fam = _family("nested")
    e = fam.engine()
    hdr, owners, off, cands = _nested_request(fam, e, [10, 20, 30, 40])
    bad_off, bad_s = MALFORMED[name]
    bad_off = np.asarray(bad_off, dtype=np.uint32)
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    for mode in MODES:
        outs = []
        with pytest.raises(E.GckError) as ei:
            _filter(e, mode, hdr, E.VARY_RESOURCE, owners, bad_off, cands, cap=50, err_cap=3, outs=outs)
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        assert f"s = {bad_s} " in ei.value.message, ei.value.message
        outs[0].guards(), outs[1].guards()
        # a following well-formed request is answered correctly
        got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, owners, off, cands, group_limit=5)
        _same(got, host, (name, mode))
        _check(csr, perm, off, cands, E.SELECT_LOOKUP, 5, 100, (name, mode))
    e.close()


# ---- 6. per-item errors ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_per_item_errors(mode):
    fam = _family("nested")
    e = fam.engine()
    lengths = [5, 0, 33, 40]
    hdr, owners, off, cands = _nested_request(fam, e, lengths)
    # every check an error: counted and listed, no survivor, the call succeeds
    bad = _bad_permission(e, hdr)
    host, perm = _yard(e, bad, E.VARY_RESOURCE, owners, off, cands)
    assert host[2] == 78 and not perm.any()
    for select in (E.SELECT_LOOKUP, E.SELECT_NO | E.SELECT_LOOKUP):
        got, csr = _filter(e, mode, bad, E.VARY_RESOURCE, owners, off, cands, select=select)
        _same(got, host, mode)
        assert got[2] == 78 and [k for k, _ in got[1]] == list(range(78))
        assert csr["n"] == 0 and csr["row_off"].tolist() == [0] * 5 and csr["row_n"].tolist() == [0] * 4
        assert len(csr["ids"]) == 0
    # a short error list: the count is whole, the first err_cap records are written
    got, csr = _filter(e, mode, bad, E.VARY_RESOURCE, owners, off, cands, err_cap=4)
    assert got[2] == 78 and [k for k, _ in got[1]] == [0, 1, 2, 3]
    # a wildcard subject id as one owner: its group's checks are errors, the others are answered
    wild = owners.copy()
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    assert ((E.SELECT_LOOKUP >> perm[38:].astype(np.uint32)) & 1).any()  # (the last owner's group has survivors to lose)
    wild[3] = E.ID_WILDCARD
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, wild, off, cands)
    assert [k for k, _ in host[1]] == list(range(38, 78)), host[1][:3]
    assert ((E.SELECT_LOOKUP >> perm.astype(np.uint32)) & 1).any()
    for select in (E.SELECT_LOOKUP, E.SELECT_NO | E.SELECT_LOOKUP):
        got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, wild, off, cands, select=select)
        _same(got, host, (mode, "wildcard"))
        _check(csr, perm, off, cands, select, 0, 78, (mode, "wildcard"))
        assert csr["row_n"][3] == 0 and not set(range(38, 78)) & set(csr["pos"].tolist())
    # an error-free request after them: the error count is written as 0
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    got, csr = _filter(e, mode, hdr, E.VARY_RESOURCE, owners, off, cands, err_cap=4)
    assert got[2] == 0 and got[1] == []
    _same(got, host)
    _check(csr, perm, off, cands, E.SELECT_LOOKUP, 0, 78)
    e.close()


# ---- 7. expanded on the device --------------------------------------------------------------------

def test_expanded_check_contexts():
    """Check contexts force the expansion: k_dc_expand reads the pairs k_dc_group_pairs wrote."""
    from tests.test_gpu_device_cross import CTXS
    fam = _family("caveated")
    e = fam.engine()
    shape = SHAPE
    res, sub = fam.shapes[shape]
    sub, res = sub[:12], res[:35]
    lengths, idx = _ragged(len(sub), len(res), 5)
    hdr, sids, rids = _ids(e, shape, sub, [res[i] for i in idx])
    off = offsets(lengths)
    k = 0
    for slot in (0, 1, 2):
        host, perm = _yard(e, hdr + (slot,), E.VARY_RESOURCE, sids, off, rids, contexts=CTXS)
        if slot == 0:
            assert (perm == E.PERM_CONDITIONAL).any() and (perm == E.PERM_HAS).any()
        for select in (E.SELECT_LOOKUP, E.SELECT_CONDITIONAL):
            s0 = e.device_compact_stats()
            mode = MODES[k % 3]
            k += 1
            got, csr = _filter(e, mode, hdr + (slot,), E.VARY_RESOURCE, sids, off, rids, select=select, contexts=CTXS)
            assert e.device_compact_stats() == (s0[0], s0[1] + 1), "not expanded"
            _same(got, host, (slot, select, mode))
            _check(csr, perm, off, rids, select, 0, len(rids), (slot, select, mode))
    e.close()


# ---- 8. refusals before any launch ----------------------------------------------------------------

def test_argument_errors():
    fam = _family("nested")
    e = fam.engine()
    hdr, owners, off, cands = _nested_request(fam, e, [10, 0, 30])
    do, dg, dc = _u32(np.concatenate([owners, owners])), _u32(np.concatenate([off, off])), _u32(np.concatenate([cands, cands]))
    out, csr = _Plane(40, 8), _Csr(3, 16)
    torch.cuda.synchronize()
    good = dict(out.args(), **csr.args())
    s0, b0 = e.device_compact_stats(), e.stats()["batches"]

    def refused(fn, hdr=hdr, S=3, n=40, d_o=do.data_ptr(), d_g=dg.data_ptr(), d_c=dc.data_ptr(), **changes):
        with pytest.raises(E.GckError) as ei:
            r = fn(hdr, d_o, S, d_g, d_c, n, **dict(good, **changes))
            if hasattr(r, "wait"):
                r.wait()
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        return ei.value.message

    for fn in (e.filter_groups_device, e.submit_filter_groups_device):
        for mask in (0, 1, 3, 15, 16, 0x12):
            assert "mask" in refused(fn, select=mask)
        assert "reserved" in refused(fn, hdr=E.Uniform(*hdr[:4], 0, 7))
        for vary in (0, 3):
            assert "vary" in refused(fn, vary=vary)
        assert "d_out_row_off" in refused(fn, d_out_row_off=0)
        assert "d_out_n" in refused(fn, d_out_n=0)
        assert "d_out_packed" in refused(fn, d_out_packed=0)
        assert "cap" in refused(fn, d_out_ids=0, d_out_pos=0, d_out_perm=0)
        assert "2^32" in refused(fn, n=2 ** 32) and "2^32" in refused(fn, S=2 ** 32)
        assert "without a group" in refused(fn, S=0)
        for null in ("d_o", "d_g", "d_c"):
            assert "null" in refused(fn, **{null: 0})
        assert "8-byte" in refused(fn, d_out_packed=good["d_out_packed"] + 4)
        for name in ("d_o", "d_g", "d_c"):
            assert "aligned" in refused(fn, **{name: do.data_ptr() + 2}), name
        for name in ("d_out_row_off", "d_out_row_n", "d_out_ids", "d_out_pos", "d_out_n", "d_out_errs", "d_out_n_errs"):
            assert "aligned" in refused(fn, **{name: good[name] + 2}), name
        assert "context_slot" in refused(fn, hdr=hdr + (1,))
        refused(fn, d_out_errs=0)
    # a null gck_select_groups
    cs, tail = e._device_tail(E.CONSISTENCY_MIN_LATENCY, 0, NOW_US, None, good["d_out_packed"], good["d_out_errs"], 8,
                              good["d_out_n_errs"])
    rev = E.C.c_uint64(0)
    rc = e._lib.gck_filter_groups_device(e._h, E.C.byref(cs), E.C.byref(E._header(hdr)), E.VARY_RESOURCE, do.data_ptr(), 3,
                                         dg.data_ptr(), dc.data_ptr(), 40, *tail[:4], None, *tail[4:], None, E.C.byref(rev))
    assert rc == E.GCK_E_INVALID_ARGUMENT
    out.untouched(), csr.untouched()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, owners, off, cands)
    got, c = _filter(e, "engine", hdr, E.VARY_RESOURCE, owners, off, cands)
    _same(got, host, "after refusals")
    _check(c, perm, off, cands, E.SELECT_LOOKUP, 0, 40)
    e.close()


# ---- 9. the torch and client surface --------------------------------------------------------------

def test_filter_groups_ids():
    fam = _family("gdocs")
    e = fam.engine()
    shape = SHAPE
    res, sub = fam.shapes[shape]
    sub = sub[:9]
    lengths, idx = _ragged(len(sub), len(res), 11)
    hdr, sids, rids = _ids(e, shape, sub, [res[i] for i in idx])  # (repeated ids are reported as often as they are listed)
    off = offsets(lengths)
    host, perm = _yard(e, hdr, E.VARY_RESOURCE, sids, off, rids)
    assert host[2] == 0 and ((E.SELECT_LOOKUP >> perm.astype(np.uint32)) & 1).sum() > 9
    n = len(rids)
    for dtype, limit in itertools.product((torch.int32, torch.uint32), (0, 2)):
        to, tg, tc = _u32(sids).view(dtype), _u32(off).view(dtype), _u32(rids).view(dtype)
        row_off, ids, pos, pm = e.filter_groups_ids(hdr, to, tg, tc, group_limit=limit, want_pos=True, want_perm=True,
                                                    now_us=NOW_US)
        assert row_off.is_cuda and row_off.dtype == torch.int32 and ids.dtype == dtype and pm.dtype == torch.uint8
        csr = {"row_off": _np(row_off), "n": int(row_off[-1]), "row_n": None, "ids": _np(ids.view(torch.int32)),
               "pos": _np(pos), "perm": pm.cpu().numpy()}
        _check(csr, perm, off, rids, E.SELECT_LOOKUP, limit, n, (dtype, limit))
        two = e.filter_groups_ids(hdr, to, tg, tc, select=E.SELECT_NO, group_limit=limit, now_us=NOW_US)
        assert len(two) == 2
        want = expect(perm, off, rids, E.SELECT_NO, limit)
        assert np.array_equal(_np(two[0]), want[0]) and np.array_equal(_np(two[1].view(torch.int32)), want[2])
    # the mirror: the same pairs grouped the other way round answer alike
    hdr2, sids2, rids2 = _ids(e, shape, [sub[i % len(sub)] for i in range(7)], res[:3])
    off2 = offsets([3, 0, 4])
    host2, perm2 = _yard(e, hdr2, E.VARY_SUBJECT, rids2, off2, sids2)
    row_off, ids = e.filter_groups_ids(hdr2, _u32(rids2), _u32(off2), _u32(sids2), vary=E.VARY_SUBJECT, now_us=NOW_US)
    want = expect(perm2, off2, sids2, E.SELECT_LOOKUP, 0)
    assert np.array_equal(_np(row_off), want[0]) and np.array_equal(_np(ids), want[2])
    empty = e.filter_groups_ids(hdr, _u32(sids), _u32(np.zeros(len(sids) + 1)), _u32(rids[:0]))
    assert empty[0].tolist() == [0] * (len(sids) + 1) and empty[1].numel() == 0
    with pytest.raises(E.GckError):  # a per-item error: raised, as filter_cross_ids raises it
        e.filter_groups_ids(_bad_permission(e, hdr), _u32(sids), _u32(off), _u32(rids))
    for host_arg in range(3):  # a host tensor is refused
        args = [_u32(sids), _u32(off), _u32(rids)]
        args[host_arg] = args[host_arg].cpu()
        with pytest.raises(E.GckError) as ei:
            e.filter_groups_ids(hdr, *args)
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    with pytest.raises(E.GckError):  # S + 1 offsets
        e.filter_groups_ids(hdr, _u32(sids), _u32(off[:-1]), _u32(rids))
    with pytest.raises(E.GckError) as ei:  # malformed offsets surface as the call's error
        e.filter_groups_ids(hdr, _u32(sids), _u32(off[::-1].copy()), _u32(rids))
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT and "s = 0 " in ei.value.message
    e.close()


def test_client_groups_against_filter_resources():
    from gochugaru_amd.client import InvalidArgument
    g = load_golden("readme_founders.json")
    e = E.Engine(device=0)
    e.load_schema(g["schema"])
    e.load_snapshot_text(1, "\n".join(g["tuples"]))
    c = Client(e)
    cs = consistency.MinLatency()
    subjects = ["user:jake", "user:nobody_of_that_name", "user:joey", "user:jimmy"]
    companies = ["company:authzed", "company:no_such_company"]
    # each subject's own candidates: repeated, unknown, none at all
    own = [[0, 1, 0], [0, 1], [], [1, 0, 0, 0]]
    user, company = e.type_id("user"), e.type_id("company")
    sids = _u32(e.intern(user, [s.split(":")[1] for s in subjects]))
    flat = [companies[i] for grp in own for i in grp]
    cids = e.intern(company, [r.split(":")[1] for r in flat])
    id_of = {name.split(":")[1]: int(i) for name, i in zip(flat, cids)}
    off = offsets([len(grp) for grp in own])
    for limit in (0, 1, 2):
        want_off, want_ids = [0], []
        for s, grp in zip(subjects, own):  # FilterResources per owner over that owner's candidates
            kept = []
            for name, err in c.FilterResources(None, cs, "company#founder", s, [companies[i] for i in grp]):
                assert err is None
                kept.append(id_of[name])
            want_ids += kept[:limit or None]
            want_off.append(len(want_ids))
        assert want_ids  # (jake and jimmy founded authzed)
        for dtype in (torch.int32, torch.uint32):
            (row_off, ids), err = c.FilterGroupsDevice(None, cs, "company#founder", _u32(cids).view(dtype),
                                                       _u32(off).view(dtype), "user", sids.view(dtype), limit=limit)
            assert err is None and ids.is_cuda and ids.dtype == dtype
            assert row_off.tolist() == want_off and _np(ids.view(torch.int32)).tolist() == want_ids, limit
    # the mirror: for each company, which of its own candidate users
    users = [["jake", "nobody_of_that_name", "jimmy", "jake"], ["joey"]]
    uflat = [u for grp in users for u in grp]
    uids = e.intern(user, uflat)
    uid_of = {u: int(i) for u, i in zip(uflat, uids)}
    rids = _u32(e.intern(company, ["authzed", "no_such_company"]))
    uoff = offsets([len(grp) for grp in users])
    for limit in (0, 2):
        want_off, want_ids = [0], []
        for r, grp in zip(companies, users):
            kept = []
            for name, err in c.FilterSubjects(None, cs, r, "founder", ["user:" + u for u in grp]):
                assert err is None
                kept.append(uid_of[name])
            want_ids += kept[:limit or None]
            want_off.append(len(want_ids))
        assert want_ids
        (row_off, ids), err = c.FilterGroupSubjectsDevice(None, cs, "company#founder", rids, "user", _u32(uids), _u32(uoff),
                                                          limit=limit)
        assert err is None and row_off.tolist() == want_off and _np(ids).tolist() == want_ids, limit
    # the same refusals and errors as FilterCrossDevice's
    out, err = c.FilterGroupsDevice(None, cs, "company#founder", _u32(cids).cpu(), _u32(off), "user", sids)
    assert out is None and isinstance(err, InvalidArgument)
    out, err = c.FilterGroupsDevice(None, cs, "company#founder", _u32(cids), _u32(off).cpu(), "user", sids)
    assert out is None and isinstance(err, InvalidArgument)
    out, err = c.FilterGroupsDevice(None, cs, "company#founder", _u32(cids), _u32(off), "user", sids, limit=-1)
    assert out is None and isinstance(err, InvalidArgument)
    out, err = c.FilterGroupsDevice(None, cs, "company#no_such_permission", _u32(cids), _u32(off), "user", sids)
    assert out is None and isinstance(err, E.GckError)
    e.close()
