"""Compact requests over device buffers (include/gck.h gck_check_bulk_uniform_device, _shaped_device,
_list_device and their submit forms): ids, index bytes, the packed plane, the error list and its
count all live in device memory (torch tensors on cuda:0).

Bar: the host compact call on the same request — the words bit for bit, the (index, code) records
and the count — and, where said, the oracle directly. Every output buffer starts poisoned: the
plane with 0xFF.. (and a word beyond it, which must stay), the error list and the count with a
sentinel (the entries beyond min(count, err_cap) must stay)."""
import numpy as np
import pytest
import torch

from gochugaru_amd import engine as E
from tests import gen
from tests.helpers import oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
POISON = 0xFFFFFFFFFFFFFFFF
SENT = 0x5A5A5A5A
R, S = E.VARY_RESOURCE, E.VARY_SUBJECT
FAMS = ["gdocs", "nested", "cyclic", "near_budget", "caveated", "hub_arrow"]
MODES = ["sync", "engine", "stream"]  # the synchronous call, a submit on the workspace's stream, one on the caller's


def _dev():
    return torch.device("cuda", 0)


def _engine(schema, tuples, revision=1, **kw):
    e = E.Engine(device=0, **kw)
    e.load_schema(schema)
    e.load_snapshot_text(revision, "\n".join(tuples))
    return e


def _u32(a):
    """A u32 numpy array as a device tensor (its bits as int32)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(_dev())


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).to(_dev())


def _records(errs):
    return [(int(x["index"]), int(x["code"])) for x in errs]


class _Out:
    """The device outputs of one request, poisoned: n_words + 1 words, err_cap + 2 records, the count."""

    def __init__(self, n, cap, count=True):
        self.nw, self.cap = (n + 31) // 32, cap
        self.words = torch.full((self.nw + 1,), -1, dtype=torch.int64, device=_dev())
        self.errs = torch.full((cap + 2, 2), SENT, dtype=torch.int32, device=_dev())
        self.cnt = torch.full((1,), SENT, dtype=torch.int32, device=_dev()) if count else None

    def args(self):
        return dict(d_out_packed=self.words.data_ptr(), d_out_errs=self.errs.data_ptr() if self.cap else 0,
                    err_cap=self.cap, d_out_n_errs=self.cnt.data_ptr() if self.cnt is not None else 0)

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


def _call(e, mode, sync, submit, head, out, contexts=None, **kw):
    kw.update(out.args(), now_us=NOW_US, contexts=contexts)
    if mode != "stream":
        torch.cuda.synchronize()  # (an engine-stream submit: the inputs are complete at the call)
    st = torch.cuda.current_stream().cuda_stream
    if mode == "sync":
        rev = sync(*head, stream=st, **kw)
    else:
        rev = submit(*head, stream=st, engine_stream=(mode == "engine"), **kw).wait()
    assert rev == e.revision
    return out.read()


def _uniform(e, mode, hdr, pairs, cap=None, count=True, contexts=None):
    n = len(pairs)
    d = _u32(pairs)
    return _call(e, mode, e.check_uniform_device, e.submit_uniform_device, (hdr, d.data_ptr(), n),
                 _Out(n, n if cap is None else cap, count), contexts)


def _shaped(e, mode, shapes, shape_of, pairs, cap=None, count=True, contexts=None):
    n = len(pairs)
    di, dp = _u8(shape_of), _u32(pairs)
    return _call(e, mode, e.check_shaped_device, e.submit_shaped_device, (shapes, di.data_ptr(), dp.data_ptr(), n),
                 _Out(n, n if cap is None else cap, count), contexts)


def _list(e, mode, hdr, fixed, vary, n, ids=None, first=0, cap=None, contexts=None):
    d = _u32(ids) if ids is not None else None
    return _call(e, mode, e.check_list_device, e.submit_list_device, (hdr, fixed, vary, n),
                 _Out(n, n if cap is None else cap), contexts, d_ids=d.data_ptr() if d is not None else 0, first_id=first)


def _host(res):
    """A host compact call's (words, errs, revision) as (words, records, count): its list is uncapped."""
    words, errs, _ = res
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


def _dense(want):
    """The oracle's (perm, err) per check as (words, records, count)."""
    words = np.zeros((len(want) + 31) // 32, dtype=np.uint64)
    rec = []
    for k, (p, x) in enumerate(want):
        if x:
            rec.append((k, x))
        else:
            words[k // 32] |= np.uint64(int(p) << (2 * (k % 32)))
    return words, rec, len(rec)


class _Family:
    """A family at seed 2: the graph, the oracle's answer of every check, and the checks as one
    shaped request (shared by the tests: computed once, never changed)."""

    def __init__(self, name):
        self.name = name
        self.schema, self.tuples, self.checks = gen.FAMILIES[name](2)
        self.depth = gen.FAMILY_DEPTH.get(name, 50)
        ck = oracle_for(self.schema, self.tuples, max_depth=self.depth, now=NOW_US / 1e6)
        self.want = [tuple(ck.check(to_oracle_item(parse_check(c)))) for c in self.checks]

    def engine(self, **kw):
        return _engine(self.schema, self.tuples, max_depth=self.depth, **kw)

    def request(self, e):
        items = e.make_items([parse_check(c) for c in self.checks])
        shapes, shape_of, pairs = E.shape_request(items)
        return shapes, np.asarray(shape_of, dtype=np.uint8), np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)


_FAMILIES = {}


def _family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = _Family(name)
    return _FAMILIES[name]


# ---- 1. parity per family -------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMS)
def test_family_parity(family):
    fam = _family(family)
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    assert len(shapes) >= 2
    # every shape as a uniform request: the host call and the oracle
    for j, shape in enumerate(shapes):
        at = np.flatnonzero(shape_of == j)
        got = _uniform(e, MODES[j % 3], shape, pairs[at])
        _same(got, _host(e.check_uniform(shape, pairs[at], now_us=NOW_US)), (family, "uniform", shape))
        _same(got, _dense([fam.want[k] for k in at]), (family, "uniform vs oracle", shape))
    # the whole check list as one shaped request
    host = _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US))
    for mode in MODES:
        got = _shaped(e, mode, shapes, shape_of, pairs)
        _same(got, host, (family, "shaped", mode))
        _same(got, _dense(fam.want), (family, "shaped vs oracle", mode))
    # one subject against the resources, one resource against the subjects, and one range
    j = int(np.argmax(np.bincount(shape_of)))
    hdr, at = shapes[j], np.flatnonzero(shape_of == j)
    res, sub = pairs[at, 0].copy(), pairs[at, 1].copy()
    _same(_list(e, "sync", hdr, int(sub[0]), R, len(res), ids=res),
          _host(e.check_list(hdr, int(sub[0]), R, res, now_us=NOW_US)), (family, "list R"))
    _same(_list(e, "engine", hdr, int(res[0]), S, len(sub), ids=sub),
          _host(e.check_list(hdr, int(res[0]), S, sub, now_us=NOW_US)), (family, "list S"))
    m = min(e.object_count(hdr[0]), 45)
    _same(_list(e, "stream", hdr, int(sub[0]), R, m, first=0),
          _host(e.check_list(hdr, int(sub[0]), R, None, 0, m, now_us=NOW_US)), (family, "range"))
    e.close()


# ---- 2. word edges --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nested():
    fam = _family("nested")
    e = fam.engine(workspaces=8)
    shapes, shape_of, pairs = fam.request(e)
    yield fam, e, shapes, shape_of, pairs
    e.close()


def _plain(shapes, shape_of):
    """The plain (user subject) shape with the most checks."""
    plain = [j for j, s in enumerate(shapes) if s[3] == E.ELLIPSIS]
    return max(plain, key=lambda j: int(np.count_nonzero(shape_of == j)))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65])
def test_word_edges(nested, n):
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)][:n]
    assert len(p) == n
    host = _host(e.check_uniform(shapes[j], p, now_us=NOW_US))
    s0 = e.device_compact_stats()
    for mode in ("engine", "sync"):
        _same(_uniform(e, mode, shapes[j], p), host, (n, mode))  # (tail bits 0, the next word kept: _Out.read)
        ids = p[:, 0].copy()
        _same(_list(e, mode, shapes[j], int(p[0, 1]), R, n, ids=ids),
              _host(e.check_list(shapes[j], int(p[0, 1]), R, ids, now_us=NOW_US)), (n, mode, "list"))
    assert e.device_compact_stats() == (s0[0] + 4, s0[1])


# ---- 3. deferred checks sharing a word ------------------------------------------------------------

def test_deferred_checks_share_a_word():
    """A userset-subject shape of the Google-Docs graph: its join leaves such checks to the bundle
    stages, so several deferred checks share each 32-check word of the plane."""
    fam = _family("gdocs")
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    userset = [j for j, s in enumerate(shapes) if s[3] != E.ELLIPSIS]
    assert userset
    j = userset[0]
    p = pairs[np.flatnonzero(shape_of == j)]
    p = np.concatenate([p] * (40 // len(p) + 1))[:40]  # (ids are not deduplicated)
    host = _host(e.check_uniform(shapes[j], p, now_us=NOW_US))
    for mode in MODES:
        e.reset_stats()
        s0 = e.device_compact_stats()
        _same(_uniform(e, mode, shapes[j], p), host, mode)
        st = e.stats()
        left = st["queries"] - st["closure_checks"]
        print(f"{mode}: {left} of {st['queries']} checks left by the join")
        assert e.device_compact_stats() == (s0[0] + 1, s0[1]), "not in place"
        # (40 checks are two words: three left checks put two in one word)
        assert st["queries"] == 40 and left >= 3, "the join left fewer than two checks of one word"
    # a plain shape among them, shaped: decided and deferred checks in one word
    k = _plain(shapes, shape_of)
    q = pairs[np.flatnonzero(shape_of == k)][:40]
    mix_idx = np.array([i % 2 for i in range(40)], dtype=np.uint8)
    mix = np.where(mix_idx[:, None] == 0, q, p).astype(np.uint32)
    table = [shapes[k], shapes[j]]
    host = _host(e.check_shaped(table, mix_idx, mix, now_us=NOW_US))
    assert len(set(E.unpack_results(host[0], 40).tolist())) >= 2  # (both answers among them)
    for mode in MODES:
        _same(_shaped(e, mode, table, mix_idx, mix), host, ("mixed", mode))
    e.close()


# ---- 4. the error list protocol -------------------------------------------------------------------

def _with_errors(e, shapes, shape_of, pairs, n, bad_at):
    """A shaped request of n checks of the plain shape in which the checks at `bad_at` use a table
    entry naming a permission the resource type lacks (a relation of the subject's side)."""
    j = _plain(shapes, shape_of)
    good = shapes[j]
    group = e.type_id("group")
    bad = (good[0], e.relation_id(group, "member"), good[2], good[3], 0)
    p = pairs[np.flatnonzero(shape_of == j)]
    p = np.concatenate([p] * (n // len(p) + 1))[:n].astype(np.uint32)
    idx = np.zeros(n, dtype=np.uint8)
    idx[list(bad_at)] = 1
    return [good, bad], idx, p


@pytest.mark.parametrize("mode", MODES)
def test_error_list_protocol(nested, mode):
    fam, e, shapes, shape_of, pairs = nested
    bad_at = [2, 3, 31, 32, 70, 95, 96, 199]
    table, idx, p = _with_errors(e, shapes, shape_of, pairs, 200, bad_at)
    host = _host(e.check_shaped(table, idx, p, now_us=NOW_US))
    assert [k for k, _ in host[1]] == bad_at and host[2] == len(bad_at)
    for cap in (0, 1, len(bad_at), len(bad_at) + 5):
        got = _shaped(e, mode, table, idx, p, cap=cap)
        _same(got, host, (mode, cap))
        assert len(got[1]) == min(cap, len(bad_at)) and got[2] == len(bad_at)
        got = _shaped(e, mode, table, idx, p, cap=cap, count=False)  # d_out_n_errs == NULL
        _same(got, host, (mode, cap, "no count"))
        assert len(got[1]) == min(cap, len(bad_at))
    # an error-free request after them: the count is written as 0
    got = _shaped(e, mode, table, np.zeros(50, dtype=np.uint8), p[:50], cap=4)
    assert got[2] == 0 and got[1] == []


def test_empty_request_writes_the_count(nested):
    fam, e, shapes, shape_of, pairs = nested
    for mode in MODES:
        out = _Out(0, 2)
        got = _call(e, mode, e.check_uniform_device, e.submit_uniform_device, (shapes[0], 0, 0), out)
        assert got[2] == 0 and got[1] == []


# ---- 5. chunks ------------------------------------------------------------------------------------

@pytest.mark.parametrize("workspaces", [0, 1], ids=["two-workspaces", "one-workspace"])
def test_chunks(workspaces):
    fam = _family("nested")
    e = fam.engine(max_batch=64, workspaces=workspaces)
    shapes, shape_of, pairs = fam.request(e)
    n = 64 * 2 + 40
    bad_at = [5, 63, 130, 167]  # the first and the last chunk
    table, idx, p = _with_errors(e, shapes, shape_of, pairs, n, bad_at)
    host = _host(e.check_shaped(table, idx, p, now_us=NOW_US))
    assert [k for k, _ in host[1]] == bad_at
    s0 = e.device_compact_stats()
    _same(_shaped(e, "sync", table, idx, p), host, "shaped")
    _same(_shaped(e, "sync", table, idx, p, cap=3), host, "shaped, cap 3")
    _same(_shaped(e, "sync", table, idx, p, cap=3, count=False), host, "shaped, no count")
    assert sum(e.device_compact_stats()) == sum(s0) + 9
    # the uniform and list forms across chunks
    j = _plain(shapes, shape_of)
    _same(_uniform(e, "sync", shapes[j], p), _host(e.check_uniform(shapes[j], p, now_us=NOW_US)), "uniform")
    ids = p[:, 0].copy()
    _same(_list(e, "sync", shapes[j], int(p[0, 1]), R, n, ids=ids),
          _host(e.check_list(shapes[j], int(p[0, 1]), R, ids, now_us=NOW_US)), "list")
    m = min(e.object_count(shapes[j][0]), n)
    assert m > 64
    _same(_list(e, "sync", shapes[j], int(p[0, 1]), R, m, first=0),
          _host(e.check_list(shapes[j], int(p[0, 1]), R, None, 0, m, now_us=NOW_US)), "range")
    e.close()


# ---- 6. every engine path -------------------------------------------------------------------------

def _all_forms(e, shapes, shape_of, pairs, contexts=None):
    host = _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US, contexts=contexts))
    for mode in MODES:
        _same(_shaped(e, mode, shapes, shape_of, pairs, contexts=contexts), host, ("shaped", mode))
    j = int(np.argmax(np.bincount(shape_of)))
    at = np.flatnonzero(shape_of == j)
    p = pairs[at]
    hu = _host(e.check_uniform(shapes[j], p, now_us=NOW_US, contexts=contexts))
    for mode in MODES:
        _same(_uniform(e, mode, shapes[j], p, contexts=contexts), hu, ("uniform", mode))
    ids = p[:, 0].copy()
    _same(_list(e, "engine", shapes[j], int(p[0, 1]), R, len(ids), ids=ids, contexts=contexts),
          _host(e.check_list(shapes[j], int(p[0, 1]), R, ids, now_us=NOW_US, contexts=contexts)), "list")
    m = min(e.object_count(shapes[j][0]), 40)
    _same(_list(e, "sync", shapes[j], int(p[0, 1]), R, m, first=0, contexts=contexts),
          _host(e.check_list(shapes[j], int(p[0, 1]), R, None, 0, m, now_us=NOW_US, contexts=contexts)), "range")
    return 3 + 3 + 2


@pytest.mark.parametrize("kw", [{}, {"labels": False}, {"closure": False, "labels": False}, {"wide_only": True},
                                {"profile": True}],
                         ids=["default", "no-labels", "no-join", "wide-only", "profiling"])
def test_every_engine_path(kw):
    fam = _family("gdocs")
    e = fam.engine(**kw)
    shapes, shape_of, pairs = fam.request(e)
    others = (e.shaped_stats(), e.list_stats(), e.cross_stats())
    s0 = e.device_compact_stats()
    k = _all_forms(e, shapes, shape_of, pairs)
    s1 = e.device_compact_stats()
    print(kw, "device_compact_stats", s0, "->", s1)
    if not kw:
        assert s1 == (s0[0] + k, s0[1])
    elif kw == {"labels": False}:
        # (the closure join alone is a one-round join where the snapshot has one: such chunks run in
        # place, as the host forms' do; without one they are expanded)
        assert s1[0] + s1[1] == s0[0] + s0[1] + k
    else:
        assert s1 == (s0[0], s0[1] + k)
    # the host requests' counters do not see device requests (the host yardstick calls are counted)
    shaped, lst, cross = e.shaped_stats(), e.list_stats(), e.cross_stats()
    assert sum(shaped) == sum(others[0]) + 1 and sum(lst) == sum(others[1]) + 2 and cross == others[2]
    e.close()


def test_header_context_slot():
    fam = _family("caveated")
    e = fam.engine()
    ctxs = [{"day_of_the_week": "tuesday"}, {"day_of_the_week": "monday"}]
    shapes, shape_of, pairs = fam.request(e)
    shapes = [s[:4] + (1 + k % 2,) for k, s in enumerate(shapes)]
    s0 = e.device_compact_stats()
    k = _all_forms(e, shapes, shape_of, pairs, contexts=ctxs)
    assert e.device_compact_stats() == (s0[0], s0[1] + k)
    # the oracle, directly: check k under its shape's context
    ck = oracle_for(fam.schema, fam.tuples, max_depth=fam.depth, now=NOW_US / 1e6)
    want = [tuple(ck.check(to_oracle_item(parse_check(c), ctxs[shapes[shape_of[i]][4] - 1])))
            for i, c in enumerate(fam.checks)]
    assert len(set(want)) >= 2
    _same(_shaped(e, "sync", shapes, shape_of, pairs, contexts=ctxs), _dense(want), "oracle")
    e.close()


# ---- 7. a bad shape index found on the device -----------------------------------------------------

@pytest.mark.parametrize("kw", [{}, {"profile": True}, {"max_batch": 64}], ids=["in-place", "expanded", "chunks"])
def test_bad_shape_index(kw):
    fam = _family("nested")
    e = fam.engine(**kw)
    shapes, shape_of, pairs = fam.request(e)
    n = 150
    assert len(shape_of) >= n
    shape_of, pairs = shape_of[:n], pairs[:n]
    broken = shape_of.copy()
    broken[[77, 140]] = len(shapes)
    modes = ["sync"] if "max_batch" in kw else MODES  # (a submitted batch is at most max_batch)
    for mode in modes:
        with pytest.raises(E.GckError) as ei:
            _shaped(e, mode, shapes, broken, pairs)
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
        assert f"shape_of[77] = {len(shapes)}" in ei.value.message, ei.value.message
        # the engine answers the next request
        _same(_shaped(e, mode, shapes, shape_of, pairs), _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US)), mode)
    e.close()


# ---- 8. refusals before any launch ----------------------------------------------------------------

def test_refusals(nested):
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    hdr = shapes[j]
    n = 64
    big = torch.zeros(4 * n + 8, dtype=torch.int32, device=_dev())   # pairs / ids, with room for an offset
    words = torch.zeros(n, dtype=torch.int64, device=_dev())
    errs = torch.zeros((n + 1, 2), dtype=torch.int32, device=_dev())
    cnt = torch.zeros(4, dtype=torch.int32, device=_dev())
    idx = torch.zeros(n, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    P, W, X, N, I = big.data_ptr(), words.data_ptr(), errs.data_ptr(), cnt.data_ptr(), idx.data_ptr()
    s0 = e.device_compact_stats()
    b0 = e.stats()["batches"]

    def refused(fn, *a, **k):
        with pytest.raises(E.GckError) as ei:
            r = fn(*a, **k)
            if hasattr(r, "wait"):
                r.wait()
        assert ei.value.code == E.GCK_E_INVALID_ARGUMENT, ei.value.message
        return ei.value.message

    for sync, submit in ((e.check_uniform_device, e.submit_uniform_device),):
        for fn in (sync, submit):
            assert "d_pairs" in refused(fn, hdr, P + 4, n, W, X, n, N)               # misaligned pairs
            assert "d_out_packed" in refused(fn, hdr, P, n, W + 4, X, n, N)          # misaligned plane
            refused(fn, hdr, P, n, W, X + 2, n, N)                                   # misaligned records
            refused(fn, hdr, P, n, W, X, n, N + 2)                                   # misaligned count
            refused(fn, hdr, 0, n, W, X, n, N)                                       # null buffers with n > 0
            refused(fn, hdr, P, n, 0, X, n, N)
            refused(fn, hdr, P, n, W, 0, n, N)                                       # err_cap without a list
            refused(fn, hdr[:4] + (1,), P, n, W, X, n, N)                            # a slot beyond the contexts
    for fn in (e.check_list_device, e.submit_list_device):
        refused(fn, hdr, 0, S, n, W, 0, 0, X, n, N)                                  # a range with VARY_SUBJECT
        refused(fn, hdr, 0, 3, n, W, P, 0, X, n, N)                                  # vary neither value
        refused(fn, hdr, 0, R, n, W, P + 2, 0, X, n, N)                              # misaligned ids
        refused(fn, E.Uniform(*hdr[:4], 0, 7), 0, R, n, W, P, 0, X, n, N)            # reserved != 0
        refused(fn, hdr, 0xFFFFFFF0, R, n, W, 0, 0xFFFFFFF0, X, n, N)                # a range past 2^32
    for fn in (e.check_shaped_device, e.submit_shaped_device):
        refused(fn, [hdr[:4] + (2,)], I, P, n, W, X, n, N)                           # a table slot beyond the contexts
        refused(fn, [hdr], 0, P, n, W, X, n, N)                                      # null index bytes
        refused(fn, [hdr] * 65, I, P, n, W, X, n, N)                                 # too many shapes
    small = fam.engine(max_batch=32, workspaces=1)
    refused(small.submit_uniform_device, hdr, P, 33, W, X, n, N, engine_stream=True)  # a submit above max_batch
    refused(small.submit_list_device, hdr, 0, R, 33, W, 0, 0, X, n, N)
    # ... and the one workspace is back in the pool
    p = pairs[np.flatnonzero(shape_of == j)][:32]
    _same(_uniform(small, "engine", hdr, p), _host(small.check_uniform(hdr, p, now_us=NOW_US)), "after refusals")
    small.close()
    assert e.device_compact_stats() == s0 and e.stats()["batches"] == b0  # nothing ran


# ---- 9. in flight and ordering --------------------------------------------------------------------

def test_eight_in_flight_waited_in_reverse(nested):
    fam, e, shapes, shape_of, pairs = nested
    host = _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US))
    n = len(pairs)
    di, dp = _u8(shape_of), _u32(pairs)
    outs = [_Out(n, n) for _ in range(8)]
    torch.cuda.synchronize()
    s0 = e.device_compact_stats()
    bs = [e.submit_shaped_device(shapes, di.data_ptr(), dp.data_ptr(), n, engine_stream=True, now_us=NOW_US, **o.args())
          for o in outs]
    for b in reversed(bs):
        assert b.wait() == e.revision
    for k, o in enumerate(outs):
        _same(o.read(), host, k)
    assert e.device_compact_stats() == (s0[0] + 8, s0[1])
    # the compiled loops: uniform and range requests, 8 in flight
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    hu = _host(e.check_uniform(shapes[j], p, now_us=NOW_US))
    du = _u32(p)
    outs = [_Out(len(p), 4) for _ in range(12)]
    torch.cuda.synchronize()
    loop = e.prepare_uniform_device([shapes[j]] * 12, [du.data_ptr()] * 12, [len(p)] * 12,
                                    [o.words.data_ptr() for o in outs], [o.errs.data_ptr() for o in outs], 4, 8,
                                    n_errs=[o.cnt.data_ptr() for o in outs], now_us=NOW_US)
    assert loop.run() > 0
    for k, o in enumerate(outs):
        _same(o.read(), hu, ("loop", k))
    m = min(e.object_count(shapes[j][0]), 70)
    hr = _host(e.check_list(shapes[j], int(p[0, 1]), R, None, 0, m, now_us=NOW_US))
    outs = [_Out(m, 4, count=False) for _ in range(12)]  # (no count words: d_out_n_errs == NULL)
    torch.cuda.synchronize()
    loop = e.prepare_list_device([shapes[j]] * 12, [int(p[0, 1])] * 12, R, [0] * 12, [0] * 12, [m] * 12,
                                 [o.words.data_ptr() for o in outs], [o.errs.data_ptr() for o in outs], 4, 8,
                                 now_us=NOW_US)
    assert loop.run() > 0
    for k, o in enumerate(outs):
        _same(o.read(), hr, ("range loop", k))


def test_caller_stream_orders_producer_and_consumer(nested):
    fam, e, shapes, shape_of, pairs = nested
    j = _plain(shapes, shape_of)
    p = pairs[np.flatnonzero(shape_of == j)]
    n = len(p)
    host = _host(e.check_uniform(shapes[j], p, now_us=NOW_US))
    # the pairs arrive reversed and are put in order by a torch op on a non-default stream just
    # before the submit on that stream; the plane is read by a torch op on it after the wait
    src = _u32(p[::-1].copy()).reshape(n, 2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):
        out = _Out(n, n)
        d = torch.flip(src, dims=[0]).contiguous()
        b = e.submit_uniform_device(shapes[j], d.data_ptr(), n, stream=side.cuda_stream, now_us=NOW_US, **out.args())
        assert b.wait() == e.revision
        plane = out.words.clone()
    side.synchronize()
    assert np.array_equal(plane.cpu().numpy().view(np.uint64)[:out.nw], host[0])
    _same(out.read(), host, "caller stream")


def test_watch_batch_between_submit_and_wait():
    fam = _family("gdocs")
    e = fam.engine()
    shapes, shape_of, pairs = fam.request(e)
    n = len(pairs)
    before = _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US))
    # direct grants for checks of the request that are answered NO: the Watch batch turns them to HAS
    perm = E.unpack_results(before[0], n)
    denied = [c for c, p in zip(fam.checks, perm) if p == 1 and c.startswith("doc:") and "#view@user:u" in c
              and not c.endswith("*")][:5]
    assert denied
    grants = sorted({c.replace("#view@", "#viewer@") for c in denied})
    di, dp = _u8(shape_of), _u32(pairs)
    out = _Out(n, n)
    torch.cuda.synchronize()
    b = e.submit_shaped_device(shapes, di.data_ptr(), dp.data_ptr(), n, engine_stream=True, now_us=NOW_US, **out.args())
    e.apply_updates_text(2, "\n".join(f"CREATE {t}" for t in grants))
    assert e.revision == 2
    assert b.wait() == 1  # gck_check_wait_at: the revision the batch ran on
    _same(out.read(), before, "the snapshot at submit")
    after = _host(e.check_shaped(shapes, shape_of, pairs, now_us=NOW_US))
    assert not np.array_equal(after[0], before[0]), "the Watch batch changed no answer of the request"
    _same(_shaped(e, "engine", shapes, shape_of, pairs), after, "after the Watch batch")
    e.close()
