"""Listed user slots (gochugaru_amd/csrc/slot_pack.hpp): a user whose cover entries exceed a slot
has them sorted and deduplicated; if they fit then, its slot is an ordinary inline one, and if not it
carries 18 of them (13 at 32 bits) and the open range in which the omitted ones lie, and decides HAS
or NO from those where it can. Every answer must stay the oracle's, on every request format and
launch path, in the label join (which reads the same slots), and across Watch batches that move a
user between the slot kinds.

The graph: 4 top groups over 220 middle groups (a third of them over two leaf groups each), and 25
groups that share their two parents, so that their covers hold a duplicate entry. Users are in m
middle groups for m at each edge — 18-22 (the inline capacity of a listed slot, the slot's capacity
of 20, one above), 37-39 (a list twice a slot), 64 / 65 (the sorting bound) and 200 — picked three
ways: the first m, evenly spread (other groups lie between their entries, inside the window too)
and at random. There is a document per group, so some interval holds each inline entry, each
omitted entry, nothing inside the window, nothing between two inline entries, a childless group
(an interval that ends one past an entry, and one that begins at it), a top group (spans the
window, a root's whole tree); and documents with no group, 2-3, 4-7 (the second half of a resource
slot) and 8 (task rounds).

Both slot widths: the engine takes 32-bit entries only for a hierarchy of 2^24 groups or more and has
no switch to force them, so the GPU tests run at 24 bits; the packing at 32 bits is covered on the
host (tests/test_slot_pack.py)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from gochugaru_amd import engine as E
from tests import gen
from tests.helpers import oracle_for, parse_check, to_oracle_item

pytestmark = pytest.mark.gpu
NOW_US = gen.NOW_US
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEMA = """
definition user {}
definition group { relation member: user | group#member }
definition doc {
  relation owner: user
  relation viewer: group#member
  permission view = viewer
}
"""
N_MID, N_DUP = 220, 25
EDGES = (18, 19, 20, 21, 22, 37, 38, 39, 64, 65, 200)


def graph():
    rng = random.Random(5)
    t = []
    groups = [f"s{k}" for k in range(4)] + ["q1", "q2"]
    for i in range(N_MID):
        t.append(f"group:s{i // 55}#member@group:m{i}#member")
        groups.append(f"m{i}")
        if i % 3 == 0:
            for c in range(2):
                t.append(f"group:m{i}#member@group:l{i}_{c}#member")
                groups.append(f"l{i}_{c}")
    for i in range(N_DUP):  # two parents each: one of them is a non-tree parent, in every cover
        t.append(f"group:q1#member@group:x{i}#member")
        t.append(f"group:q2#member@group:x{i}#member")
        groups.append(f"x{i}")
    users = {}
    for m in EDGES:
        users[f"first{m}"] = [f"m{i}" for i in range(m)]
        users[f"even{m}"] = [f"m{(k * N_MID) // m}" for k in range(m)]
        users[f"rand{m}"] = [f"m{i}" for i in rng.sample(range(N_MID), m)]
    users["dup_fits"] = [f"x{i}" for i in range(15)]                 # 30 raw entries, 16 unique: inline
    users["dup_one_over"] = [f"x{i}" for i in range(20)]             # 40 raw, 21 unique: listed by one
    users["dup_mixed"] = [f"x{i}" for i in range(10)] + [f"m{7 * i}" for i in range(11)]  # 31 raw, 22 unique
    users["dup_leaf"] = [f"l{3 * i}_{i % 2}" for i in range(30)]     # leaves: 30 plain entries
    users["one"] = ["m100"]
    users["five"] = ["m3", "l30_1", "x2", "s3", "m219"]
    for u, gs in users.items():
        t += [f"group:{g}#member@user:{u}" for g in gs]
    docs = {}
    for g in groups:
        docs[f"d_{g}"] = [g]
    for k in (2, 3, 4, 5, 6, 7, 8):
        for r in range(6):
            docs[f"k{k}_{r}"] = rng.sample(groups, k)
    for d, gs in docs.items():
        t += [f"doc:{d}#viewer@group:{g}#member" for g in gs]
    t.append("doc:empty#owner@user:one")
    docs["empty"] = []
    return sorted(set(t)), sorted(users), sorted(docs), users


_CACHE = {}


def reference():
    """(tuples, users, docs, checks, want) — computed once, shared and left unchanged."""
    if not _CACHE:
        tuples, users, docs, _ = graph()
        checks = [f"doc:{d}#view@user:{u}" for u in users for d in docs]
        ck = oracle_for(SCHEMA, tuples, now=NOW_US / 1e6)
        want = [ck.check(to_oracle_item(parse_check(c))) for c in checks]
        assert all(x == 0 for _, x in want)
        _CACHE["ref"] = (tuples, users, docs, checks, np.array([p for p, _ in want], dtype=np.uint8))
    return _CACHE["ref"]


def engine(tuples, **kw):
    e = E.Engine(device=0, **kw)
    e.load_schema(SCHEMA)
    e.load_snapshot_text(1, "\n".join(tuples))
    return e


def header(e):
    t_r, t_s = e.type_id("doc"), e.type_id("user")
    return (t_r, e.relation_id(t_r, "view"), t_s, E.ELLIPSIS, 0)


def ids_of(e, users, docs):
    return (np.asarray(e.intern(e.type_id("user"), users), dtype=np.uint32),
            np.asarray(e.intern(e.type_id("doc"), docs), dtype=np.uint32))


def all_formats(e, users, docs, checks, want):
    """Items, uniform, cross and list requests over every (user, document): each the oracle's."""
    out = {}
    perm, err = e.check_bulk(e.make_items([parse_check(c) for c in checks]), now_us=NOW_US)
    assert not np.asarray(err).any()
    out["items"] = np.asarray(perm, dtype=np.uint8)
    hdr = header(e)
    uid, did = ids_of(e, users, docs)
    U, D = len(uid), len(did)
    pairs = np.stack([np.tile(did, U), np.repeat(uid, D)], axis=1)
    w, errs, _ = e.check_uniform(hdr, pairs, now_us=NOW_US)
    assert len(errs) == 0
    out["uniform"] = E.unpack_results(w, U * D)
    w, errs, _ = e.check_cross(hdr, uid, did, now_us=NOW_US)
    assert len(errs) == 0
    out["cross"] = E.unpack_cross(w, U, D).reshape(-1)
    by_user = []
    for u in uid:  # one user against every document
        w, errs, _ = e.check_list(hdr, int(u), E.VARY_RESOURCE, did, now_us=NOW_US)
        assert len(errs) == 0
        by_user.append(E.unpack_results(w, D))
    out["list_resources"] = np.concatenate(by_user)
    by_doc = []
    for d in did[::7]:  # one document against every user
        w, errs, _ = e.check_list(hdr, int(d), E.VARY_SUBJECT, uid, now_us=NOW_US)
        assert len(errs) == 0
        by_doc.append(E.unpack_results(w, U))
    got = np.stack(by_doc, axis=1).reshape(-1)
    assert np.array_equal(got, want.reshape(U, D)[:, ::7].reshape(-1)), "list_subjects"
    for name, got in out.items():
        bad = np.nonzero(np.asarray(got) != want)[0]
        assert bad.size == 0, (name, [(checks[i], int(want[i]), int(got[i])) for i in bad[:8]])


def test_every_format_matches_the_oracle():
    tuples, users, docs, checks, want = reference()
    assert set(want.tolist()) == {1, 2}
    e = engine(tuples)
    # only the documents with 8 groups leave the slots (for the task rounds): no listed user has
    # become an overflowing one, and no check is left to the bundles
    n_viewers = {d: sum(1 for t in tuples if t.startswith(f"doc:{d}#viewer@")) for d in docs}
    n_slot = sum(1 for u in users for d in docs if n_viewers[d] <= 7)
    assert 0 < len(checks) - n_slot < 0.05 * len(checks)
    e.reset_stats()
    e.check_bulk(e.make_items([parse_check(c) for c in checks]), now_us=NOW_US)
    st = e.stats()
    assert st["slot_checks"] == n_slot and st["closure_checks"] == len(checks), st
    all_formats(e, users, docs, checks, want)
    assert e.stats()["aql_batches"] > 0, e.stats()
    e.close()


_CHILD = """
import json, sys
sys.path.insert(0, {root!r})
from tests import test_gpu_slot_window as T
tuples, users, docs, checks, want = T.reference()
e = T.engine(tuples)
T.all_formats(e, users, docs, checks, want)
print(json.dumps({{"aql": int(e.stats()["aql_batches"]), "slot": int(e.stats()["slot_checks"])}}))
"""


def test_without_aql():
    """GCK_AQL=0 (read once per process: a child): the joins launched through HIP."""
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GCK_AQL="0"))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["aql"] == 0 and out["slot"] > 0, out


def test_resident_launch():
    import torch

    tuples, users, docs, checks, want = reference()
    e = engine(tuples, resident=True, workspaces=8)
    e.reset_stats()
    items = torch.from_numpy(e.make_items([parse_check(c) for c in checks]).view(np.uint8).copy()).cuda()
    perm = torch.zeros(len(checks), dtype=torch.uint8, device="cuda")
    err = torch.zeros(len(checks), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e.submit(items.data_ptr(), len(checks), perm.data_ptr(), err.data_ptr(), device=True, engine_stream=True,
             now_us=NOW_US).wait()
    got = perm.cpu().numpy()
    assert not err.cpu().numpy().any()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(checks[i], int(want[i]), int(got[i])) for i in bad[:8]]
    assert e.stats()["resident_batches"] > 0, e.stats()
    e.close()


def test_label_join_reads_listed_slots():
    """A config-2-shaped schema (folders, viewers and editors through groups): the label join's
    subjects include listed users of every kind, and its answers stay the oracle's."""
    tuples, users, docs, _ = graph()
    rng = random.Random(9)
    t = [x for x in tuples if x.startswith("group:")]
    groups = sorted({x.split("#")[0][6:] for x in t})
    for f in range(1, 6):
        t.append(f"folder:f{f}#parent@folder:f{f - 1}")
    for f in range(6):
        t.append(f"folder:f{f}#viewer@group:{rng.choice(groups)}#member")
        t.append(f"folder:f{f}#editor@user:{rng.choice(users)}")
    names = []
    for i, g in enumerate(groups[::3]):
        d = f"d{i}"
        names.append(d)
        t.append(f"doc:{d}#parent@folder:f{rng.randrange(6)}")
        t.append(f"doc:{d}#owner@user:{rng.choice(users)}")
        t.append(f"doc:{d}#{rng.choice(['viewer', 'editor'])}@group:{g}#member")
    checks = [f"doc:{d}#{p}@user:{u}" for u in users for d in names for p in ("view", "edit")]
    ck = oracle_for(gen.GDOCS, t, now=NOW_US / 1e6)
    want = [ck.check(to_oracle_item(parse_check(c))) for c in checks]
    e = E.Engine(device=0)
    e.load_schema(gen.GDOCS)
    e.load_snapshot_text(1, "\n".join(sorted(set(t))))
    e.reset_stats()
    perm, err = e.check_bulk(e.make_items([parse_check(c) for c in checks]), now_us=NOW_US)
    got = [(int(p), int(x)) for p, x in zip(perm, err)]
    bad = [(c, w, g) for c, w, g in zip(checks, want, got) if tuple(w) != g]
    assert not bad, bad[:8]
    st = e.stats()
    assert st["label_checks"] > 0.9 * len(checks), st
    e.close()


def test_watch_moves_a_user_between_slot_kinds():
    """Updates of a user's memberships only (the hierarchy keeps its labels: the batch rebuilds
    that user's slot alone): 20 entries inline -> 21, listed -> back; and with shared-parent groups
    19 raw -> 21 raw but 20 unique, inline through the duplicates only -> 21 unique, listed -> back.
    Checks against every document before and after each publication."""
    tuples, _, docs, _ = graph()
    store = set(tuples)
    store |= {f"group:m{2 * i}#member@user:w_plain" for i in range(20)}
    store |= {f"group:m{3 * i + 1}#member@user:w_dup" for i in range(17)} | {"group:x0#member@user:w_dup"}
    e = engine(sorted(store))
    checks = [f"doc:{d}#view@user:{u}" for u in ("w_plain", "w_dup", "even21", "dup_one_over") for d in docs]
    items = e.make_items([parse_check(c) for c in checks])

    def verify(step):
        ck = oracle_for(SCHEMA, sorted(store), now=NOW_US / 1e6)
        want = [ck.check(to_oracle_item(parse_check(c))) for c in checks]
        perm, err = e.check_bulk(items, now_us=NOW_US)
        got = [(int(p), int(x)) for p, x in zip(perm, err)]
        bad = [(c, w, g) for c, w, g in zip(checks, want, got) if tuple(w) != g]
        assert not bad, (step, bad[:8])

    verify(0)
    steps = [
        [("CREATE", "group:m101#member@user:w_plain")],                    # 20 -> 21 unique: listed
        [("DELETE", "group:m101#member@user:w_plain")],                    # and back: inline
        [("CREATE", "group:x1#member@user:w_dup")],                        # 19 raw -> 21 raw, 20 unique: inline
        [("CREATE", "group:x2#member@user:w_dup")],                        # 23 raw, 21 unique: listed
        [("DELETE", "group:x1#member@user:w_dup"), ("DELETE", "group:m1#member@user:w_dup")],  # 20 raw: inline
        [("CREATE", "group:m1#member@user:w_dup"), ("CREATE", "group:x1#member@user:w_dup"),
         ("CREATE", "group:m5#member@user:w_plain"), ("CREATE", "group:m7#member@user:w_plain")],
    ]
    for k, ups in enumerate(steps):
        for op, line in ups:
            (store.add if op == "CREATE" else store.discard)(line)
        e.apply_updates_text(2 + k, "\n".join(f"{op} {line}" for op, line in ups))
        verify(1 + k)
    e.close()


_PHASES = """
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tools")
import numpy as np
import analyze_cj
from tests import test_gpu_slot_window as T
from tests.helpers import parse_check
tuples, _, _, _ = T.graph()
e = T.engine(tuples)
checks = json.load(open({checks!r}))
perm, err = e.check_bulk(e.make_items([parse_check(c) for c in checks]), now_us=T.NOW_US)
names = T.group_names(tuples)
ids = [int(x) for x in e.intern(e.type_id("group"), names)]
e.close()
recs = [r[r[:, 0] > 0] for r in analyze_cj.launches({prefix!r} + "_cj.bin")]
print(json.dumps({{"n_list": [(r[:, 7] >> 32).tolist() for r in recs], "n_take": [(r[:, 7] & 0xFFFFFFFF).tolist() for r in recs],
                  "list_round": analyze_cj.list_round(recs), "group_ids": dict(zip(names, ids))}}))
"""


def group_names(tuples):
    """Every group a tuple names, on either side."""
    return sorted({t.split("#")[0][6:] for t in tuples if t.startswith("group:")} |
                  {t.split("@group:")[1].split("#")[0] for t in tuples if "@group:" in t})


def host_labels(tuples, gid):
    """The hierarchy's tree labels and covers as the engine builds them: the tree parent
    is the parent with the smallest id, roots and children are numbered in id order, and a group's
    cover is itself and its parents' covers without the tree ancestors of other entries. Returns
    pre, end and cover (preorder numbers) by group name."""
    parents = {g: [] for g in gid}
    for t in tuples:
        if t.startswith("group:") and "@group:" in t:
            parents[t.split("@group:")[1].split("#")[0]].append(t.split("#")[0][6:])
    tpar = {g: min(ps, key=gid.get) if ps else None for g, ps in parents.items()}
    kids = {g: [] for g in gid}
    for g in sorted(gid, key=gid.get):
        if tpar[g] is not None:
            kids[tpar[g]].append(g)
    pre, end = {}, {}

    def number(g, at):
        pre[g] = at
        at += 1
        for c in kids[g]:
            at = number(c, at)
        end[g] = at
        return at

    at = 0
    for g in sorted(gid, key=gid.get):
        if tpar[g] is None:
            at = number(g, at)
    cover = {}

    def cover_of(g):  # (as group names)
        if g not in cover:
            ent = {g}.union(*[cover_of(p) for p in parents[g]])
            cover[g] = {a for a in ent if not any(b != a and pre[a] <= pre[b] < end[a] for b in ent)}
        return cover[g]

    for g in gid:
        cover_of(g)
    cover = {g: sorted(pre[a] for a in c) for g, c in cover.items()}
    return pre, end, cover


def test_phase_dump_reports_the_list_round(tmp_path):
    """The timing build (libgck_timing.so, which build() makes beside the engine) records per wave
    how many of its checks go into the cover-list round, and tools/analyze_cj.py reports the share
    of waves and of checks. Expected, per wave, from the same graph on the host: the engine's group
    ids give the tree labels and covers (host_labels), each user's raw entries are packed by the
    code the kernels run (gck_test_slot_pack) and the slot round's rule (tests/test_slot_pack.py
    decide) says whether the check is left to the list — for every kind of user: inline, inline
    after deduplication, listed with a window, plain lists. Documents with 8 groups leave the
    slots for the task rounds. (The dump holds the first ceil(n / 64) waves of a batch: of 32
    checks each, the first half of the batch.)"""
    from tests import test_slot_pack as P

    timing_lib = os.path.join(ROOT, "gochugaru_amd", "libgck_timing.so")
    assert os.path.exists(timing_lib), "libgck_timing.so is missing: build() makes it (make -C gochugaru_amd/csrc TIMING=1)"
    tuples, users, docs, members = graph()
    viewers = {d: [t.split("@group:")[1].split("#")[0] for t in tuples if t.startswith(f"doc:{d}#viewer@")] for d in docs}
    inline = [u for u in users if len(members[u]) <= 20 and not u.startswith("dup")]
    # (every user with every other block of 8 documents, the inline ones alone with the rest: waves with and without)
    pairs = [(d, u) for k, d in enumerate(docs) for u in (users if (k // 8) % 2 == 0 else inline)]
    checks = [f"doc:{d}#view@user:{u}" for d, u in pairs]
    n = len(checks)
    n_rec = (n + 63) // 64
    (tmp_path / "checks.json").write_text(json.dumps(checks))
    r = subprocess.run([sys.executable, "-c", _PHASES.format(root=ROOT, checks=str(tmp_path / "checks.json"),
                                                             prefix=str(tmp_path / "t"))],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GCK_LIBRARY=timing_lib, GCK_DEBUG_TIMING=str(tmp_path / "t")))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    pre, end, cover = host_labels(tuples, out["group_ids"])
    lib = E.load_library()
    lib.gck_test_slot_pack.restype = C.c_int
    lib.gck_test_slot_pack.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    slots, kinds = {}, {}
    for u in users:
        raw = [x for g in members[u] for x in cover[g]]
        if len(raw) <= 20:
            slots[u], kinds[u] = None, "inline"
            continue
        m, w = P.pack(lib, 24, raw, 0)
        slots[u] = w if int(w[0]) & P.LIST else None
        kinds[u] = "deduplicated" if slots[u] is None else "plain" if len(raw) > 64 else "window"
    assert {k: sum(1 for v in kinds.values() if v == k) for k in ("inline", "deduplicated", "window", "plain")} == \
        {"inline": 11, "deduplicated": 1, "window": 21, "plain": 6}, kinds
    listed = np.array([slots[u] is not None and 1 <= len(viewers[d]) <= 7 and
                       P.decide(24, slots[u], [(pre[g], end[g]) for g in viewers[d]]) == 3 for d, u in pairs])
    window = np.array([kinds[u] == "window" and 1 <= len(viewers[d]) <= 7 for d, u in pairs])
    # the window rule keeps most of the windowed users' checks out of the round, and not all
    assert 0 < (listed & window).sum() < 0.5 * window.sum(), ((listed & window).sum(), window.sum())
    head = np.zeros(n_rec * 32, dtype=bool)
    head[:min(n, n_rec * 32)] = listed[:n_rec * 32]
    want = head.reshape(n_rec, 32).sum(axis=1)
    assert 0.1 < float((want > 0).mean()) < 0.9  # (at least a tenth of the waves of either kind)
    assert len(out["n_list"]) == 1 and out["n_list"][0] == want.tolist(), \
        [(k, a, b) for k, (a, b) in enumerate(zip(out["n_list"][0], want.tolist())) if a != b][:10]
    assert sum(out["n_take"][0]) == min(n, n_rec * 32)
    assert out["list_round"][0] == pytest.approx(float((want > 0).mean()))
    assert out["list_round"][1] == pytest.approx(float(want.sum() / min(n, n_rec * 32)))
    assert out["list_round"][2] >= 0.0 and out["list_round"][3] >= 0.0  # (the lists phase's medians, us)
