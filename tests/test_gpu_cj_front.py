"""Resource fronts of the closure join (gochugaru_amd/csrc/slot_pack.hpp front_pack; closure.inc
cj_block): at 24 bits a check reads its document's 16-B front instead of half its 64-B slot, and
only a flagged front — more than 3 viewer groups, a group whose subtree is longer than 2^18 - 1
labels, an overflow slot — sends the lane to the slot. Every answer must stay the oracle's and stay,
bit for bit, what the join without fronts gives (GCK_DEBUG_CJ_FRONT=0, a switch of the debug builds),
through AQL and through HIP launches, across a Watch batch that moves a document over the 3-group
edge, and on a 32-bit snapshot, which has no fronts.

The graph: 4 top groups over 40 small ones, and one group `big` over 512 groups of 512 leaves each —
262,657 labels, one more level than a length of 18 bits holds (a label is a group: such a subtree
takes that many tuples, and nothing smaller reaches the long-interval flag on the device).
Documents have 0, 1, 2, 3, 4 and 8 viewer groups; `dbig` is viewed by `big` alone (one interval,
too long), `dbig3` by `big` and two small groups, `dsub` by one of big's children (513 labels:
packs). The oracle walks big's whole subtree for every check of big's documents, so only a few
checks name them, and the batch sizes, launch paths and the join without fronts are crossed on the
graph without `big` (a few hundred tuples; its flagged fronts are the documents with 4 and 8 groups)."""
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
TIMING_LIB = os.path.join(ROOT, "gochugaru_amd", "libgck_timing.so")  # the switches, per-wave records, HIP launches only
DEBUG_LIB = os.path.join(ROOT, "gochugaru_amd", "libgck_debug.so")    # the switches over the product kernels: AQL
BATCHES = (1, 31, 32, 33, 64, 1000)

SCHEMA = """
definition user {}
definition group { relation member: user | group#member }
definition doc {
  relation owner: user
  relation viewer: group#member
  permission view = viewer
}
"""
N_BIG = 512


def small_graph():
    """(tuples, users, docs: name -> viewer groups) without `big`."""
    rng = random.Random(11)
    t = [f"group:t{i // 10}#member@group:m{i}#member" for i in range(40)]
    small = [f"m{i}" for i in range(40)] + [f"t{i}" for i in range(4)]
    users = {f"s{k}": [f"m{3 * k}", f"m{3 * k + 1}"] for k in range(12)}
    users["top"] = ["t2"]
    users["lone"] = ["m39"]
    docs = {"v0": []}
    for k in (1, 2, 3, 4, 8):
        for r in range(4):
            docs[f"v{k}_{r}"] = rng.sample(small, k)
    for u, gs in users.items():
        t += [f"group:{g}#member@user:{u}" for g in gs]
    t.append("doc:v0#owner@user:top")
    return t, users, docs


def graph():
    t, users, docs = small_graph()
    for i in range(N_BIG):
        t.append(f"group:big#member@group:b{i}#member")
        t += [f"group:b{i}#member@group:l{i}_{j}#member" for j in range(N_BIG)]
    users.update({"leaf": ["l7_3"], "mid": ["b100"], "bigtop": ["big"], "both": ["l500_511", "m5"]})
    for u in ("leaf", "mid", "bigtop", "both"):
        t += [f"group:{g}#member@user:{u}" for g in users[u]]
    docs.update({"dbig": ["big"], "dbig3": ["big", "m5", "t1"], "dsub": ["b7"]})
    for d, gs in docs.items():
        t += [f"doc:{d}#viewer@group:{g}#member" for g in gs]
    return sorted(set(t)), sorted(users), docs


_CACHE = {}
BIGS = ("dbig", "dbig3", "dsub")


def cases(big):
    """(tuples, 1,000 checks) of the graph with or without `big`: every user against every small
    document and, with `big`, six checks of its documents; shuffled, so that flagged and packed
    fronts share waves, and repeated to the largest batch. No oracle: a child process calls it too."""
    if big:
        tuples, users, docs = graph()
    else:
        t, users, docs = small_graph()
        for d, gs in docs.items():
            t += [f"doc:{d}#viewer@group:{g}#member" for g in gs]
        tuples, users = sorted(set(t)), sorted(users)
    base = [f"doc:{d}#view@user:{u}" for u in users for d in docs if d not in BIGS]
    if big:
        base += [f"doc:{d}#view@user:{u}" for d, u in (("dbig", "leaf"), ("dbig", "s1"), ("dbig3", "mid"), ("dbig3", "top"),
                                                      ("dbig3", "both"), ("dsub", "leaf"))]
    random.Random(3).shuffle(base)
    return tuples, [base[k % len(base)] for k in range(max(BATCHES))]


def fast_store(tuples):
    """The oracle's tuple store, filled without TupleStore.add's scan for an earlier relationship of
    the same subject (quadratic in a group's members; the tuples here are distinct)."""
    from oracle import spicedb_ref as ref

    st = ref.TupleStore()
    for line in tuples:
        t = ref.parse_tuple(line)
        st.index.setdefault((t.resource_type, t.resource_id, t.relation), []).append(t)
        st.count += 1
    return st


def reference(big):
    """(tuples, checks, the oracle's perm) — computed once, shared and left unchanged."""
    if big not in _CACHE:
        from oracle import spicedb_ref as ref

        tuples, checks = cases(big)
        ck = ref.Checker(ref.Schema(SCHEMA), fast_store(tuples), now=NOW_US / 1e6)
        memo = {c: ck.check(to_oracle_item(parse_check(c))) for c in set(checks)}
        assert all(x == 0 for _, x in memo.values())
        want = np.array([memo[c][0] for c in checks], dtype=np.uint8)
        assert set(want.tolist()) == {1, 2}
        _CACHE[big] = (tuples, checks, want)
    return _CACHE[big]


def engine(tuples):
    e = E.Engine(device=0)
    e.load_schema(SCHEMA)
    e.load_snapshot_text(1, "\n".join(tuples))
    return e


def run_batches(e, checks, batches=BATCHES):
    """[perm, err] of the first n checks, for every n of batches, as lists."""
    items = e.make_items([parse_check(c) for c in checks])
    out = []
    for n in batches:
        perm, err = e.check_bulk(items[:n], now_us=NOW_US)
        out.append([np.asarray(perm, dtype=np.uint8).tolist(), np.asarray(err, dtype=np.int32).tolist()])
    return out


def verify(out, want, batches=BATCHES):
    for n, (perm, err) in zip(batches, out):
        assert not any(err), (n, err[:8])
        bad = [k for k in range(n) if perm[k] != want[k]]
        assert not bad, (n, bad[:8])


def want_flags(checks, batches=BATCHES):
    """Per batch, the checks whose front says "read the slot" among those the timing dump holds: the
    first ceil(n / 64) waves of a batch, of 32 checks each."""
    flagged = [c.split("#")[0][4:].split("_")[0] in ("v4", "v8", "dbig", "dbig3") for c in checks]
    return [sum(flagged[:min(n, 32 * ((n + 63) // 64))]) for n in batches]


_CHILD = """
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tools")
import analyze_cj
from tests import test_gpu_cj_front as T
tuples, checks = T.cases({big!r})
e = T.engine(tuples)
e.reset_stats()
out = T.run_batches(e, checks, {batches!r})
st = e.stats()
e.close()
flags = None
if {timed!r}:
    flags = [int(r[r[:, 0] > 0][:, 11].sum()) for r in analyze_cj.launches({prefix!r} + "_cj.bin")]
print(json.dumps({{"out": out, "aql": int(st["aql_batches"]), "slot": int(st["slot_checks"]), "flags": flags}}))
"""


def child(env, prefix, big=False, batches=BATCHES, timed=True):
    """The batches in a process of its own through a build that reads the debug switches: results and
    launch path; timed, the timing build (HIP launches) and the flagged fronts its per-wave records
    count, otherwise the debug build (the product kernels, dispatched through AQL)."""
    lib = TIMING_LIB if timed else DEBUG_LIB
    assert os.path.exists(lib), lib + " is missing: build() makes it (make -C gochugaru_amd/csrc TIMING=1 / DEBUG=1)"
    code = _CHILD.format(root=ROOT, big=big, prefix=str(prefix), batches=tuple(batches), timed=timed)
    full = dict(os.environ, GCK_LIBRARY=lib, **env)
    if timed:
        full["GCK_DEBUG_TIMING"] = str(prefix)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=full)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_fronts_match_the_oracle():
    tuples, checks, want = reference(False)
    e = engine(tuples)
    e.reset_stats()
    out = run_batches(e, checks)
    verify(out, want)
    st = e.stats()
    assert st["aql_batches"] > 0 and st["slot_checks"] > 0, st
    e.close()
    _CACHE["product"] = out


@pytest.mark.parametrize("aql", ["1", "0"])
def test_fronts_equal_the_join_without_them(aql, tmp_path):
    """The same batches with fronts and without (GCK_DEBUG_CJ_FRONT=0), through AQL and through HIP
    launches (GCK_AQL=0): the oracle's, and bit for bit each other's and the product library's. The
    HIP runs' per-wave records say that fronts were read: flagged lanes with them, exactly the
    checks of documents with 4 and 8 groups, and none without."""
    tuples, checks, want = reference(False)
    timed = aql == "0"  # (the timing build launches through HIP only)
    off = child({"GCK_DEBUG_CJ_FRONT": "0", "GCK_AQL": aql}, tmp_path / "off", timed=timed)
    on = child({"GCK_AQL": aql}, tmp_path / "on", timed=timed)
    for o in (off, on):
        verify(o["out"], want)
        assert (o["aql"] > 0) == (aql == "1") and o["slot"] > 0, (o["aql"], o["slot"])
    assert on["out"] == off["out"]
    if "product" in _CACHE:
        assert _CACHE["product"] == on["out"]
    if timed:
        assert sum(off["flags"]) == 0, off["flags"]
        wf = want_flags(checks)
        assert on["flags"] == wf and min(wf[1:]) > 0, (on["flags"], wf)


def test_a_subtree_longer_than_18_bits(tmp_path):
    """`big` (262,657 labels): the fronts of dbig and dbig3 are flagged by the length alone, dsub's
    packs; answers from the oracle, HAS and NO through each, equal with and without fronts."""
    tuples, checks, want = reference(True)
    batches = (33, 1000)
    e = engine(tuples)
    out = run_batches(e, checks, batches)
    verify(out, want, batches)
    e.close()
    off = child({"GCK_DEBUG_CJ_FRONT": "0"}, tmp_path / "off", big=True, batches=batches)
    on = child({}, tmp_path / "on", big=True, batches=batches)
    assert out == on["out"] == off["out"]
    wf = want_flags(checks, batches)
    assert on["flags"] == wf and sum(off["flags"]) == 0, (on["flags"], wf, off["flags"])
    # (dbig and dbig3 are flagged by their length alone: counted in wf, and the dump's 512 checks hold some)
    assert sum(1 for c in checks[:512] if c.split("#")[0][4:] in ("dbig", "dbig3")) > 0


def test_32_bit_snapshot_has_no_fronts(tmp_path):
    """GCK_DEBUG_SLOT_BITS=32 (timing build) gives the graph the 32-bit layout and kernels: no entry
    has a front pointer, so no wave records a flagged front although documents with 4 and 8 groups
    are checked, and the answers are the oracle's and those of the 24-bit snapshot."""
    tuples, checks, want = reference(False)
    wide = child({"GCK_DEBUG_SLOT_BITS": "32"}, tmp_path / "w")
    verify(wide["out"], want)
    assert wide["slot"] > 0 and sum(wide["flags"]) == 0, (wide["slot"], wide["flags"])
    e = engine(tuples)
    assert run_batches(e, checks) == wide["out"]
    e.close()


def test_watch_moves_a_document_over_the_three_group_edge():
    """3 -> 4 -> 3 viewer groups across two Watch batches: the batch rebuilds the document's slot
    and, in the same publication, its front (packed -> flagged -> packed). Checks of every user
    against the document and its neighbours before, between and after."""
    t, users, docs = small_graph()
    docs["w"] = ["m0", "m13", "t3"]
    for d, gs in docs.items():
        t += [f"doc:{d}#viewer@group:{g}#member" for g in gs]
    store = set(t)
    e = engine(sorted(store))
    checks = [f"doc:{d}#view@user:{u}" for u in sorted(users) for d in ("w", "v3_0", "v4_0", "v0")]
    items = e.make_items([parse_check(c) for c in checks])

    def check(step):
        ck = oracle_for(SCHEMA, sorted(store), now=NOW_US / 1e6)
        want = [ck.check(to_oracle_item(parse_check(c))) for c in checks]
        perm, err = e.check_bulk(items, now_us=NOW_US)
        got = [(int(p), int(x)) for p, x in zip(perm, err)]
        bad = [(c, w, g) for c, w, g in zip(checks, want, got) if tuple(w) != g]
        assert not bad, (step, bad[:8])
        return [p for p, _ in got]

    before = check(0)
    store.add("doc:w#viewer@group:m22#member")  # s7 is in m21 and m22: NO -> HAS
    e.apply_updates_text(2, "CREATE doc:w#viewer@group:m22#member")
    between = check(1)
    assert between != before
    store.discard("doc:w#viewer@group:m22#member")
    e.apply_updates_text(3, "DELETE doc:w#viewer@group:m22#member")
    assert check(2) == before
    e.close()
