"""The closure join's reordered arguments (closure.inc CjArgs: one hot 64-B kernarg line, a mode
word for the null tests of `pairs` and `bad_slot`, cold fields read inside their branches), its
16-B table copy and its rare-path arrays inside the wave's stage region.

A config-4 graph of about 1e5 tuples (tests/synth.build) with rows added by hand, every answer
compared with the C oracle on the same CSR arrays:

* a user who is a direct member of 30 leaf groups: 30 covers exceed a slot's 20 entries, so only
  the list round can decide its checks from the slots;
* a document with 5 viewer groups (the second half of its resource slot), one with 8 (more than a
  slot's 7 intervals: the task rounds) and one with 9 (more than the task rounds take: deferred);
* a check of another shape, doc#view@group:g (a group object as a plain subject): deferred.

Each batch runs once on the engine's stream (dispatched into the engine's HSA queue) and once on
the caller's stream (a HIP launch): both fill the same struct."""
import numpy as np
import pytest
import torch

from gochugaru_amd import engine as E
from oracle import corc
from tests import synth
from tests.test_gpu_scale import load_engine
from tests.test_synth import _oracle

pytestmark = pytest.mark.gpu

N_LIST_GROUPS = 30  # > 20, the entries of a 24-bit user slot (closure.inc slot_cap)
SIZES = [1, 31, 32, 33, 127, 128, 129, 1000]  # partial waves (32 checks) and partial blocks (128)


def _item(doc, sub, stype=synth.T_USER):
    return (synth.T_DOC, synth.R_VIEW, doc, stype, synth.ELLIPSIS, sub, 0)


def _graph():
    G = synth.build(1e5, device="cuda")
    H = synth.host_arrays(G)
    rng = np.random.default_rng(5)
    n_groups = G.n_groups
    ls = G.layer_start.cpu().numpy()
    # the list-round user: a new id (the largest, so it lands at the end of each row it joins)
    u_list = G.n_users
    leaf = rng.choice(np.arange(ls[-2], ls[-1]), N_LIST_GROUPS, replace=False)
    off = H["mem_user_off"].astype(np.int64)
    rows = np.repeat(np.arange(n_groups), np.diff(off))
    key = np.concatenate([rows * (u_list + 1) + H["mem_user_nbr"].astype(np.int64), leaf * (u_list + 1) + u_list])
    key.sort()
    mu_rows, mu_nbr = key // (u_list + 1), key % (u_list + 1)
    mu_off = np.concatenate([[0], np.cumsum(np.bincount(mu_rows, minlength=n_groups))])
    # parent of the first leaf group: a viewer group through which the list user HAS view
    goff = H["mem_group_off"].astype(np.int64)
    parent = np.repeat(np.arange(n_groups), np.diff(goff))[np.flatnonzero(H["mem_group_nbr"] == leaf[0])[0]]
    # new documents: 2 viewer groups (one above the list user), 5, 8 and 9 viewer groups
    d_up, d5, d8, d9 = (G.n_docs + k for k in range(4))
    new_rows = []
    for k, base in ((2, [parent]), (5, [parent]), (8, []), (9, [])):
        others = rng.choice(np.setdiff1d(np.arange(n_groups), base), k - len(base), replace=False)
        new_rows.append(np.sort(np.concatenate([np.array(base, dtype=np.int64), others])))
    v_nbr = np.concatenate([H["viewer_nbr"].astype(np.int64)] + new_rows)
    v_off = np.concatenate([H["viewer_off"].astype(np.int64), H["viewer_off"][-1] + np.cumsum([len(r) for r in new_rows])])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64)).to(dt).cuda()
    G2 = synth.Graph(G.n_users + 1, n_groups, G.n_docs + 4, G.layer_start,
                     t(mu_off, torch.int64), t(mu_nbr, torch.int32), G.mem_group_off, G.mem_group_nbr,
                     t(v_off, torch.int64), t(v_nbr, torch.int32))
    # a direct member of one viewer group of each new document (HAS) and the users before them
    member = lambda d: int(mu_nbr[mu_off[new_rows[d - d_up][-1]]])
    special = {
        "list": [_item(d_up, u_list), _item(int(rng.integers(0, G.n_docs)), u_list), _item(int(rng.integers(0, G.n_docs)), u_list)],
        "half2": [_item(d5, member(d5)), _item(d5, 3), _item(d5, u_list)],
        "tasks": [_item(d8, member(d8)), _item(d8, 7), _item(d8, u_list)],
        "deferred": [_item(d9, member(d9)), _item(d9, 11), _item(d_up, int(parent), stype=synth.T_GROUP)],
    }
    return G2, special


@pytest.fixture(scope="module")
def world():
    G, special = _graph()
    e = load_engine(G, workspaces=2)
    _, prog, tab = _oracle(G)
    rand = synth.checks(G, 1000, seed=31).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
    spec = np.array([it for k in ("list", "half2", "tasks", "deferred") for it in special[k]], dtype=E.ITEM_DTYPE)
    oracle = lambda items: corc.check(prog, tab, np.ascontiguousarray(items).view(corc.ITEM_DTYPE), threads=4)[:2]
    yield {"e": e, "G": G, "special": special, "rand": rand, "spec": spec, "oracle": oracle,
           "want_rand": oracle(rand), "want_spec": oracle(spec)}
    e.close()


def _run(e, items, engine_stream, offset=0):
    """One device batch; the items start `offset` bytes into their (16-B aligned) buffer."""
    n = len(items)
    raw = np.ascontiguousarray(items).view(np.uint8)
    buf = torch.zeros(offset + raw.size + 16, dtype=torch.uint8, device="cuda")
    buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    perm = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    err = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    if engine_stream:
        e.submit(buf.data_ptr() + offset, n, perm.data_ptr(), err.data_ptr(), device=True, engine_stream=True).wait()
    else:
        e.check_bulk_device(buf.data_ptr() + offset, n, perm.data_ptr(), err.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return perm.cpu().numpy(), err.cpu().numpy()


def _settle(world):
    """A batch whose join left checks makes the engine chain the bundle stages behind the next 16
    joins through HIP: 16 clean batches, so that an engine-stream batch goes into the HSA queue."""
    for _ in range(16):
        _run(world["e"], world["rand"][:32], False)


@pytest.mark.parametrize("engine_stream", [True, False], ids=["engine-stream", "caller-stream"])
@pytest.mark.parametrize("offset", [0, 20], ids=["aligned", "offset20"])
def test_batch_sizes_match_the_oracle(world, engine_stream, offset):
    e = world["e"]
    wp, we = world["want_rand"]
    assert set(np.unique(wp)) == {1, 2}
    _settle(world)
    e.reset_stats()
    for n in SIZES:
        perm, err = _run(e, world["rand"][:n], engine_stream, offset)
        assert np.array_equal(err, we[:n]), n
        assert np.array_equal(perm, wp[:n]), (n, np.flatnonzero(perm != wp[:n])[:10])
    st = e.stats()
    assert st["closure_checks"] == sum(SIZES) and st["label_checks"] == 0, st
    assert (st["aql_batches"] > 0) == engine_stream, st["aql_batches"]


def test_uniform_request_of_33(world):
    e = world["e"]
    items = world["rand"][:33]
    wp, we = world["want_rand"]
    pairs = np.stack([items["resource_id"], items["subject_id"]], axis=1).astype(np.uint32)
    e.reset_stats()
    words, errs, _ = e.check_uniform((synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS), pairs)
    assert E.unpack_results(words, 33).tolist() == wp[:33].tolist() and len(errs) == 0
    assert e.stats()["closure_checks"] == 33
    # ... and one whose checks the join leaves to the bundle stages (their items written for them)
    d9 = world["special"]["deferred"][0][2]
    pairs[:, 0] = d9
    want = world["oracle"](np.array([_item(d9, int(u)) for u in pairs[:, 1]], dtype=E.ITEM_DTYPE))[0]
    words, errs, _ = e.check_uniform((synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS), pairs)
    assert E.unpack_results(words, 33).tolist() == want.tolist() and len(errs) == 0


@pytest.mark.parametrize("engine_stream", [True, False], ids=["engine-stream", "caller-stream"])
def test_every_path_of_the_join(world, engine_stream):
    """The hand-built rows alone, so that the counters tell which path took each check; then
    mixed into a batch of ordinary checks."""
    e, sp = world["e"], world["special"]
    wp, we = world["want_spec"]
    assert 2 in wp[:3] and 1 in wp[:3]  # the list user HAS view through its leaf group's parent
    assert wp[3] == 2 and wp[6] == 2 and wp[9] == 2  # the direct members
    _settle(world)
    e.reset_stats()
    perm, err = _run(e, world["spec"], engine_stream)
    assert np.array_equal(err, we) and np.array_equal(perm, wp), (perm, wp)
    st = e.stats()
    n = len(world["spec"])
    n_def, n_task = len(sp["deferred"]), len(sp["tasks"])
    assert n - st["closure_checks"] == n_def, st        # left to the bundle stages
    assert st["closure_checks"] - st["slot_checks"] == n_task, st  # the task rounds
    assert st["slot_checks"] == len(sp["list"]) + len(sp["half2"]), st  # the slots, lists included
    if engine_stream:
        assert st["aql_batches"] == 1, st
    mixed = np.concatenate([world["rand"][:150], world["spec"], world["rand"][150:333]])
    perm, err = _run(e, mixed, engine_stream)
    want_p = np.concatenate([world["want_rand"][0][:150], wp, world["want_rand"][0][150:333]])
    assert np.all(err == 0) and np.array_equal(perm, want_p), np.flatnonzero(perm != want_p)[:10]


def test_zero_copy_batch_reports_the_bad_context_slot(world):
    e = world["e"]
    n, bad_at = 300, 171
    items = e.host_array(n, E.ITEM_DTYPE)
    items[:] = world["rand"][:n]
    items[bad_at]["context_slot"] = 1
    items[n - 1]["context_slot"] = 4  # (a later offender: the first one is reported)
    pp, pe = e.host_array(n, np.uint8), e.host_array(n, np.int32)
    _settle(world)
    e.reset_stats()
    with pytest.raises(E.GckError) as ei:
        e.submit_into(items, pp, pe).wait()
    assert ei.value.code == E.GCK_E_INVALID_ARGUMENT
    assert f"item {bad_at}: context_slot 1 beyond the 0 contexts" in str(ei.value), str(ei.value)
    items[bad_at]["context_slot"] = 0
    items[n - 1]["context_slot"] = 0
    e.submit_into(items, pp, pe).wait()
    assert np.array_equal(pp, world["want_rand"][0][:n]) and np.all(pe == 0)
    assert e.stats()["aql_batches"] > 0  # the join read the items in place
