#!/usr/bin/env python3
"""Recheck requests (gck_recheck_cross_device) on one GPU, against what a caller did without them.

Config 4's graph (tests/synth.py at --tuples; `doc#view@user`). A request is --shape S x R, one device
tile at the default max_batch; its subject and resource ids are those of the config's own checks. Each
request buffer's plane is taken at revision 1 and kept in HBM; then one real Watch batch is applied
(gck_apply_updates -> revision 2) that touches the requests' own ids — viewer grants of listed docs
deleted, listed users added to groups that view listed docs — and every line answers, at revision 2,
"what changed since the plane I kept". Lines, each a Python loop of one request at a time on the
current stream:

    a_recheck_cross_ids       Engine.recheck_cross_ids(prev = the kept plane): the new plane and the CSR of
                              changes (ids, columns, transition bytes) by kernels; two count words read back
    b_check_twice_torch_diff  the same job the parent commit's way: Engine.check_cross_ids twice (the call
                              that gives the previous plane and the call after the batch), then a torch
                              unpack of both planes, a compare and an ordered nonzero with a gather
    b1_check_once_torch_diff  (b) with one check_cross_ids only: a caller in a steady loop, whose
                              previous call already paid for the previous plane

The lines alternate within each of --rounds rounds after one untimed warm-up run each; per line the
median and max - min over the rounds, in checks per second. Before any timing every line's plane and
CSR are compared, on every request buffer, with a numpy diff of the host cross call's planes taken
before and after the batch. One JSON line out.

    python tools/bench_recheck.py [--shape 256x200] [--tuples 1e8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=float, default=1e8, help="the graph's tuples")
    ap.add_argument("--shape", default="256x200", help="S x R")
    ap.add_argument("--requests", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=8, help="distinct request buffers the loops cycle through")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gochugaru_amd import engine as E
    from tests import synth

    E.pin_to_device_node(0)
    mb = 65536
    eng = E.Engine(device=0, max_batch=mb)
    G = synth.build(args.tuples, device="cuda")
    eng.load_schema(synth.SCHEMA)
    eng.begin_snapshot(1)
    for t, cnt in ((synth.T_USER, G.n_users), (synth.T_GROUP, G.n_groups), (synth.T_DOC, G.n_docs)):
        eng.reserve_objects(t, cnt)
    keep = []
    n_tuples = 0
    for rel, st, sr, n_rows, off, nbr in G.csrs():
        off32, nbr32 = off.to(torch.int32).contiguous(), nbr.contiguous()
        keep.append((off32, nbr32))
        n_tuples += nbr32.numel()
        eng.load_csr(rel, st, sr, n_rows, off32.data_ptr(), nbr32.data_ptr(), nbr32.numel(), device=True)
    eng.commit_snapshot()
    torch.cuda.synchronize()
    header = (synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS)

    S, R = (int(x) for x in args.shape.split("x"))
    n, stride, nb, k = S * R, (R + 31) // 32, args.buffers, args.requests
    assert E.cross_tile_device(S, R, mb) == S, args.shape + " is not one device tile"
    assert k >= nb
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    shifts = torch.arange(0, 64, 2, dtype=torch.int64, device=dev)
    H = synth.host_arrays(G)
    v_off, v_nbr = H["viewer_off"].astype(np.int64), H["viewer_nbr"]

    # the request buffers, their planes at revision 1 (device: kept; host: the yardstick), and the batch
    bufs, ups = [], {}
    for b in range(nb):
        it = synth.checks(G, mb, seed=100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
        sub, res = it["subject_id"].astype(np.uint32)[:S].copy(), it["resource_id"].astype(np.uint32)[:R].copy()
        words, errs, _ = eng.check_cross(header, sub, res)
        assert len(errs) == 0, "a check has a per-item error"
        ds, dr = to_dev(sub), to_dev(res)
        bufs.append({"sub": sub, "res": res, "ds": ds, "dr": dr, "host_a": np.asarray(words).copy(),
                     "prev": eng.check_cross_ids(header, ds, dr)})
        for j in range(0, R, 4):  # every fourth listed doc with a viewer group: the grant goes, or a listed user joins the group
            d = int(res[j])
            if v_off[d + 1] == v_off[d]:
                continue
            g = int(v_nbr[v_off[d] + (j // 4) % (v_off[d + 1] - v_off[d])])
            if j % 8 == 0:
                ups[(synth.T_DOC, synth.R_VIEWER, d, synth.T_GROUP, synth.R_MEMBER, g)] = E.UPDATE_DELETE
            else:
                ups[(synth.T_GROUP, synth.R_MEMBER, g, synth.T_USER, synth.ELLIPSIS, int(sub[(j // 4) % S]))] = E.UPDATE_TOUCH
    # (one update per relationship: a doc or a user that two buffers share is updated once)
    batch = np.zeros(len(ups), dtype=E.UPDATE_DTYPE)
    batch["op"] = list(ups.values())
    t = batch["tuple"]
    for f, col in zip(("resource_type", "relation", "resource_id", "subject_type", "subject_relation", "subject_id"),
                      zip(*ups.keys())):
        t[f] = col
    batch["tuple"] = t
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.apply_updates(2, batch)
    apply_s = time.perf_counter() - t0
    assert eng.revision == 2

    def unpack(plane):
        return ((plane.reshape(S, stride).unsqueeze(2) >> shifts) & 3).reshape(S, -1)[:, :R]

    def torch_diff(prev, new, dr):
        vo, vn = unpack(prev), unpack(new)
        ch = vo != vn  # CHANGE_ANY
        row_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        row_off[1:] = torch.cumsum(ch.sum(dim=1), dim=0)
        r, c = ch.nonzero(as_tuple=True)
        return new, row_off, dr[c], c.to(torch.int32), (4 * vo[r, c] + vn[r, c]).to(torch.uint8)

    def line_a(b):
        plane, _, row_off, ids, col, trans = eng.recheck_cross_ids(header, b["ds"], b["dr"], prev=b["prev"])
        return plane, row_off, ids, col, trans

    def line_b(b):
        eng.check_cross_ids(header, b["ds"], b["dr"])  # (the call that gives a caller its previous plane)
        return torch_diff(b["prev"], eng.check_cross_ids(header, b["ds"], b["dr"]), b["dr"])

    def line_b1(b):
        return torch_diff(b["prev"], eng.check_cross_ids(header, b["ds"], b["dr"]), b["dr"])

    class Loop:
        def __init__(self, one):
            self.one, self.got = one, [None] * nb

        def run(self):
            t0 = time.perf_counter()
            for i in range(k):
                self.got[i % nb] = self.one(bufs[i % nb])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

    loops = {"a_recheck_cross_ids": Loop(line_a), "b_check_twice_torch_diff": Loop(line_b),
             "b1_check_once_torch_diff": Loop(line_b1)}
    order = sorted(loops)
    d0 = eng.device_compact_stats()
    for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
        loops[line].run()
    # agreement, on every request buffer: the numpy diff of the host call's planes before and after the batch
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    changes = gained = lost = 0
    for j, b in enumerate(bufs):
        words, errs, _ = eng.check_cross(header, b["sub"], b["res"])
        assert len(errs) == 0, "a check has a per-item error"
        host_b = np.asarray(words)
        va, vb = E.unpack_cross(b["host_a"], S, R), E.unpack_cross(host_b, S, R)
        assert np.array_equal(b["prev"].cpu().numpy().view(np.uint64).reshape(-1), b["host_a"].reshape(-1)), "the kept plane"
        ch = va != vb
        row_off = np.concatenate([[0], np.cumsum(ch.sum(axis=1))]).astype(np.uint32)
        col = np.nonzero(ch)[1].astype(np.uint32)
        trans = (4 * va[ch] + vb[ch]).astype(np.uint8)
        for line in order:
            plane, g_off, g_ids, g_col, g_trans = loops[line].got[j]
            assert np.array_equal(plane.cpu().numpy().view(np.uint64).reshape(-1), host_b.reshape(-1)), line + ": plane"
            assert np.array_equal(u32(g_off), row_off) and np.array_equal(u32(g_col), col), line + ": offsets or columns"
            assert np.array_equal(u32(g_ids), b["res"][col]) and np.array_equal(g_trans.cpu().numpy(), trans), line + ": records"
        changes += int(ch.sum())
        gained += int(((va < 2) & (vb >= 2)).sum())
        lost += int(((va >= 2) & (vb < 2)).sum())
    assert gained and lost, "the Watch batch changed nothing both ways"
    runs = {line: [] for line in order}
    d1 = eng.device_compact_stats()
    for _ in range(args.rounds):
        for line in order:
            runs[line].append(k * n / loops[line].run())
    d2 = eng.device_compact_stats()

    m = {line: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v} for line, v in runs.items()}
    two = lambda x, y: max(m[x]["spread_max_minus_min"], m[y]["spread_max_minus_min"])
    a, b_, b1 = "a_recheck_cross_ids", "b_check_twice_torch_diff", "b1_check_once_torch_diff"
    result = {"tool": "bench_recheck", "config": f"config-4-shaped nested groups, {n_tuples} tuples", "tuples": n_tuples,
              "shape": args.shape, "subjects": S, "resources": R, "checks_per_request": n, "buffers": nb,
              "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s",
              "every_line_is_a_python_loop_one_request_at_a_time": True,
              "watch_batch_updates": int(len(batch)), "watch_batch_apply_s": apply_s,
              "changes_per_request": changes / nb, "gained_per_request": gained / nb, "lost_per_request": lost / nb,
              "lines": m, "us_per_request": {line: n / m[line]["median"] * 1e6 for line in order},
              "a_over_b": m[a]["median"] / m[b_]["median"], "a_over_b1": m[a]["median"] / m[b1]["median"],
              "expectations": {
                  "a_not_slower_than_b_by_more_than_both_spreads": bool(m[b_]["median"] - m[a]["median"] <= two(a, b_)),
                  "a_not_slower_than_b1_by_more_than_both_spreads": bool(m[b1]["median"] - m[a]["median"] <= two(a, b1))},
              "device_tiles_in_place_timed": d2[0] - d1[0], "device_chunks_expanded_timed": d2[1] - d1[1],
              "device_tiles_in_place_warmup": d1[0] - d0[0], "device_chunks_expanded_warmup": d1[1] - d0[1]}
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
