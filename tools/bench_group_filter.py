#!/usr/bin/env python3
"""Group filter requests (gck_filter_groups_device) on one GPU, against the same job done without
them: a candidate list per subject, each subject's permitted candidates as a CSR.

Config 4's graph (tests/synth.py at --tuples; `doc#view@user`). A request is --groups subjects with
--per candidates each (512 x 128: one 64K batch); its subject and resource ids are those of the
config's own checks. Lines, each a Python loop of one request at a time on the current stream:

    a_filter_groups_ids   Engine.filter_groups_ids: owners, offsets and candidates in, the CSR out
    b_uniform_torch       what a caller did without it: the pairs built with torch (repeat_interleave +
                          stack), Engine.check_uniform_device over them, a torch unpack of the plane, then
                          a per-group ordered selection in torch (segment ranks from a cumsum, a compare
                          with the limit, nonzero, gather) that yields the same CSR

The lines alternate within each of --rounds rounds after one untimed warm-up run each; per line the
median and max - min over the rounds, in checks per second, for every --limit. Before any timing both
lines' CSRs are compared, on every request buffer, with a numpy selection over the host uniform call's
plane. One JSON line out.

    python tools/bench_group_filter.py [--groups 512] [--per 128] [--limit 0,10] [--out FILE]
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
    ap.add_argument("--groups", type=int, default=512)
    ap.add_argument("--per", type=int, default=128, help="candidates per group")
    ap.add_argument("--limit", default="0,10", help="gck_select_groups.group_limit values, comma-separated (0: every survivor)")
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
    eng = E.Engine(device=0, max_batch=mb, workspaces=2)
    keep = []
    G = synth.build(args.tuples, device="cuda")
    eng.load_schema(synth.SCHEMA)
    eng.begin_snapshot(1)
    for t, cnt in ((synth.T_USER, G.n_users), (synth.T_GROUP, G.n_groups), (synth.T_DOC, G.n_docs)):
        eng.reserve_objects(t, cnt)
    csrs = G.csrs()
    n_tuples = int(sum(c[5].numel() for c in csrs))
    header = (synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS)
    for rel, st, sr, n_rows, off, nbr in csrs:
        off32, nbr32 = off.to(torch.int32).contiguous(), nbr.contiguous()
        keep.append((off32, nbr32))
        eng.load_csr(rel, st, sr, n_rows, off32.data_ptr(), nbr32.data_ptr(), nbr32.numel(), device=True)
    eng.commit_snapshot()
    torch.cuda.synchronize()

    S, per, nb, k = args.groups, args.per, args.buffers, args.requests
    n = S * per
    assert n <= mb and k >= nb
    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    shifts = torch.arange(0, 64, 2, dtype=torch.int64, device=dev)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)

    bufs = []
    off = np.arange(S + 1, dtype=np.uint32) * per
    for b in range(nb):
        it = synth.checks(G, mb, seed=100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
        sub, res = it["subject_id"].astype(np.uint32)[:S].copy(), it["resource_id"].astype(np.uint32)[:n].copy()
        bufs.append({"sub": sub, "res": res, "do": to_dev(sub), "dg": to_dev(off), "dc": to_dev(res),
                     "plane": torch.zeros((n + 31) // 32, dtype=torch.int64, device=dev)})
    torch.cuda.synchronize()

    def uniform_torch(b, limit):
        """Line b: the pairs, the uniform device request, the unpack and the per-group selection, in torch."""
        lens = b["dg"][1:] - b["dg"][:-1]
        own = torch.repeat_interleave(b["do"], lens)
        pairs = torch.stack([b["dc"], own], dim=1).contiguous()
        eng.check_uniform_device(header, pairs.data_ptr(), n, b["plane"].data_ptr(),
                                 stream=torch.cuda.current_stream(dev).cuda_stream)
        v = ((b["plane"].unsqueeze(1) >> shifts) & 3).reshape(-1)[:n]
        keep_ = v >= 2  # SELECT_LOOKUP
        run = torch.cumsum(keep_, dim=0)
        base = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        base[1:] = run[(b["dg"][1:] - 1).long()]  # (no empty group here: every group's last check exists)
        if limit:
            group = torch.repeat_interleave(torch.arange(S, device=dev), lens)
            keep_ = keep_ & (run - base[group] <= limit)
            run = torch.cumsum(keep_, dim=0)
            base[1:] = run[(b["dg"][1:] - 1).long()]
        return base.to(torch.int32), b["dc"][keep_.nonzero(as_tuple=True)[0]]

    def numpy_csr(words, res, limit):
        perm = E.unpack_results(words, n).reshape(S, per)
        surv = perm >= 2
        if limit:
            surv &= np.cumsum(surv, axis=1) <= limit
        return np.concatenate([[0], np.cumsum(surv.sum(axis=1))]).astype(np.uint32), res[np.nonzero(surv.reshape(-1))[0]]

    class Loop:
        def __init__(self, one):
            self.one, self.got = one, [None] * nb

        def run(self):
            t0 = time.perf_counter()
            for i in range(k):
                self.got[i % nb] = self.one(bufs[i % nb])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

    result = {"tool": "bench_group_filter", "config": f"config-4-shaped nested groups, {n_tuples} tuples", "tuples": n_tuples,
              "groups": S, "candidates_per_group": per, "checks_per_request": n, "timed_requests_per_run": k,
              "rounds": args.rounds, "unit": "checks/s", "both_lines_are_python_loops_one_request_at_a_time": True,
              "limits": {}}
    yard = []
    for b in bufs:  # the host uniform call's plane of each buffer, once
        pairs = np.stack([b["res"], np.repeat(b["sub"], per)], axis=1).astype(np.uint32)
        words, errs, _ = eng.check_uniform(header, pairs)
        assert len(errs) == 0, "a check has a per-item error"
        yard.append(np.asarray(words).copy())
    for limit in (int(x) for x in args.limit.split(",")):
        loops = {"a_filter_groups_ids": Loop(lambda b: eng.filter_groups_ids(header, b["do"], b["dg"], b["dc"], group_limit=limit)),
                 "b_uniform_torch": Loop(lambda b: uniform_torch(b, limit))}
        order = sorted(loops)
        d0 = eng.device_compact_stats()
        for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
            loops[line].run()
        kept = surv = 0
        for j, b in enumerate(bufs):  # agreement, on every request buffer
            row_off, ids = numpy_csr(yard[j], b["res"], limit)
            for line in order:
                g_off, g_ids = loops[line].got[j]
                assert np.array_equal(u32(g_off), row_off) and np.array_equal(u32(g_ids), ids), line + " differs"
            kept += int(row_off[-1])
            surv += int((E.unpack_results(yard[j], n) >= 2).sum())
        runs = {line: [] for line in order}
        d1 = eng.device_compact_stats()
        for _ in range(args.rounds):
            for line in order:
                runs[line].append(k * n / loops[line].run())
        d2 = eng.device_compact_stats()
        m = {line: line_of(v) for line, v in runs.items()}
        spread = max(m[x]["spread_max_minus_min"] for x in order)
        result["limits"][str(limit)] = {
            "group_limit": limit, "survivor_share": surv / (n * nb), "kept_per_request": kept / nb, "lines": m,
            "us_per_request": {line: n / m[line]["median"] * 1e6 for line in order},
            "a_over_b": m["a_filter_groups_ids"]["median"] / m["b_uniform_torch"]["median"],
            "a_not_slower_than_b": bool(m["a_filter_groups_ids"]["median"] >= m["b_uniform_torch"]["median"]),
            "a_above_b_by_more_than_both_spreads":
                bool(m["a_filter_groups_ids"]["median"] - m["b_uniform_torch"]["median"] > spread),
            "device_chunks_in_place_timed": d2[0] - d1[0], "device_chunks_expanded_timed": d2[1] - d1[1],
            "device_chunks_in_place_warmup": d1[0] - d0[0], "device_chunks_expanded_warmup": d1[1] - d0[1]}

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
