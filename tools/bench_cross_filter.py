#!/usr/bin/env python3
"""Cross filter requests (gck_filter_cross_device, and by resource gck_filter_cross_cols_device) on one
GPU, against the plain cross device request and against what a caller did without them.

Config 4's graph (tests/synth.py at --tuples; `doc#view@user`) or, with --config gdocs, config 2
(tests/synth_configs.py at --scale). A request's subject and resource ids are those of the config's
own checks; its shape is --shape S x R, one device tile each at the default max_batch. Lines:

    a_cross_dev         the plain cross device request, two separate id lists: the plane and nothing else
                        (gckd_run_cross_device, --inflight in flight on the engine's streams)
    c_filter_cross      the cross filter request on the same lists: plane + row offsets, row counts and
                        surviving ids (gckd_run_filter_cross_device, the same loop)
    b_torch_csr         what a caller did without it: Engine.check_cross_ids, then torch ops on the plane
                        (shift, mask, compare, cumsum, nonzero, gather) that yield the same CSR — a
                        Python loop, one request at a time
    c_filter_cross_ids  the same caller with the filter: Engine.filter_cross_ids — a Python loop, one
                        request at a time, so that (b) and (c) are compared in the same kind of loop
    d_filter_cross_cols      the cross filter request by resource on the same lists: plane + column offsets,
                             column counts and surviving subject ids (gckd_run_filter_cross_cols_device,
                             the same compiled loop as c_filter_cross)
    d_filter_cross_cols_ids  Engine.filter_cross_cols_ids — a Python loop, one request at a time
    e_torch_csr_cols         what a caller did without it: Engine.check_cross_ids, then torch ops (shift,
                             mask, compare, transpose, sum, cumsum, nonzero, gather) that yield the same CSR
                             by resource — a Python loop, one request at a time, to compare with the line above

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds, in checks per second. Before any timing (c)'s, (b)'s, (d)'s and (e)'s CSR are compared, on every
request buffer, with a numpy selection over (a)'s plane. Then a lone request's latency (one in flight,
--lone requests) for the compiled (a), (c) and (d): the differences from (a) are the cost of the three
selection kernels of each form. One JSON line out.

    python tools/bench_cross_filter.py [--config nested|gdocs] [--shape 64x1000,256x200,1024x32] [--out FILE]
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
    ap.add_argument("--config", default="nested", choices=["gdocs", "nested"])
    ap.add_argument("--scale", type=float, default=0.2, help="--config gdocs: config 2 at this scale (1.0 = 10M tuples)")
    ap.add_argument("--tuples", type=float, default=1e8, help="--config nested: the graph's tuples")
    ap.add_argument("--shape", default="64x1000,256x200,1024x32", help="S x R, comma-separated")
    ap.add_argument("--row-limit", type=int, default=0, help="gck_select_rows.row_limit (0: every survivor)")
    ap.add_argument("--col-limit", type=int, default=0, help="gck_select_cols.col_limit (0: every survivor)")
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=16, help="distinct request buffers the loops cycle through")
    ap.add_argument("--lone", type=int, default=300, help="lone requests per latency line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gochugaru_amd import engine as E

    E.pin_to_device_node(0)
    mb = 65536
    eng = E.Engine(device=0, max_batch=mb, workspaces=args.inflight)
    keep = []
    if args.config == "gdocs":
        from tests import synth_configs
        W = synth_configs.gdocs(args.scale, device="cuda")
        eng.load_schema(W.schema)
        eng.begin_snapshot(1)
        for t, cnt in W.counts.items():
            eng.reserve_objects(W.t(t), cnt)
        csrs, n_tuples = W.csrs, W.n_tuples
        header = (W.t("doc"), W.r("doc", "view"), W.t("user"), E.ELLIPSIS)
        checks = lambda seed: synth_configs.checks(W, mb, seed=seed)
        what = f"config 2 (gdocs) at scale {args.scale}"
    else:
        from tests import synth
        G = synth.build(args.tuples, device="cuda")
        eng.load_schema(synth.SCHEMA)
        eng.begin_snapshot(1)
        for t, cnt in ((synth.T_USER, G.n_users), (synth.T_GROUP, G.n_groups), (synth.T_DOC, G.n_docs)):
            eng.reserve_objects(t, cnt)
        csrs = G.csrs()
        n_tuples = int(sum(c[5].numel() for c in csrs))
        header = (synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS)
        checks = lambda seed: synth.checks(G, mb, seed=seed)
        what = f"config-4-shaped nested groups, {n_tuples} tuples"
    for rel, st, sr, n_rows, off, nbr in csrs:
        off32, nbr32 = off.to(torch.int32).contiguous(), nbr.contiguous()
        keep.append((off32, nbr32))
        eng.load_csr(rel, st, sr, n_rows, off32.data_ptr(), nbr32.data_ptr(), nbr32.numel(), device=True)
    eng.commit_snapshot()
    torch.cuda.synchronize()

    nb, k, depth, limit, climit = args.buffers, args.requests, args.inflight, args.row_limit, args.col_limit
    dev = torch.device("cuda", 0)
    ERR_CAP = 64
    assert k >= nb
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    cyc = lambda xs, m=k: [xs[i % len(xs)] for i in range(m)]
    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    shifts = torch.arange(0, 64, 2, dtype=torch.int64, device=dev)
    result = {"tool": "bench_cross_filter", "config": what, "tuples": n_tuples, "inflight": depth, "row_limit": limit, "col_limit": climit,
              "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s",
              "b_and_c_filter_cross_ids_are_python_loops_one_request_at_a_time": True, "shapes": {}}

    def torch_csr(b, S, R):
        """Line b: the plane from check_cross_ids, then the CSR by torch ops."""
        plane = eng.check_cross_ids(header, b["ds"], b["dr"])
        v = ((plane.unsqueeze(2) >> shifts) & 3).reshape(S, -1)[:, :R]
        keep_ = v >= 2  # SELECT_LOOKUP
        if limit:
            keep_ &= torch.cumsum(keep_, dim=1) <= limit
        row_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        row_off[1:] = torch.cumsum(keep_.sum(dim=1), dim=0)
        col = keep_.nonzero(as_tuple=True)[1]
        return row_off, b["dr"][col]

    def torch_csr_cols(b, S, R):
        """Line e: the plane from check_cross_ids, then the CSR by resource by torch ops."""
        plane = eng.check_cross_ids(header, b["ds"], b["dr"])
        v = ((plane.unsqueeze(2) >> shifts) & 3).reshape(S, -1)[:, :R]
        keep_ = (v >= 2).t()  # SELECT_LOOKUP, by resource
        if climit:
            keep_ = keep_ & (torch.cumsum(keep_, dim=1) <= climit)
        col_off = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        col_off[1:] = torch.cumsum(keep_.sum(dim=1), dim=0)
        row = keep_.nonzero(as_tuple=True)[1]
        return col_off, b["ds"][row]

    def numpy_csr_cols(words, sub, S, R):
        perm = E.unpack_cross(words, S, R).T
        surv = perm >= 2
        if climit:
            surv &= np.cumsum(surv, axis=1) <= climit
        return np.concatenate([[0], np.cumsum(surv.sum(axis=1))]).astype(np.uint32), sub[np.nonzero(surv)[1]], \
            (perm >= 2).sum(axis=1).astype(np.uint32)

    def numpy_csr(words, res, S, R):
        perm = E.unpack_cross(words, S, R)
        surv = perm >= 2
        if limit:
            surv &= np.cumsum(surv, axis=1) <= limit
        return np.concatenate([[0], np.cumsum(surv.sum(axis=1))]).astype(np.uint32), res[np.nonzero(surv)[1]], \
            (perm >= 2).sum(axis=1).astype(np.uint32)

    for shape in args.shape.split(","):
        S, R = (int(x) for x in shape.split("x"))
        n, stride = S * R, (R + 31) // 32
        assert E.cross_tile_device(S, R, mb) == S, shape + " is not one device tile"
        cap = S * (min(limit, R) if limit else R)
        ccap = R * (min(climit, S) if climit else S)
        zeros = lambda m, dt=torch.int32: torch.zeros(m, dtype=dt, device=dev)
        bufs = []
        for b in range(nb):
            it = checks(100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
            sub, res = it["subject_id"].astype(np.uint32)[:S].copy(), it["resource_id"].astype(np.uint32)[:R].copy()
            bufs.append({"res": res, "sub": sub, "ds": to_dev(sub), "dr": to_dev(res),
                         "d": {"words": zeros(S * stride, torch.int64), "errs": zeros((ERR_CAP, 2)), "cnt": zeros(1),
                               "col_off": zeros(R + 1), "col_n": zeros(R), "ids": zeros(ccap), "n": zeros(1)},
                         "a": {"words": zeros(S * stride, torch.int64), "errs": zeros((ERR_CAP, 2)), "cnt": zeros(1)},
                         "c": {"words": zeros(S * stride, torch.int64), "errs": zeros((ERR_CAP, 2)), "cnt": zeros(1),
                               "row_off": zeros(S + 1), "row_n": zeros(S), "ids": zeros(cap), "n": zeros(1)}})
        torch.cuda.synchronize()

        def loops_for(bs_, m, d):
            ptr = lambda f: cyc([f(b).data_ptr() for b in bs_], m)
            lists = ([header] * m, ptr(lambda b: b["ds"]), [S] * m, ptr(lambda b: b["dr"]), [R] * m)
            return {"a_cross_dev": eng.prepare_cross_device(*lists, ptr(lambda b: b["a"]["words"]),
                                                            ptr(lambda b: b["a"]["errs"]), ERR_CAP, d,
                                                            n_errs=ptr(lambda b: b["a"]["cnt"]), engine_streams=True),
                    "c_filter_cross": eng.prepare_filter_cross_device(
                        *lists, ptr(lambda b: b["c"]["row_off"]), ptr(lambda b: b["c"]["n"]), cap,
                        ptr(lambda b: b["c"]["words"]), d, out_ids=ptr(lambda b: b["c"]["ids"]),
                        row_n=ptr(lambda b: b["c"]["row_n"]), row_limit=limit, errs=ptr(lambda b: b["c"]["errs"]),
                        err_cap=ERR_CAP, n_errs=ptr(lambda b: b["c"]["cnt"]), engine_streams=True),
                    "d_filter_cross_cols": eng.prepare_filter_cross_cols_device(
                        *lists, ptr(lambda b: b["d"]["col_off"]), ptr(lambda b: b["d"]["n"]), ccap,
                        ptr(lambda b: b["d"]["words"]), d, out_ids=ptr(lambda b: b["d"]["ids"]),
                        col_n=ptr(lambda b: b["d"]["col_n"]), col_limit=climit, errs=ptr(lambda b: b["d"]["errs"]),
                        err_cap=ERR_CAP, n_errs=ptr(lambda b: b["d"]["cnt"]), engine_streams=True)}

        class Loop:  # (a Python loop with the compiled loops' interface)
            def __init__(self, one):
                self.one, self.got = one, [None] * nb

            def run(self):
                t0 = time.perf_counter()
                for i in range(k):
                    self.got[i % nb] = self.one(bufs[i % nb])
                torch.cuda.synchronize()
                return time.perf_counter() - t0

        loops = loops_for(bufs, k, depth)
        loops["b_torch_csr"] = Loop(lambda b: torch_csr(b, S, R))
        loops["c_filter_cross_ids"] = Loop(lambda b: eng.filter_cross_ids(header, b["ds"], b["dr"], row_limit=limit))
        loops["e_torch_csr_cols"] = Loop(lambda b: torch_csr_cols(b, S, R))
        loops["d_filter_cross_cols_ids"] = Loop(lambda b: eng.filter_cross_cols_ids(header, b["ds"], b["dr"],
                                                                                     col_limit=climit))
        order = sorted(loops)
        d0 = eng.device_compact_stats()
        for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
            loops[line].run()
        torch.cuda.synchronize()
        # agreement, on every request buffer: each CSR against a numpy selection over (a)'s plane
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        kept = surv = ckept = 0
        for j, b in enumerate(bufs):
            assert int(u32(b["a"]["cnt"])[0]) == 0 and int(u32(b["c"]["cnt"])[0]) == 0, "a check has a per-item error"
            words = b["a"]["words"].cpu().numpy().view(np.uint64)
            assert np.array_equal(b["c"]["words"].cpu().numpy().view(np.uint64), words), "the filter's plane differs"
            row_off, ids, row_n = numpy_csr(words, b["res"], S, R)
            total = int(row_off[-1])
            assert int(u32(b["c"]["n"])[0]) == total and np.array_equal(u32(b["c"]["row_off"]), row_off), "line c: offsets"
            assert np.array_equal(u32(b["c"]["ids"])[:total], ids), "line c: ids"
            assert np.array_equal(u32(b["c"]["row_n"]), row_n), "line c: row counts"
            for line in ("b_torch_csr", "c_filter_cross_ids"):
                g_off, g_ids = loops[line].got[j]
                assert np.array_equal(u32(g_off), row_off) and np.array_equal(u32(g_ids), ids), line + " differs"
            kept += total
            surv += int(row_n.sum())
            # by resource: (d)'s and (e)'s CSR against the numpy selection over the same plane, transposed
            assert int(u32(b["d"]["cnt"])[0]) == 0, "a check has a per-item error"
            assert np.array_equal(b["d"]["words"].cpu().numpy().view(np.uint64), words), "the column filter's plane differs"
            col_off, cids, col_n = numpy_csr_cols(words, b["sub"], S, R)
            ctotal = int(col_off[-1])
            assert int(u32(b["d"]["n"])[0]) == ctotal and np.array_equal(u32(b["d"]["col_off"]), col_off), "line d: offsets"
            assert np.array_equal(u32(b["d"]["ids"])[:ctotal], cids), "line d: ids"
            assert np.array_equal(u32(b["d"]["col_n"]), col_n), "line d: column counts"
            for line in ("e_torch_csr_cols", "d_filter_cross_cols_ids"):
                g_off, g_ids = loops[line].got[j]
                assert np.array_equal(u32(g_off), col_off) and np.array_equal(u32(g_ids), cids), line + " differs"
            ckept += ctotal
        runs = {line: [] for line in order}
        d1 = eng.device_compact_stats()
        for _ in range(args.rounds):
            for line in order:
                runs[line].append(k * n / loops[line].run())
        d2 = eng.device_compact_stats()

        # a lone request's latency through the compiled loops: one at a time, (a) and (c) alternated
        one = [loops_for([b], 1, 1) for b in bufs]
        for p in one:
            for line in p:
                p[line].run()
        lone = {"a_cross_dev": [], "c_filter_cross": [], "d_filter_cross_cols": []}
        for i in range(args.lone):
            for line in lone:
                lone[line].append(one[i % nb][line].run() * 1e6)

        m = {line: line_of(v) for line, v in runs.items()}
        two = lambda x, y: max(m[x]["spread_max_minus_min"], m[y]["spread_max_minus_min"])
        us = lambda line: n / m[line]["median"] * 1e6  # (of the loop's wall time; the compiled loops overlap `inflight`)
        lone_m = {name: {"median": statistics.median(v), "p10": float(np.percentile(v, 10)),
                         "p90": float(np.percentile(v, 90)), "requests": len(v)} for name, v in lone.items()}
        result["shapes"][shape] = {
            "subjects": S, "resources": R, "checks_per_request": n, "survivor_share": surv / (n * nb),
            "kept_per_request": kept / nb, "lines": m, "lone_us": lone_m,
            "us_per_request": {line: us(line) for line in order},
            "c_minus_a_us_per_request_in_the_loop": us("c_filter_cross") - us("a_cross_dev"),
            "c_minus_a_us_lone_median": lone_m["c_filter_cross"]["median"] - lone_m["a_cross_dev"]["median"],
            "c_filter_cross_ids_over_b_torch_csr": m["c_filter_cross_ids"]["median"] / m["b_torch_csr"]["median"],
            "kept_per_request_by_resource": ckept / nb,
            "d_minus_a_us_per_request_in_the_loop": us("d_filter_cross_cols") - us("a_cross_dev"),
            "d_minus_a_us_lone_median": lone_m["d_filter_cross_cols"]["median"] - lone_m["a_cross_dev"]["median"],
            "d_minus_c_us_per_request_in_the_loop": us("d_filter_cross_cols") - us("c_filter_cross"),
            "d_filter_cross_cols_ids_over_e_torch_csr_cols":
                m["d_filter_cross_cols_ids"]["median"] / m["e_torch_csr_cols"]["median"],
            "d_filter_cross_cols_over_c_filter_cross": m["d_filter_cross_cols"]["median"] / m["c_filter_cross"]["median"],
            "expectations": {
                "d_filter_cross_cols_ids_above_e_by_more_than_both_spreads":
                    bool(m["d_filter_cross_cols_ids"]["median"] - m["e_torch_csr_cols"]["median"]
                         > two("d_filter_cross_cols_ids", "e_torch_csr_cols")),
                "d_filter_cross_cols_below_c_by_more_than_both_spreads":
                    bool(m["c_filter_cross"]["median"] - m["d_filter_cross_cols"]["median"]
                         > two("c_filter_cross", "d_filter_cross_cols")),
                "c_filter_cross_ids_above_b_by_more_than_both_spreads":
                    bool(m["c_filter_cross_ids"]["median"] - m["b_torch_csr"]["median"] > two("c_filter_cross_ids", "b_torch_csr")),
                "c_filter_cross_above_b": bool(m["c_filter_cross"]["median"] > m["b_torch_csr"]["median"])},
            "device_tiles_in_place_timed": d2[0] - d1[0], "device_chunks_expanded_timed": d2[1] - d1[1],
            "device_tiles_in_place_warmup": d1[0] - d0[0], "device_chunks_expanded_warmup": d1[1] - d0[1]}
        del bufs, loops, one
        torch.cuda.empty_cache()

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
