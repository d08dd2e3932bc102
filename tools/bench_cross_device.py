#!/usr/bin/env python3
"""Cross requests over device buffers on one GPU, against what a device caller had before them.

Config 2 (tests/synth_configs.py gdocs at --scale; `doc#view@user`) or, with --config nested, a
config-4-shaped graph (tests/synth.py at --tuples; `doc#view@user`). A request's subject and
resource ids are those of the config's own checks; its shape is --shape S x R (256x256: 65,536
checks; 32x2016: 64,512, the widest tile the id block holds). Lines, --inflight in flight through
the compiled submit/wait loops of libgck_driver.so, the device lines on the engine's streams:

    a_uniform_dev    the same product as (resource, subject) pairs prebuilt in HBM, a uniform device request
    b_cross_dev      the cross device request, two separate id lists (gathered into the id block)
    c_cross_block    the cross device request, the lists in block layout (read where they are)
    d_cross_host     gckd_run_cross from pinned host lists
    e_torch_pairs    what a device caller did without the cross device call: torch builds the pairs from
                     the two lists (repeat, repeat_interleave, stack), then the synchronous uniform
                     device call — a Python loop, one request at a time, not 8 in flight

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds are reported in checks per second. Before any timing every line's plane is compared on every
request buffer. Then a lone request's latency for a, c and e. One JSON line out.

    python tools/bench_cross_device.py [--config gdocs|nested] [--shape 256x256] [--rounds 5] [--out FILE]
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
    ap.add_argument("--config", default="gdocs", choices=["gdocs", "nested"])
    ap.add_argument("--scale", type=float, default=0.2, help="config 2 at this scale (1.0 = 10M tuples)")
    ap.add_argument("--tuples", type=float, default=1e8, help="--config nested: the graph's tuples")
    ap.add_argument("--shape", default="256x256,32x2016", help="S x R, comma-separated")
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=200)
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

    nb, k, depth = args.buffers, args.requests, args.inflight
    dev = torch.device("cuda", 0)
    ERR_CAP = 1024
    assert k >= nb
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    cyc = lambda xs, m=k: [xs[i % len(xs)] for i in range(m)]
    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    result = {"tool": "bench_cross_device", "config": what, "tuples": n_tuples, "inflight": depth,
              "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s", "shapes": {}}

    for shape in args.shape.split(","):
        S, R = (int(x) for x in shape.split("x"))
        n, stride = S * R, (R + 31) // 32
        assert E.cross_tile_device(S, R, mb) == S and E.cross_tile(S, R, mb) == (S, R), shape
        dev_lines = ["a_uniform_dev", "b_cross_dev", "c_cross_block"]

        def out(words):
            return {"words": torch.zeros(words, dtype=torch.int64, device=dev),
                    "errs": torch.zeros((ERR_CAP, 2), dtype=torch.int32, device=dev),
                    "cnt": torch.zeros(1, dtype=torch.int32, device=dev)}

        bufs = []
        for b in range(nb):
            it = checks(100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
            sub, res = it["subject_id"].astype(np.uint32)[:S].copy(), it["resource_id"].astype(np.uint32)[:R].copy()
            ds, dr = to_dev(sub), to_dev(res)
            block, bs, br = E.cross_id_block(ds, dr)
            hs, hr = eng.host_array(S, np.uint32), eng.host_array(R, np.uint32)
            hs[:], hr[:] = sub, res
            pairs = torch.stack([dr.repeat(S), ds.repeat_interleave(R)], dim=1).contiguous()
            bufs.append({"ds": ds, "dr": dr, "block": block, "bs": bs, "br": br, "hs": hs, "hr": hr, "pairs": pairs,
                         "h_plane": eng.host_array(S * stride, np.uint64),
                         "h_errs": eng.host_array(ERR_CAP, E.ITEM_ERROR_DTYPE), "e_out": out((n + 31) // 32),
                         "out": {line: out((n + 31) // 32 if line == "a_uniform_dev" else S * stride)
                                 for line in dev_lines}})
        torch.cuda.synchronize()
        outp = lambda line, what, m=k: cyc([b["out"][line][what].data_ptr() for b in bufs], m)

        def uniform_loop(bs_, m, d):
            return eng.prepare_uniform_device([header] * m, cyc([b["pairs"].data_ptr() for b in bs_], m), [n] * m,
                                              cyc([b["out"]["a_uniform_dev"]["words"].data_ptr() for b in bs_], m),
                                              cyc([b["out"]["a_uniform_dev"]["errs"].data_ptr() for b in bs_], m), ERR_CAP,
                                              d, n_errs=cyc([b["out"]["a_uniform_dev"]["cnt"].data_ptr() for b in bs_], m),
                                              engine_streams=True)

        def cross_loop(line, sub_key, res_key, bs_, m, d):
            return eng.prepare_cross_device([header] * m, cyc([b[sub_key].data_ptr() for b in bs_], m), [S] * m,
                                            cyc([b[res_key].data_ptr() for b in bs_], m), [R] * m,
                                            cyc([b["out"][line]["words"].data_ptr() for b in bs_], m),
                                            cyc([b["out"][line]["errs"].data_ptr() for b in bs_], m), ERR_CAP, d,
                                            n_errs=cyc([b["out"][line]["cnt"].data_ptr() for b in bs_], m),
                                            engine_streams=True)

        def torch_pairs(b):
            """Line e: one request as a device caller sent it before the cross device call."""
            pairs = torch.stack([b["dr"].repeat(S), b["ds"].repeat_interleave(R)], dim=1)
            o = b["e_out"]
            eng.check_uniform_device(header, pairs.data_ptr(), n, o["words"].data_ptr(), o["errs"].data_ptr(), ERR_CAP,
                                     o["cnt"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)

        class Loop:  # (a Python loop with the compiled loops' interface)
            def run(self):
                t0 = time.perf_counter()
                for i in range(k):
                    torch_pairs(bufs[i % nb])
                return time.perf_counter() - t0

        loops = {"a_uniform_dev": uniform_loop(bufs, k, depth),
                 "b_cross_dev": cross_loop("b_cross_dev", "ds", "dr", bufs, k, depth),
                 "c_cross_block": cross_loop("c_cross_block", "bs", "br", bufs, k, depth),
                 "d_cross_host": eng.prepare_cross([header] * k, cyc([b["hs"].ctypes.data for b in bufs]), [S] * k,
                                                   cyc([b["hr"].ctypes.data for b in bufs]), [R] * k,
                                                   cyc([b["h_plane"].ctypes.data for b in bufs]),
                                                   cyc([b["h_errs"].ctypes.data for b in bufs]), ERR_CAP, depth),
                 "e_torch_pairs": Loop()}
        order = sorted(loops)
        d0 = eng.device_compact_stats()
        for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
            loops[line].run()
        torch.cuda.synchronize()
        # agreement, on every request buffer: each plane against the uniform device request's dense words
        words = lambda o: o["words"].cpu().numpy().view(np.uint64)
        count = lambda o: int(o["cnt"].cpu().numpy().view(np.uint32)[0])
        for b in bufs:
            dense = E.unpack_results(words(b["out"]["a_uniform_dev"]), n).reshape(S, R)
            assert np.array_equal(E.unpack_results(words(b["e_out"]), n).reshape(S, R), dense), "line e differs"
            assert np.array_equal(E.unpack_cross(np.asarray(b["h_plane"]), S, R), dense), "line d differs"
            for line in dev_lines[1:]:
                assert np.array_equal(E.unpack_cross(words(b["out"][line]), S, R), dense), line + " differs"
                assert count(b["out"][line]) == count(b["out"]["a_uniform_dev"]), line + ": error counts differ"
        runs = {line: [] for line in order}
        left = {line: [0, 0] for line in order}  # checks the joins left to the bundle stages, of how many
        d1 = eng.device_compact_stats()
        for _ in range(args.rounds):
            for line in order:
                eng.reset_stats()
                runs[line].append(k * n / loops[line].run())
                st = eng.stats()
                left[line][0] += int(st["queries"] - st["closure_checks"])
                left[line][1] += int(st["queries"])
        d2 = eng.device_compact_stats()

        # a lone request's latency: one at a time
        lone = {}
        one = {"a_uniform_dev": [uniform_loop([b], 1, 1) for b in bufs],
               "c_cross_block": [cross_loop("c_cross_block", "bs", "br", [b], 1, 1) for b in bufs]}
        for name, ps in one.items():
            for p in ps:
                p.run()
            lone[name] = [ps[i % nb].run() * 1e6 for i in range(args.lone)]
        lone["e_torch_pairs"] = []
        for i in range(args.lone):
            t0 = time.perf_counter()
            torch_pairs(bufs[i % nb])
            lone["e_torch_pairs"].append((time.perf_counter() - t0) * 1e6)

        m = {line: line_of(v) for line, v in runs.items()}
        above = lambda x, y: m[x]["median"] - m[y]["median"] > max(m[x]["spread_max_minus_min"],
                                                                   m[y]["spread_max_minus_min"])
        r = {"subjects": S, "resources": R, "checks_per_request": n, "lines": m,
             "bytes_in_per_check": {"a_uniform_dev": 8.0, "b_cross_dev": 4 * (S + R) / n, "c_cross_block": 4 * (S + R) / n,
                                    "d_cross_host": 4 * (S + R) / n, "e_torch_pairs": 8.0},
             "lone_us": {name: {"median": statistics.median(v), "p10": float(np.percentile(v, 10)),
                                "p90": float(np.percentile(v, 90)), "requests": len(v)} for name, v in lone.items()},
             "device_tiles_in_place_timed": d2[0] - d1[0], "device_chunks_expanded_timed": d2[1] - d1[1],
             "device_tiles_in_place_warmup": d1[0] - d0[0], "device_chunks_expanded_warmup": d1[1] - d0[1],
             "deferred_share": {line: (v[0] / v[1] if v[1] else 0.0) for line, v in left.items()},
             "expectations": {"c_above_a_by_more_than_both_spreads": bool(above("c_cross_block", "a_uniform_dev")),
                              "c_at_least_d": bool(m["c_cross_block"]["median"] >= m["d_cross_host"]["median"]),
                              "b_above_e": bool(m["b_cross_dev"]["median"] > m["e_torch_pairs"]["median"])}}
        result["shapes"][shape] = r
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
