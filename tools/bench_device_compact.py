#!/usr/bin/env python3
"""Compact requests over device buffers against device-resident items on one GPU.

Config 2 (tests/synth_configs.py gdocs at --scale; `doc#view@user`) or, with --config nested, a
config-4-shaped graph (tests/synth.py at --tuples; `doc#view@user`). 65,536 checks per request,
--inflight in flight through the compiled submit/wait loops of libgck_driver.so, every device line
on the engine's workspace streams. Lines:

    items          the ids of the config's checks under `doc#view@user` as device-resident 20-B items, 5 B per
                   check out (the headline path)
    uniform_dev    the same checks as a uniform device request: 8 B in, 1/4 B out, a count word per request
    uniform_dev_nc the same without a count word (d_out_n_errs == NULL: no clear, no stream wait)
    list_dev       one subject against the resource ids of those checks, a device id list: 4 B in
    range_dev      one subject against 65,536 consecutive resource ids: nothing in
    uniform_host   the uniform request from pinned host buffers, for context

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds are reported in checks per second. Before any timing the answers are compared on every
request buffer: uniform_dev with items (packed on the host), with uniform_dev_nc and with
uniform_host; list_dev and range_dev with the host list calls. One JSON line out.

    python tools/bench_device_compact.py [--config gdocs|nested] [--scale 0.2] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="gdocs", choices=["gdocs", "nested"])
    ap.add_argument("--scale", type=float, default=0.2, help="config 2 at this scale (1.0 = 10M tuples)")
    ap.add_argument("--tuples", type=float, default=1e8, help="--config nested: the graph's tuples")
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=16, help="distinct request buffers the loops cycle through")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gochugaru_amd import engine as E

    E.pin_to_device_node(0)
    n = 65536
    eng = E.Engine(device=0, max_batch=n, workspaces=args.inflight)
    keep = []
    if args.config == "gdocs":
        from tests import synth_configs
        W = synth_configs.gdocs(args.scale, device="cuda")
        eng.load_schema(W.schema)
        eng.begin_snapshot(1)
        for t, cnt in W.counts.items():
            eng.reserve_objects(W.t(t), cnt)
        csrs, n_tuples = W.csrs, W.n_tuples
        header = (W.t("doc"), W.r("doc", "view"), W.t("user"), E.ELLIPSIS, 0)
        checks = lambda seed: synth_configs.checks(W, n, seed=seed)
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
        header = (synth.T_DOC, synth.R_VIEW, synth.T_USER, synth.ELLIPSIS, 0)
        checks = lambda seed: synth.checks(G, n, seed=seed)
        what = f"config-4-shaped nested groups, {n_tuples} tuples"
    for rel, st, sr, n_rows, off, nbr in csrs:
        off32, nbr32 = off.to(torch.int32).contiguous(), nbr.contiguous()
        keep.append((off32, nbr32))
        eng.load_csr(rel, st, sr, n_rows, off32.data_ptr(), nbr32.data_ptr(), nbr32.numel(), device=True)
    eng.commit_snapshot()
    torch.cuda.synchronize()
    n_docs = eng.object_count(header[0])

    nb, k, depth = args.buffers, args.requests, args.inflight
    hdr4 = header[:4]
    dev = torch.device("cuda", 0)
    ERR_CAP = 1024
    DEV_LINES = ("uniform_dev", "uniform_dev_nc", "list_dev", "range_dev")

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(dev)

    def dev_out():
        return {"words": torch.zeros(n // 32, dtype=torch.int64, device=dev),
                "errs": torch.zeros((ERR_CAP, 2), dtype=torch.int32, device=dev),
                "cnt": torch.zeros(1, dtype=torch.int32, device=dev)}

    bufs = []
    for b in range(nb):
        # the ids of the config's checks under the one header (as tools/bench_list.py takes them): the
        # item line and the uniform lines check the same (header, resource id, subject id) triples
        it = checks(100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1).copy()
        for f, v in zip(("resource_type", "permission", "subject_type", "subject_relation", "context_slot"), header):
            it[f] = v
        items = torch.from_numpy(it.view(np.uint8).copy()).to(dev)
        res, sub = it["resource_id"].astype(np.uint32), it["subject_id"].astype(np.uint32)
        pairs = np.stack([res, sub], axis=1)
        h_pairs = eng.host_array(2 * n, np.uint32)
        h_pairs[:] = pairs.reshape(-1)
        first = (b * 40009 + 13) % (n_docs - n) if n_docs > n else 0
        bufs.append({"items": items, "perm": torch.zeros(n, dtype=torch.uint8, device=dev),
                     "err": torch.zeros(n, dtype=torch.int32, device=dev), "pairs": to_dev(pairs), "res": to_dev(res),
                     "res_np": res, "sub0": int(sub[0]), "first": first, "h_pairs": h_pairs,
                     "h_words": eng.host_array(n // 32, np.uint64), "h_errs": eng.host_array(ERR_CAP, E.ITEM_ERROR_DTYPE),
                     "out": {line: dev_out() for line in DEV_LINES}})
    torch.cuda.synchronize()
    cyc = lambda xs: [xs[i % len(xs)] for i in range(k)]
    outp = lambda line, what: cyc([b["out"][line][what].data_ptr() for b in bufs])

    def uniform_loop(line, count):
        return eng.prepare_uniform_device([hdr4] * k, cyc([b["pairs"].data_ptr() for b in bufs]), [n] * k,
                                          outp(line, "words"), outp(line, "errs"), ERR_CAP, depth,
                                          n_errs=outp(line, "cnt") if count else None, engine_streams=True)

    def list_loop(line, ids, first):
        return eng.prepare_list_device([hdr4] * k, cyc([b["sub0"] for b in bufs]), E.VARY_RESOURCE, cyc(ids), cyc(first),
                                       [n] * k, outp(line, "words"), outp(line, "errs"), ERR_CAP, depth,
                                       n_errs=outp(line, "cnt"), engine_streams=True)

    loops = {
        "items": eng.prepare_batches(cyc([b["items"].data_ptr() for b in bufs]), cyc([b["perm"].data_ptr() for b in bufs]),
                                     cyc([b["err"].data_ptr() for b in bufs]), n, depth, engine_streams=True),
        "uniform_dev": uniform_loop("uniform_dev", True),
        "uniform_dev_nc": uniform_loop("uniform_dev_nc", False),
        "list_dev": list_loop("list_dev", [b["res"].data_ptr() for b in bufs], [0] * nb),
        "range_dev": list_loop("range_dev", [0] * nb, [b["first"] for b in bufs]),
        "uniform_host": eng.prepare_uniform([hdr4] * k, cyc([b["h_pairs"].ctypes.data for b in bufs]), [n] * k,
                                            cyc([b["h_words"].ctypes.data for b in bufs]),
                                            cyc([b["h_errs"].ctypes.data for b in bufs]), ERR_CAP, depth),
    }
    order = list(loops)
    assert k >= nb
    d0 = eng.device_compact_stats()
    for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
        loops[line].run()
    torch.cuda.synchronize()
    # agreement, on every request buffer
    words = lambda b, line: b["out"][line]["words"].cpu().numpy().view(np.uint64)
    count = lambda b, line: int(b["out"][line]["cnt"].cpu().numpy().view(np.uint32)[0])
    for b in bufs:
        perm, err = b["perm"].cpu().numpy(), b["err"].cpu().numpy()
        two = np.where(err != 0, 0, perm & 3).astype(np.uint64).reshape(-1, 32)
        packed = (two << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
        assert np.array_equal(words(b, "uniform_dev"), packed), "uniform device and item answers differ"
        assert count(b, "uniform_dev") == int(np.count_nonzero(err)), "uniform device and item error counts differ"
        assert np.array_equal(words(b, "uniform_dev_nc"), packed), "uniform device (no count) and item answers differ"
        assert np.array_equal(np.asarray(b["h_words"]), packed), "host uniform and item answers differ"
        lw, le, _ = eng.check_list(hdr4, b["sub0"], E.VARY_RESOURCE, b["res_np"])
        assert np.array_equal(words(b, "list_dev"), lw) and count(b, "list_dev") == len(le), "list answers differ"
        rw, re_, _ = eng.check_list(hdr4, b["sub0"], E.VARY_RESOURCE, None, b["first"], n)
        assert np.array_equal(words(b, "range_dev"), rw) and count(b, "range_dev") == len(re_), "range answers differ"
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

    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    out = {
        "tool": "bench_device_compact", "config": what, "tuples": n_tuples, "checks_per_request": n, "inflight": depth,
        "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s", "doc_objects": n_docs,
        "lines": {line: line_of(v) for line, v in runs.items()},
        "bytes_per_check_in_out": {"items": [20, 5], "uniform_dev": [8, 0.25], "uniform_dev_nc": [8, 0.25],
                                   "list_dev": [4, 0.25], "range_dev": [0, 0.25], "uniform_host": [8, 0.25]},
        "device_chunks_in_place": d2[0] - d0[0], "device_chunks_expanded": d2[1] - d0[1],
        "device_chunks_timed": (d2[0] - d1[0]) + (d2[1] - d1[1]),
        "deferred_share": {line: (v[0] / v[1] if v[1] else 0.0) for line, v in left.items()},
    }
    m = out["lines"]
    out["uniform_dev_over_items"] = m["uniform_dev"]["median"] / m["items"]["median"]
    out["uniform_dev_minus_items_exceeds_both_spreads"] = (
        m["uniform_dev"]["median"] - m["items"]["median"]
        > max(m["uniform_dev"]["spread_max_minus_min"], m["items"]["spread_max_minus_min"]))
    out["uniform_dev_nc_over_items"] = m["uniform_dev_nc"]["median"] / m["items"]["median"]
    out["range_dev_over_uniform_dev"] = m["range_dev"]["median"] / m["uniform_dev"]["median"]

    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
