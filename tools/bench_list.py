#!/usr/bin/env python3
"""List requests against the uniform request on one GPU, from pinned host buffers.

Config 2 (tests/synth_configs.py gdocs at --scale; `doc#view@user`) or, with --config nested, a
config-4-shaped graph (tests/synth.py at --tuples; `doc#view@user`). A request is one id of the
config's own checks on the fixed side and 65,536 ids on the other. Lines, --inflight in flight
through the compiled submit/wait loops of libgck_driver.so:

    uniform       one subject against the resource ids of the config's checks, as pairs: 8 B per check
    list_res      the same checks as a list request, VARY_RESOURCE: 4 B per check
    range         one subject against 65,536 consecutive resource ids, as a range: 0 B per check
    list_sorted   the range's checks as a list request (what the range saves beyond the id order)
    list_sub      one resource against the subject ids of the config's checks, VARY_SUBJECT

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds are reported in checks per second. Before any timing the answers are compared on every
request buffer: list_res with uniform, range with list_sorted and with a uniform request of its
pairs, list_sub with a uniform request of its pairs. With --lookup, the whole-type lookup: for
one subject, gck_lookup_resources against gck_lookup_resources_among without candidates over the
`doc` type, --lookup calls each, alternated; equal results, the median times and their ratio.
One JSON line out.

    python tools/bench_list.py [--config gdocs|nested] [--scale 0.2] [--rounds 5] [--lookup 10] [--out FILE]
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
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=16, help="distinct request buffers the loops cycle through")
    ap.add_argument("--lookup", type=int, default=0, help="whole-type lookups per line (0: skip)")
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

    nb, k = args.buffers, args.requests
    R, S = E.VARY_RESOURCE, E.VARY_SUBJECT
    hdr4 = header[:4]

    def out_buffers():
        return eng.host_array(n // 32, np.uint64), eng.host_array(1024, E.ITEM_ERROR_DTYPE)

    def pinned(a, dtype=np.uint32):
        h = eng.host_array(len(a), dtype)
        h[:] = a
        return h

    def pairs_of(res, sub):
        p = eng.host_array(2 * n, np.uint32)
        p[0::2], p[1::2] = res, sub
        return p

    # a buffer: the fixed ids, the id lists, the range's first id, and per line its outputs
    bufs = []
    for b in range(nb):
        it = checks(100 + b).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
        sub, res = it["subject_id"].astype(np.uint32), it["resource_id"].astype(np.uint32)
        first = (b * 40009 + 13) % (n_docs - n) if n_docs > n else 0
        seq = np.arange(first, first + n, dtype=np.uint64).astype(np.uint32)
        bufs.append({"sub0": int(sub[0]), "res0": int(res[0]), "first": first, "res": pinned(res), "sub": pinned(sub),
                     "seq": pinned(seq), "pairs": pairs_of(res, np.full(n, sub[0], dtype=np.uint32)),
                     "out": {line: out_buffers() for line in ("uniform", "list_res", "range", "list_sorted", "list_sub")}})
    ptr = lambda xs: [x.ctypes.data for x in xs]
    cyc = lambda xs: [xs[i % len(xs)] for i in range(k)]

    def list_loop(line, fixed, vary, ids, first):
        return eng.prepare_list([hdr4] * k, cyc(fixed), vary, cyc(ids), cyc(first), [n] * k,
                                ptr(cyc([b["out"][line][0] for b in bufs])), ptr(cyc([b["out"][line][1] for b in bufs])),
                                1024, args.inflight)

    zeros = [0] * nb
    loops = {
        "uniform": eng.prepare_uniform([hdr4] * k, ptr(cyc([b["pairs"] for b in bufs])), [n] * k,
                                       ptr(cyc([b["out"]["uniform"][0] for b in bufs])),
                                       ptr(cyc([b["out"]["uniform"][1] for b in bufs])), 1024, args.inflight),
        "list_res": list_loop("list_res", [b["sub0"] for b in bufs], R, ptr([b["res"] for b in bufs]), zeros),
        "range": list_loop("range", [b["sub0"] for b in bufs], R, zeros, [b["first"] for b in bufs]),
        "list_sorted": list_loop("list_sorted", [b["sub0"] for b in bufs], R, ptr([b["seq"] for b in bufs]), zeros),
        "list_sub": list_loop("list_sub", [b["res0"] for b in bufs], S, ptr([b["sub"] for b in bufs]), zeros),
    }
    order = list(loops)
    l0 = eng.list_stats()
    assert k >= nb
    for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
        loops[line].run()
    # agreement, on every request buffer
    words = lambda b, line: np.asarray(b["out"][line][0])
    for b in bufs:
        assert np.array_equal(words(b, "list_res"), words(b, "uniform")), "list and uniform answers differ"
        assert np.array_equal(words(b, "range"), words(b, "list_sorted")), "range and list answers differ"
        fx = np.full(n, b["sub0"], dtype=np.uint32)
        uw, _, _ = eng.check_uniform(hdr4, np.stack([np.asarray(b["seq"]), fx], axis=1))
        assert np.array_equal(words(b, "range"), uw), "range and uniform answers differ"
        fx = np.full(n, b["res0"], dtype=np.uint32)
        uw, _, _ = eng.check_uniform(hdr4, np.stack([fx, np.asarray(b["sub"])], axis=1))
        assert np.array_equal(words(b, "list_sub"), uw), "list (VARY_SUBJECT) and uniform answers differ"
    runs = {line: [] for line in order}
    for _ in range(args.rounds):
        for line in order:
            runs[line].append(k * n / loops[line].run())
    l1 = eng.list_stats()

    st = eng.stats()
    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    out = {
        "tool": "bench_list", "config": what, "tuples": n_tuples, "checks_per_request": n, "inflight": args.inflight,
        "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s", "doc_objects": n_docs,
        "lines": {line: line_of(v) for line, v in runs.items()},
        "bytes_in_per_check": {"uniform": 8.0, "list_res": 4.0, "range": 0.0, "list_sorted": 4.0, "list_sub": 4.0},
        "list_chunks_in_place": l1[0] - l0[0], "list_chunks_expanded": l1[1] - l0[1],
        "deferred_checks_total": int(st["deferred"]),
    }
    m = out["lines"]
    out["list_res_over_uniform"] = m["list_res"]["median"] / m["uniform"]["median"]
    out["list_res_minus_uniform_exceeds_both_spreads"] = (
        m["list_res"]["median"] - m["uniform"]["median"]
        > max(m["list_res"]["spread_max_minus_min"], m["uniform"]["spread_max_minus_min"]))
    out["range_over_list_res"] = m["range"]["median"] / m["list_res"]["median"]

    if args.lookup:
        # the whole-type lookup for one subject: the sweep of gck_lookup_resources against one range
        sid = bufs[0]["sub0"]
        t_old, t_new, res = [], [], {}
        for i in range(args.lookup + 1):  # (the first pair is the warm-up)
            for name, fn, ts in (("lookup_resources", lambda: eng.lookup_resources(*hdr4, sid), t_old),
                                 ("lookup_resources_among", lambda: eng.lookup_resources_among(*hdr4, sid, None), t_new)):
                t0 = time.perf_counter()
                ids, perms = fn()
                dt = time.perf_counter() - t0
                if i:
                    ts.append(dt * 1e3)
                res[name] = (np.array(ids), np.array(perms))
            assert np.array_equal(res["lookup_resources"][0], res["lookup_resources_among"][0]), "lookup ids differ"
            assert np.array_equal(res["lookup_resources"][1], res["lookup_resources_among"][1]), "lookup perms differ"
        out["whole_type_lookup_ms"] = {
            "objects": n_docs, "matches": int(len(res["lookup_resources"][0])), "calls": args.lookup,
            "lookup_resources": {"median": statistics.median(t_old), "min": min(t_old), "max": max(t_old)},
            "lookup_resources_among": {"median": statistics.median(t_new), "min": min(t_new), "max": max(t_new)},
            "old_over_new": statistics.median(t_old) / statistics.median(t_new)}

    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
