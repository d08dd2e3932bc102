#!/usr/bin/env python3
"""Cross requests against the uniform request on one GPU, from pinned host buffers.

Config 2 (tests/synth_configs.py gdocs at --scale; `doc#view@user`) or, with --config nested, a
config-4-shaped graph (tests/synth.py at --tuples; `doc#view@user`). A request's subject and
resource ids are those of the config's own checks. Lines, 65,536 checks per request, --inflight
in flight through the compiled submit/wait loops of libgck_driver.so:

    uniform     the pairs of a 256 x 256 product, 8 B per check
    cross256    the same product as a cross request: 256 + 256 ids
    cross32     32 x 2016 (the widest tile the id block holds)

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds are reported in checks per second. Before any timing the cross and the uniform answers are
compared on every request buffer. Then the lone-request latency, one request at a time: uniform
against cross at 1 x 1024, the median over --lone requests in microseconds. One JSON line out.

    python tools/bench_cross.py [--config gdocs|nested] [--scale 0.2] [--rounds 5] [--out FILE]
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
    ap.add_argument("--lone", type=int, default=300, help="lone requests per latency line")
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

    nb, k = args.buffers, args.requests
    shapes = {"cross256": (256, 256), "cross32": (32, 2016)}
    for S, R in shapes.values():
        assert E.cross_tile(S, R, n) == (S, R), (S, R)

    def ids(seed):
        it = checks(seed).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
        return it["subject_id"].astype(np.uint32), it["resource_id"].astype(np.uint32)

    def cross_buffers(S, R, seed):
        sub, res = ids(seed)
        hs, hr = eng.host_array(S, np.uint32), eng.host_array(R, np.uint32)
        hs[:], hr[:] = sub[:S], res[:R]
        return hs, hr, eng.host_array(S * ((R + 31) // 32), np.uint64), eng.host_array(1024, E.ITEM_ERROR_DTYPE)

    def product_pairs(hs, hr):
        pairs = eng.host_array(2 * len(hs) * len(hr), np.uint32)
        pairs[0::2], pairs[1::2] = np.tile(hr, len(hs)), np.repeat(hs, len(hr))
        return pairs

    bufs = {line: [cross_buffers(S, R, 100 + b) for b in range(nb)] for line, (S, R) in shapes.items()}
    bufs["uniform"] = [(product_pairs(hs, hr), eng.host_array(n // 32, np.uint64), eng.host_array(1024, E.ITEM_ERROR_DTYPE))
                       for hs, hr, _, _ in bufs["cross256"]]
    ptr = lambda xs: [x.ctypes.data for x in xs]
    cyc = lambda xs, m=k: [xs[i % len(xs)] for i in range(m)]

    def cross_loop(bs, m, depth):
        return eng.prepare_cross([header] * m, ptr(cyc([b[0] for b in bs], m)), cyc([len(b[0]) for b in bs], m),
                                 ptr(cyc([b[1] for b in bs], m)), cyc([len(b[1]) for b in bs], m),
                                 ptr(cyc([b[2] for b in bs], m)), ptr(cyc([b[3] for b in bs], m)), 1024, depth)

    def uniform_loop(bs, m, depth):
        return eng.prepare_uniform([header] * m, ptr(cyc([b[0] for b in bs], m)), cyc([len(b[0]) // 2 for b in bs], m),
                                   ptr(cyc([b[1] for b in bs], m)), ptr(cyc([b[2] for b in bs], m)), 1024, depth)

    loops = {"uniform": uniform_loop(bufs["uniform"], k, args.inflight),
             "cross256": cross_loop(bufs["cross256"], k, args.inflight),
             "cross32": cross_loop(bufs["cross32"], k, args.inflight)}
    order = ["uniform", "cross256", "cross32"]
    c0 = eng.cross_stats()
    for line in order:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
        loops[line].run()
    assert k >= nb
    # agreement, on every request buffer: the 256 x 256 plane has no padding, so its words are the
    # uniform request's; the 32 x 2016 plane against a uniform request of its product
    for (hs, hr, plane, _), (_, words, _) in zip(bufs["cross256"], bufs["uniform"]):
        assert np.array_equal(np.asarray(plane), np.asarray(words)), "cross256 and uniform answers differ"
    for hs, hr, plane, _ in bufs["cross32"]:
        words, errs, _ = eng.check_uniform(header, np.asarray(product_pairs(hs, hr)).reshape(-1, 2))
        assert np.array_equal(E.unpack_cross(plane, len(hs), len(hr)).reshape(-1), E.unpack_results(words, n))
    runs = {line: [] for line in order}
    for _ in range(args.rounds):
        for line in order:
            runs[line].append(k * n / loops[line].run())
    c1 = eng.cross_stats()

    # lone-request latency: one request at a time, 1 x 1024
    lone_cross = [cross_buffers(1, 1024, 300 + b) for b in range(nb)]
    lone_uni = [(product_pairs(hs, hr), eng.host_array(32, np.uint64), eng.host_array(1024, E.ITEM_ERROR_DTYPE))
                for hs, hr, _, _ in lone_cross]
    lone = {}
    for name, mk, bs in (("uniform", uniform_loop, lone_uni), ("cross", cross_loop, lone_cross)):
        one = [mk([b], 1, 1) for b in bs]
        for p in one:
            p.run()
        lone[name] = [one[i % nb].run() * 1e6 for i in range(args.lone)]
    for (_, _, plane, _), (_, words, _) in zip(lone_cross, lone_uni):
        assert np.array_equal(np.asarray(plane), np.asarray(words)), "lone cross and uniform answers differ"

    st = eng.stats()
    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    out = {
        "tool": "bench_cross", "config": what, "tuples": n_tuples, "checks_per_request": n, "inflight": args.inflight,
        "timed_requests_per_run": k, "rounds": args.rounds, "unit": "checks/s",
        "lines": {line: line_of(v) for line, v in runs.items()},
        "bytes_in_per_check": {"uniform": 8.0, "cross256": 4 * 512 / n, "cross32": 4 * 2048 / (32 * 2016)},
        "lone_1x1024_us": {name: {"median": statistics.median(v), "p10": float(np.percentile(v, 10)),
                                  "p90": float(np.percentile(v, 90)), "requests": len(v)} for name, v in lone.items()},
        "cross_tiles_in_place": c1[0] - c0[0], "cross_chunks_expanded": c1[1] - c0[1],
        "deferred_checks_total": int(st["deferred"]),
    }
    m = out["lines"]
    out["cross256_over_uniform"] = m["cross256"]["median"] / m["uniform"]["median"]
    out["cross256_minus_uniform_exceeds_both_spreads"] = (
        m["cross256"]["median"] - m["uniform"]["median"]
        > max(m["cross256"]["spread_max_minus_min"], m["uniform"]["spread_max_minus_min"]))
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
