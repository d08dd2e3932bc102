#!/usr/bin/env python3
"""Host-buffer request formats side by side on one GPU: 20-B items, a uniform request, a shaped
request with one shape and a shaped request with four interleaved shapes.

Config 2 (tests/synth_configs.py gdocs at --scale): `doc#view@user` is the one shape of the uniform
and one-shape lines; the four shapes are doc#view, doc#edit, folder#view and folder#edit for a
user, a shape drawn per check. Every line runs through the compiled submit/wait loops of
libgck_driver.so from pinned host buffers, --checks per request, --inflight in flight, --requests
timed requests per run. The four lines alternate within each of --rounds rounds; per line the
median and max - min over the rounds are reported, in checks per second, as one JSON line.

    python tools/bench_shaped.py [--scale 0.2] [--rounds 5] [--requests 200] [--out FILE]
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
    ap.add_argument("--scale", type=float, default=0.2, help="config 2 at this scale (1.0 = 10M tuples)")
    ap.add_argument("--checks", type=int, default=65536)
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=16, help="distinct request buffers the loops cycle through")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gochugaru_amd import engine as E
    from tests import synth_configs

    E.pin_to_device_node(0)
    W = synth_configs.gdocs(args.scale, device="cuda")
    eng = E.Engine(device=0, max_batch=args.checks, workspaces=args.inflight)
    eng.load_schema(W.schema)
    eng.begin_snapshot(1)
    for t, cnt in W.counts.items():
        eng.reserve_objects(W.t(t), cnt)
    keep = []
    for rel, st, sr, n_rows, off, nbr in W.csrs:
        off32, nbr32 = off.to(torch.int32).contiguous(), nbr.contiguous()
        keep.append((off32, nbr32))
        eng.load_csr(rel, st, sr, n_rows, off32.data_ptr(), nbr32.data_ptr(), nbr32.numel(), device=True)
    eng.commit_snapshot()
    torch.cuda.synchronize()

    n, nb = args.checks, args.buffers
    t_user = W.t("user")
    names = ["doc#view@user", "doc#edit@user", "folder#view@user", "folder#edit@user"]
    shapes = [(W.t(r), W.r(r, p), t_user, E.ELLIPSIS, 0) for r, p in (s.split("@")[0].split("#") for s in names)]
    rng = np.random.default_rng(20251003)

    def doc_items(seed):  # config 2's own checks (doc#view|edit@user, half likely positive)
        return synth_configs.checks(W, n, seed=seed).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1).copy()

    def request(seed, which):
        """Items of one request whose check k has shape shapes[which[k]]."""
        it = doc_items(seed)
        folder = which >= 2
        it["resource_id"][folder] = rng.integers(0, W.counts["folder"], int(folder.sum()))
        for j, s in enumerate(shapes):
            m = which == j
            it["resource_type"][m], it["permission"][m] = s[0], s[1]
        return it

    bufs = {"items": [], "uniform": [], "shaped1": [], "shaped4": []}
    for b in range(nb):
        one = request(100 + b, np.zeros(n, dtype=np.int64))
        four_of = rng.integers(0, 4, n)
        four = request(200 + b, four_of)
        h_items = eng.host_array(n, E.ITEM_DTYPE)
        h_items[:] = four
        bufs["items"].append((h_items, eng.host_array(n, np.uint8), eng.host_array(n, np.int32)))
        for line, it, of in (("uniform", one, None), ("shaped1", one, np.zeros(n, np.uint8)),
                             ("shaped4", four, four_of.astype(np.uint8))):
            pairs = eng.host_array(2 * n, np.uint32)
            pairs[0::2], pairs[1::2] = it["resource_id"], it["subject_id"]
            idx = eng.host_array(n, np.uint8)
            if of is not None:
                idx[:] = of
            bufs[line].append((pairs, idx, eng.host_array((n + 31) // 32, np.uint64),
                               eng.host_array(n, E.ITEM_ERROR_DTYPE)))

    k = args.requests
    ptr = lambda xs: [x.ctypes.data for x in xs]
    cyc = lambda xs: [xs[i % nb] for i in range(k)]
    loops = {
        "items": eng.prepare_batches(ptr(cyc([b[0] for b in bufs["items"]])), ptr(cyc([b[1] for b in bufs["items"]])),
                                     ptr(cyc([b[2] for b in bufs["items"]])), n, args.inflight, host=True),
        "uniform": eng.prepare_uniform([shapes[0]] * k, ptr(cyc([b[0] for b in bufs["uniform"]])), [n] * k,
                                       ptr(cyc([b[2] for b in bufs["uniform"]])),
                                       ptr(cyc([b[3] for b in bufs["uniform"]])), n, args.inflight),
        "shaped1": eng.prepare_shaped([shapes[:1]] * k, ptr(cyc([b[1] for b in bufs["shaped1"]])),
                                      ptr(cyc([b[0] for b in bufs["shaped1"]])), [n] * k,
                                      ptr(cyc([b[2] for b in bufs["shaped1"]])),
                                      ptr(cyc([b[3] for b in bufs["shaped1"]])), n, args.inflight),
        "shaped4": eng.prepare_shaped([shapes] * k, ptr(cyc([b[1] for b in bufs["shaped4"]])),
                                      ptr(cyc([b[0] for b in bufs["shaped4"]])), [n] * k,
                                      ptr(cyc([b[2] for b in bufs["shaped4"]])),
                                      ptr(cyc([b[3] for b in bufs["shaped4"]])), n, args.inflight),
    }
    order = ["items", "uniform", "shaped1", "shaped4"]
    s0 = eng.shaped_stats()
    for line in order:  # warm-up: one untimed run each
        loops[line].run()
    # the formats agree on the warm-up's answers: the four-shape request against its items
    perm, err = bufs["items"][0][1], bufs["items"][0][2]
    got = E.unpack_results(bufs["shaped4"][0][2], n)
    assert np.array_equal(got, np.where(err == 0, perm, 0)), "shaped and item results differ"
    runs = {line: [] for line in order}
    for _ in range(args.rounds):
        for line in order:
            secs = loops[line].run()
            runs[line].append(k * n / secs)
    s1 = eng.shaped_stats()
    st = eng.stats()
    out = {
        "tool": "bench_shaped", "config": f"config 2 (gdocs) at scale {args.scale}", "tuples": W.n_tuples,
        "checks_per_request": n, "inflight": args.inflight, "timed_requests_per_run": k, "rounds": args.rounds,
        "shapes": names, "unit": "checks/s",
        "lines": {line: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
                  for line, v in runs.items()},
        "shaped_requests_in_place": s1[0] - s0[0], "shaped_requests_expanded": s1[1] - s0[1],
        "deferred_checks_total": int(st["deferred"]),
    }
    m = out["lines"]
    out["shaped4_over_items"] = m["shaped4"]["median"] / m["items"]["median"]
    out["shaped4_over_uniform"] = m["shaped4"]["median"] / m["uniform"]["median"]
    out["shaped4_minus_items_exceeds_items_spread"] = (
        m["shaped4"]["median"] - m["items"]["median"] > m["items"]["spread_max_minus_min"])
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
