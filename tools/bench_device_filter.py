#!/usr/bin/env python3
"""Filter requests (gck_filter_list_device) against the list device request on one GPU.

Config 2 (tests/synth_configs.py gdocs at --scale; `doc#view@user`) or, with --config nested, a
config-4-shaped graph (tests/synth.py at --tuples). One subject against 65,536 candidate documents
per request, --inflight in flight on the engine's workspace streams, --requests timed requests per
run. The candidates are chosen from the host lookup's answer for the subject (every document of the
type it may see, and those it may not), so that about --shares of them survive; the realised share
is reported. Lines, per share:

    list_dev     gckd_run_list_device alone: the plane and nothing else (the ceiling: no select runs)
    filter_ids   gckd_run_filter_device, surviving ids only, no plane of the caller's
    filter_all   the same with ids + positions + Permissionships
    torch_plane  what a caller does without the filter call: submit_list_device, and after each wait
                 torch ops on the plane (shift, mask, compare, boolean index) that produce the same
                 id tensor. A Python loop with the same number in flight — NOT a compiled loop.

The lines alternate within each of --rounds rounds; per line the median and max - min over the
rounds, in candidates per second. Before any timing filter_ids' and torch_plane's survivors are
compared with the host lookup's on every request buffer. Also: a lone request's median latency
(one in flight, --lone requests) for list_dev, filter_ids and torch_plane. One JSON line out.

    python tools/bench_device_filter.py [--config gdocs|nested] [--scale 0.2] [--out FILE]
"""
import argparse
import collections
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
    ap.add_argument("--shares", default="0.01,0.5,1.0")
    ap.add_argument("--inflight", type=int, default=8)
    ap.add_argument("--requests", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lone", type=int, default=50)
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
    ERR_CAP = 64
    rng = np.random.default_rng(5)
    now_us = time.time_ns() // 1000
    shifts = torch.arange(0, 64, 2, dtype=torch.int64, device=dev)

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(dev)

    def lookup(sub, cand):
        return eng.lookup_resources_among(header[0], header[1], header[2], header[3], sub, cand, now_us=now_us)[0]

    # per buffer: a subject of the config's checks that may see some documents and not others, and
    # the host lookup's answer over a pool of the type's documents (the first 2^20 at the most)
    subjects = []
    it = checks(100).cpu().numpy().view(E.ITEM_DTYPE).reshape(-1)
    pool = np.arange(min(n_docs, 1 << 20), dtype=np.uint32)
    for sub in np.unique(it["subject_id"].astype(np.uint32))[:64 * nb]:
        yes = lookup(int(sub), pool).astype(np.uint32)
        if 0 < len(yes) < len(pool):
            subjects.append((int(sub), yes, np.setdiff1d(pool, yes)))
        if len(subjects) == nb:
            break
    assert subjects, "no subject sees some documents of the pool and not others"

    def torch_select(words, ids):
        """The survivors of a plane by torch ops: unpack the 2-bit fields, keep HAS and CONDITIONAL."""
        v = (words.unsqueeze(1) >> shifts) & 3
        return ids[(v >= 2).reshape(-1)[:ids.numel()]]

    def torch_loop(bufs, kk, dd):
        """kk list device requests, dd in flight, each followed by torch_select (a Python loop)."""
        q = collections.deque()
        got = [None] * len(bufs)
        t0 = time.perf_counter()
        for i in range(kk):
            if len(q) >= dd:
                j, b = q.popleft()
                b.wait()
                got[j] = torch_select(bufs[j]["tw"], bufs[j]["ids"])
            j = i % len(bufs)
            q.append((j, eng.submit_list_device(hdr4, bufs[j]["sub"], E.VARY_RESOURCE, n, bufs[j]["tw"].data_ptr(),
                                                d_ids=bufs[j]["ids"].data_ptr(), engine_stream=True, now_us=now_us)))
        while q:
            j, b = q.popleft()
            b.wait()
            got[j] = torch_select(bufs[j]["tw"], bufs[j]["ids"])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, got

    line_of = lambda v: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
    out = {"tool": "bench_device_filter", "config": what, "tuples": n_tuples, "candidates_per_request": n,
           "inflight": depth, "timed_requests_per_run": k, "rounds": args.rounds, "unit": "candidates/s",
           "doc_objects": n_docs, "torch_plane_is_a_python_loop": True, "shares": {}}
    for share in [float(s) for s in args.shares.split(",")]:
        bufs = []
        for b in range(nb):
            sub, yes, no = subjects[b % len(subjects)]
            pick = rng.random(n) < share
            cand = np.where(pick, yes[rng.integers(0, len(yes), n)], no[rng.integers(0, len(no), n)]).astype(np.uint32)
            bufs.append({"sub": sub, "cand": cand, "ids": to_dev(cand), "want": lookup(sub, cand),
                         "words": torch.zeros(n // 32, dtype=torch.int64, device=dev),
                         "tw": torch.zeros(n // 32, dtype=torch.int64, device=dev),
                         "errs": torch.zeros((ERR_CAP, 2), dtype=torch.int32, device=dev),
                         "cnt": torch.zeros(4, dtype=torch.int32, device=dev),
                         "o_ids": [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)],
                         "o_pos": torch.zeros(n, dtype=torch.int32, device=dev),
                         "o_perm": torch.zeros(n, dtype=torch.uint8, device=dev)})
        torch.cuda.synchronize()
        realised = sum(len(b["want"]) for b in bufs) / (n * nb)

        def loops_for(kk, dd):
            cyc = lambda xs: [xs[i % len(xs)] for i in range(kk)]
            ptr = lambda f: cyc([f(b).data_ptr() for b in bufs])
            common = ([hdr4] * kk, cyc([b["sub"] for b in bufs]), E.VARY_RESOURCE, ptr(lambda b: b["ids"]), [0] * kk,
                      [n] * kk)
            tail = dict(errs=ptr(lambda b: b["errs"]), err_cap=ERR_CAP, engine_streams=True, now_us=now_us)
            cnt = lambda at: cyc([b["cnt"].data_ptr() + 4 * at for b in bufs])
            return {
                "list_dev": eng.prepare_list_device(*common, ptr(lambda b: b["words"]), tail["errs"], ERR_CAP, dd,
                                                    n_errs=cnt(0), engine_streams=True, now_us=now_us),
                "filter_ids": eng.prepare_filter_device(*common, cnt(1), n, dd, out_ids=ptr(lambda b: b["o_ids"][0]),
                                                        n_errs=cnt(0), **tail),
                "filter_all": eng.prepare_filter_device(*common, cnt(2), n, dd, out_ids=ptr(lambda b: b["o_ids"][1]),
                                                        out_pos=ptr(lambda b: b["o_pos"]),
                                                        out_perm=ptr(lambda b: b["o_perm"]), n_errs=cnt(0), **tail),
            }

        loops = loops_for(k, depth)
        order = list(loops) + ["torch_plane"]
        assert k >= nb
        for line in loops:  # warm-up: one untimed run each (k >= the buffers: every buffer is answered)
            loops[line].run()
        _, tgot = torch_loop(bufs, k, depth)
        torch.cuda.synchronize()
        # agreement with the host lookup, on every request buffer
        for j, b in enumerate(bufs):
            cnts = b["cnt"].cpu().numpy().view(np.uint32)
            assert cnts[0] == 0, "a candidate has a per-item error"
            for at, o in ((1, b["o_ids"][0]), (2, b["o_ids"][1])):
                assert cnts[at] == len(b["want"]), "filter and host lookup counts differ"
                assert np.array_equal(o[:cnts[at]].cpu().numpy().view(np.uint32), b["want"]), "filter and host lookup differ"
            assert np.array_equal(tgot[j].cpu().numpy().view(np.uint32), b["want"]), "torch ops and host lookup differ"
            m = int(cnts[2])
            assert np.array_equal(b["cand"][b["o_pos"][:m].cpu().numpy()], b["want"]), "positions do not gather the ids"
        runs = {line: [] for line in order}
        for _ in range(args.rounds):
            for line in order:
                secs = loops[line].run() if line in loops else torch_loop(bufs, k, depth)[0]
                runs[line].append(k * n / secs)
        lone_loops = loops_for(1, 1)
        lone = {line: [] for line in ("list_dev", "filter_ids", "torch_plane")}
        for _ in range(args.lone):
            for line in lone:
                secs = lone_loops[line].run() if line in lone_loops else torch_loop(bufs[:1], 1, 1)[0]
                lone[line].append(secs * 1e6)
        m = {line: line_of(v) for line, v in runs.items()}
        two = lambda x, y: max(m[x]["spread_max_minus_min"], m[y]["spread_max_minus_min"])
        out["shares"][str(share)] = {
            "realised_share": realised, "lines": m,
            "lone_request_median_us": {line: statistics.median(v) for line, v in lone.items()},
            "filter_ids_over_torch_plane": m["filter_ids"]["median"] / m["torch_plane"]["median"],
            "filter_ids_minus_torch_plane_exceeds_both_spreads":
                m["filter_ids"]["median"] - m["torch_plane"]["median"] > two("filter_ids", "torch_plane"),
            "filter_ids_over_list_dev": m["filter_ids"]["median"] / m["list_dev"]["median"],
            "filter_ids_below_half_of_list_dev": m["filter_ids"]["median"] < 0.5 * m["list_dev"]["median"],
            "us_per_request_added_by_the_select":  # (of the loop's wall time, `inflight` requests overlapping)
                n * (1 / m["filter_ids"]["median"] - 1 / m["list_dev"]["median"]) * 1e6,
        }

    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
