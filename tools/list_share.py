"""What share of the flagship's checks and 32-check waves reach the closure join's cover-list round
(closure.inc round 1b), predicted on the host from tests/synth.py at a given scale: numpy, no GPU.

    python tools/list_share.py [--tuples 2e7] [--seeds 1000 1001] [--bits 24] [--device cpu]

Builds the synthetic graph on the CPU, the tree labels (first parent = lowest id, children in id
order) and pruned covers per group as DESIGN §3.1 defines them, and for every check of
synth.checks(G, 65536, seed) — bench.py's batches — the user's concatenated cover entries. Three
layouts of a user slot are counted (gochugaru_amd/csrc/slot_pack.hpp):
  raw      a user with more raw entries than a slot holds is listed (before this layout)
  dedup    ... with more sorted unique entries than a slot holds
  window   ... and neither an inline entry nor the omitted window decides the check
The timing build's phase dump (tools/analyze_cj.py, "list round (1b)") reports the same two
shares from the device. Beside them, `front_flag`: the checks whose document's 16-B front (slot_pack.hpp
front_pack) says "read the slot" — more than 3 viewer groups, or a group whose interval is longer
than 2^18 - 1 labels or starts at 2^24 or later — and the waves that hold one (analyze_cj.py,
"flagged fronts"). torch's CPU and GPU generators give different graphs from one seed, and
the heavy tail of the group sizes moves the shares from instance to instance (raw: 5.2 % of the
checks at 2e7 tuples, 3.4 % at 1e8, 4.1 % at 4e8, 4.2 % at 1e9, all on the CPU), so a prediction
for the graph the device runs is made with --device cuda: the graph and the checks are generated
there and everything else runs on the host. The group loop is plain Python: 7 s at 2e7 tuples, 3 minutes at 4e8; 1e9 needs some 50 GB of host memory."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CAP = {24: 20, 32: 15}
SORT_MAX = 64
CPW = 32  # checks per wave of the flagship variant
FRONT_V, FRONT_LEN_MAX, FRONT_START_END = 3, (1 << 18) - 1, 1 << 24  # slot_pack.hpp kFrontV, kFrontLenMax, 24-bit starts


def labels_and_covers(n_groups, g_off, g_nbr):
    """pre, end per group and the cover (a tuple of group ids) per group."""
    par_of = [[] for _ in range(n_groups)]
    rows = np.repeat(np.arange(n_groups), np.diff(g_off))
    for p, c in zip(rows.tolist(), g_nbr.tolist()):
        par_of[c].append(p)
    tree_par = np.array([min(ps) if ps else -1 for ps in par_of], dtype=np.int64)
    size = np.ones(n_groups, dtype=np.int64)
    for g in range(n_groups - 1, -1, -1):  # (a parent's id is below its children's: layers)
        if tree_par[g] >= 0:
            size[tree_par[g]] += size[g]
    pre = np.zeros(n_groups, dtype=np.int64)
    nxt = np.zeros(n_groups, dtype=np.int64)  # next free preorder number under each group
    at = 0
    for g in range(n_groups):  # (id order: a parent is numbered before its children)
        p = tree_par[g]
        if p < 0:
            pre[g] = at
            at += size[g]
        else:
            pre[g] = nxt[p]
            nxt[p] += size[g]
        nxt[g] = pre[g] + 1
    end = pre + size
    cover = [None] * n_groups
    for g in range(n_groups):
        ent = {g}
        for p in par_of[g]:
            ent.update(cover[p])
        if len(ent) > 1:
            ent = [a for a in ent if not any(b != a and pre[a] <= pre[b] < end[a] for b in ent)]
        cover[g] = tuple(ent)
    return pre, end, cover


def window(e, n_in):
    n_om = len(e) - n_in
    best, best_w = 0, 1 << 40
    for s in range(n_in + 1):
        lo1 = e[s - 1] + 1 if s else 0
        hi = e[s + n_om] if s + n_om < len(e) else 0xFFFFFFFF
        if hi - lo1 < best_w:
            best, best_w = s, hi - lo1
    lo1 = e[best - 1] + 1 if best else 0
    hi = e[best + n_om] if best + n_om < len(e) else 0xFFFFFFFF
    return best, lo1, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuples", type=float, default=2e7)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1000, 1001])
    ap.add_argument("--bits", type=int, default=24, choices=[24, 32])
    ap.add_argument("--device", default="cpu", help="where tests/synth.py generates the graph and the checks")
    a = ap.parse_args()
    from tests import synth

    G = synth.build(a.tuples, device=a.device)
    host = lambda t: t.cpu().numpy()
    g_off, g_nbr = host(G.mem_group_off), host(G.mem_group_nbr).astype(np.int64)
    u_off, u_nbr = host(G.mem_user_off), host(G.mem_user_nbr)  # (int32: a billion entries at full scale)
    v_off, v_nbr = host(G.viewer_off), host(G.viewer_nbr).astype(np.int64)
    pre, end, cover = labels_and_covers(G.n_groups, g_off, g_nbr)
    cov_n = np.array([len(c) for c in cover])
    order = np.argsort(u_nbr, kind="stable")  # the transposed member CSR, for the checked users
    sorted_users = u_nbr[order]
    group_of = np.repeat(np.arange(G.n_groups, dtype=np.int32), np.diff(u_off))[order]
    del order
    cap, n_in = CAP[a.bits], CAP[a.bits] - 2
    tot = {k: [0, 0] for k in ("raw", "dedup", "window", "front_flag")}  # listed / flagged checks, waves with one
    unfit = np.concatenate([[0], np.cumsum(((end - pre > FRONT_LEN_MAX) | (pre >= FRONT_START_END))[v_nbr])])
    n_checks = n_waves = 0
    raw_sizes = []
    for seed in a.seeds:
        items = host(synth.checks(G, 65536, seed=seed)).view(np.uint32).reshape(-1, 5)
        docs, users = items[:, 1].astype(np.int64), items[:, 3].astype(np.int64)
        b, e_ = np.searchsorted(sorted_users, users, "left"), np.searchsorted(sorted_users, users, "right")
        flags = {k: np.zeros(len(users), dtype=bool) for k in tot}
        flags["front_flag"] = (v_off[docs + 1] - v_off[docs] > FRONT_V) | (unfit[v_off[docs + 1]] - unfit[v_off[docs]] > 0)
        for i in range(len(users)):
            gs = group_of[b[i]:e_[i]]
            raw = [int(pre[c]) for g in gs for c in cover[g]]
            raw_sizes.append(len(raw))
            if len(raw) <= cap:
                continue
            flags["raw"][i] = True
            if len(raw) > SORT_MAX:
                flags["dedup"][i] = flags["window"][i] = True
                continue
            e = sorted(set(raw))
            if len(e) <= cap:
                continue
            flags["dedup"][i] = True
            s, lo1, hi = window(e, n_in)
            inline = e[:s] + e[s + len(e) - n_in:]
            iv = [(int(pre[v]), int(end[v])) for v in v_nbr[v_off[docs[i]]:v_off[docs[i] + 1]]]
            hit = any(p <= x < q for p, q in iv for x in inline)
            reach = any(p < hi and q > lo1 for p, q in iv)
            flags["window"][i] = not hit and reach
        n_checks += len(users)
        n_waves += len(users) // CPW
        for k, f in flags.items():
            tot[k][0] += int(f.sum())
            tot[k][1] += int(f.reshape(-1, CPW).any(axis=1).sum())
    rs = np.array(raw_sizes)
    print(json.dumps({
        "tuples": G.n_tuples, "device": a.device, "groups": G.n_groups, "bits": a.bits, "checks": n_checks,
        "cover_entries_per_group": {"mean": round(float(cov_n.mean()), 2), "max": int(cov_n.max())},
        "raw_entries_per_checked_user": {"mean": round(float(rs.mean()), 2), "p99": int(np.percentile(rs, 99)),
                                         "max": int(rs.max())},
        **{k: {"checks_pct": round(100.0 * v[0] / n_checks, 2), "waves_pct": round(100.0 * v[1] / n_waves, 1)}
           for k, v in tot.items()}}))


if __name__ == "__main__":
    main()
