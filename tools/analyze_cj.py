"""Per-wave phase timing of k_closure_join (GCK_DEBUG_TIMING=<prefix> with the TIMING=1 build
writes <prefix>_cj.bin): where a launch's time goes. wall_clock64 ticks at 100 MHz (10 ns)."""
import sys

import numpy as np

TICK_US = 0.01
W = 12  # closure.inc kCjTimingWords


def launches(path):
    raw = np.fromfile(path, dtype=np.uint64)
    at = 0
    while at + 2 <= raw.size:
        assert raw[at] == 0xC10C, "bad record"
        nw = int(raw[at + 1])
        rec = raw[at + 2: at + 2 + W * nw].reshape(nw, W).astype(np.int64)
        at += 2 + W * nw
        yield rec


def pct(x):
    return " ".join(f"{q}:{np.percentile(x, q):7.2f}" for q in (10, 50, 90, 99, 100))


def list_round(recs):
    """Word 7 of a wave's record: its decided checks in the low half, its checks that went into the
    cover-list round (round 1b) in the high half. Returns (share of waves with a list round, share
    of checks in it, median `lists` phase in us of the waves with one, of the waves without)."""
    a = np.concatenate(recs)
    n_take, n_list = a[:, 7] & 0xFFFFFFFF, a[:, 7] >> 32
    with_l = n_list > 0
    lists_us = (a[:, 9] - a[:, 10]) * TICK_US
    med = lambda m: float(np.median(lists_us[m])) if m.any() else float("nan")
    return (float(with_l.mean()), float(n_list.sum() / max(1, n_take.sum())), med(with_l), med(~with_l))


def front_flags(recs):
    """Word 11 of a wave's record: its checks whose 16-B resource front said "read the slot" (0
    without fronts). Returns (share of waves with such a check, share of checks)."""
    a = np.concatenate(recs)
    n_take, n_flag = a[:, 7] & 0xFFFFFFFF, a[:, 11]
    return float((n_flag > 0).mean()), float(n_flag.sum() / max(1, n_take.sum()))


def main(path):
    spans, recs, raw = [], [], []
    for r in launches(path):
        r = r[r[:, 0] > 0]
        raw.append(r)
        t0 = r[:, 0].min()
        spans.append((r[:, 4].max() - t0) * TICK_US)
        recs.append(np.column_stack([(r[:, 0] - t0) * TICK_US, (r[:, 1] - r[:, 0]) * TICK_US,
                                     (r[:, 8] - r[:, 1]) * TICK_US, (r[:, 10] - r[:, 8]) * TICK_US,
                                     (r[:, 9] - r[:, 10]) * TICK_US,
                                     (r[:, 2] - r[:, 9]) * TICK_US, (r[:, 3] - r[:, 2]) * TICK_US,
                                     (r[:, 4] - r[:, 3]) * TICK_US, (r[:, 4] - t0) * TICK_US,
                                     r[:, 5], r[:, 6], r[:, 7] & 0xFFFFFFFF, (r[:, 4] - r[:, 0]) * TICK_US]))
    a = np.concatenate(recs)
    print(f"launches {len(spans)}  span us (first wave start -> last wave end): {pct(np.array(spans))}")
    names = ["start offset", "table copy", "items", "slots", "lists", "extents", "tasks", "end", "wave end offset"]
    for k, nm in enumerate(names):
        print(f"{nm:>16} us  {pct(a[:, k])}")
    print(f"{'wave lifetime':>16} us  {pct(a[:, 12])}")
    print(f"{'tasks/wave':>16}     {pct(a[:, 9])}")
    print(f"{'probes/wave':>16}     {pct(a[:, 10])}")
    w_share, c_share, med_with, med_without = list_round(raw)
    print(f"list round (1b): {100 * w_share:.1f} % of waves, {100 * c_share:.2f} % of checks; "
          f"median lists phase {med_with:.2f} us with one, {med_without:.2f} us without")
    fw, fc = front_flags(raw)
    print(f"flagged fronts (slot read instead): {100 * fw:.1f} % of waves, {100 * fc:.2f} % of checks")


if __name__ == "__main__":
    main(sys.argv[1])
