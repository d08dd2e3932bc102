#!/usr/bin/env python3
"""submit_probe.py — per-submit host time of the four host-buffer request formats, one request in
flight. tools/host_probe.py times item batches only; this runs tools/bench_shaped.py's own loops
(items, uniform, shaped with one shape, shaped with four, in turn) under the driver's trace
(gckd_set_trace) and keeps, for each run of a loop, the median time from the previous wait's return
to the submit's return — host_probe.py's lone_submit_us_median — and from there to the wait's.

One JSON line after bench_shaped's own: per format the median over the rounds and every round's
figure, in microseconds. GCK_LIBRARY selects the library, as everywhere.

    python3 tools/submit_probe.py
"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gochugaru_amd import engine as E  # noqa: E402

RUNS = []
_run = E._Prepared.run


def traced(self):
    stamps = np.zeros(2 * self._k, dtype=np.float64)
    E._driver().gckd_set_trace(stamps.ctypes.data_as(ctypes.c_void_p), self._k)
    try:
        secs = _run(self)
    finally:
        E._driver().gckd_set_trace(None, 0)
    sub, wt = stamps[0::2], stamps[1::2]
    prev_end = np.concatenate([[0.0], wt[:-1]])
    RUNS.append((float(np.median((sub - prev_end)[3:])) * 1e6, float(np.median((wt - sub)[3:])) * 1e6))
    return secs


E._Prepared.run = traced
import bench_shaped  # noqa: E402

sys.argv = ["bench_shaped.py", "--inflight", "1", "--requests", "203", "--rounds", "5"]
bench_shaped.main()
order = ["items", "uniform", "shaped1", "shaped4"]
timed = RUNS[4:]  # (the first run of each loop is bench_shaped's warm-up)
out = {"unit": "us", "what": "lone request, pinned buffers, 65,536 checks: median submit time per run", "lines": {}}
for j, line in enumerate(order):
    s = [round(r[0], 3) for r in timed[j::4]]
    w = [round(r[1], 2) for r in timed[j::4]]
    out["lines"][line] = {"submit_us_median": statistics.median(s), "submit_us_runs": s, "wait_us_runs": w}
print(json.dumps(out))
