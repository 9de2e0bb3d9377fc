#!/usr/bin/env python3
"""Host side of the 1080p call: median of papof_last_host_times (seconds the host spends enqueueing a call, and waiting for
it) over `reps` uint8 calls, 5 levels, default schedule.  PAPOF_LIB selects the build (A/B: alternate processes).
usage: host_times_probe.py [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402

import cases  # noqa: E402
from papteam_opticalflow_amd import Papof  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
a, b = cases.load_frame_u8("1920", 1), cases.load_frame_u8("1920", 2)
g = Papof(0)
for _ in range(3):
    g.coarse2fine_flow_u8(a, b, 5)
enq, wait = [], []
for _ in range(reps):
    g.coarse2fine_flow_u8(a, b, 5)
    t = g.last_host_times()
    enq.append(t[0])
    wait.append(t[1])
print("%-34s host enqueue median %.3f ms (min %.3f)  wait median %.3f ms" % (
    os.environ.get("PAPOF_LIB") or "this build", np.median(enq) * 1e3, min(enq) * 1e3, np.median(wait) * 1e3))
