#!/usr/bin/env python3
"""One small workload per route through the flow calls, to be run under rocprofv3 --kernel-trace --memory-copy-trace with
two builds of the library (PAPOF_LIB selects the build) and compared by tools/trace_compare.py:

  hostio  papof_flow from host arrays into page-locked result arrays, 1080p, 5 levels (the early result copies)
  seq     a uint8 sequence, prime plus three pushes, 480x270, 5 levels
  fb      flow_pairs_fb on 4 pairs of 240x135, 4 levels (the batched chain, both directions)
  branch  one 64x48 call with bicubic interpolation, the Gaussian-mixture model and n_inner = 2
  deep    one 53x37 call with 7 levels (the pyramid chains through finer levels)
  bands   the exact-order band split on 2 ranks, 480x270, 5 levels (needs two devices)

(the headline is bench.py itself).  usage: trace_cases.py <case>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402

import cases  # noqa: E402
from papteam_opticalflow_amd import Papof, default_params  # noqa: E402


def _f64(u8):
    return u8.astype(np.float64) / 255.0


def _noise(h, w):
    rng = np.random.default_rng(h * w)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return a, np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))


def hostio():
    g = Papof(0)
    a, b = _f64(cases.load_frame_u8("1920", 1)), _f64(cases.load_frame_u8("1920", 2))
    vx = g.coarse2fine_flow(a, b, 5)[0]  # result arrays of this size come from the page-locked pool
    print("hostio: vx sum %.17g" % vx.sum())


def seq():
    g = Papof(0)
    f = [cases.load_frame_u8("480", i + 1) for i in range(3)]
    g.seq_reset()
    assert g.seq_push(f[0], 5) is None
    for x in (f[1], f[2], f[0]):
        print("seq: vx sum %.17g" % g.seq_push(x, 5)[0].sum())


def fb():
    import torch
    from papteam_opticalflow_amd import tensors
    f = [cases.load_frame_u8("240", i + 1) for i in range(3)]
    a = torch.from_numpy(np.stack([f[0], f[1], f[2], f[1]])).cuda()
    b = torch.from_numpy(np.stack([f[1], f[2], f[0], f[0]])).cuda()
    out = tensors.flow_pairs_fb(a, b, 4, layout="NHWC")
    torch.cuda.synchronize()
    print("fb: flow sum %.17g" % float(out[0].double().sum()))


def branch():
    g = Papof(0)
    a, b = _noise(48, 64)
    p = default_params(interpolation=1, noise_model=1, n_inner=2)
    print("branch: vx sum %.17g" % g.coarse2fine_flow(_f64(a), _f64(b), 2, p)[0].sum())


def deep():
    g = Papof(0)
    a, b = _noise(37, 53)
    print("deep: vx sum %.17g" % g.coarse2fine_flow_u8(a, b, 7)[0].sum())


def bands():
    from papteam_opticalflow_amd import SOR_EXACT
    from papteam_opticalflow_amd.capi import LocalTileGroup
    a, b = _f64(cases.load_frame_u8("480", 1)), _f64(cases.load_frame_u8("480", 2))
    grp = LocalTileGroup(2)
    try:
        print("bands: vx sum %.17g" % grp.coarse2fine_flow(a, b, 5, default_params(sor_mode=SOR_EXACT))[0].sum())
    finally:
        grp.close()


if __name__ == "__main__":
    {"hostio": hostio, "seq": seq, "fb": fb, "branch": branch, "deep": deep, "bands": bands}[sys.argv[1]]()
