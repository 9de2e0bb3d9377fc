#!/usr/bin/env python3
"""Cost of the hierarchical block matcher (tensors.match_pairs with levels > 1 -> papof_match_hier_tensor: k_match_prepare
per level, k_match on the top level, k_match_refine per lower level) against the flat search, in ONE run on the shipped build.

Frames: one uint8 NHWC pair (C = 3) of band-limited texture per size -- 1920x1080 and 240x135 -- the second frame a pan of
the first by (52, -24) pixels (tests/_hmatch_ref.py: wide_pan_scene), which every hierarchical configuration below reaches
and the flat search does not.  Both directions (two items), stride 2, patch 3, refine 1.  Per size:
  flat, search 20 and 32;  levels 2, 3 and 4 at search 20;  levels 3 at search 8 (the reach of the flat search at its maximum,
  64 px);  and each hierarchical configuration once more with PAPOF_MATCH_STAGED=0 (every tile of k_match_refine reads B
  through global addresses).
The time is the device time between two events around the call, median (min, max) of 11 after two warm-up calls; the share
is that of the forward cells that hold the pan exactly, among the cells whose target stays 8 px inside the frame.  The bar:
at 1920x1080, levels 3 at search 20 takes at most half the flat search 20's time of the same run.

    python3 tools/hmatch_probe.py --out profiles/hmatch_probe.txt"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import match_pairs  # noqa: E402

SIZES = ((1080, 1920), (135, 240))
PAN = (52, -24)
REPS = 11
CONFIGS = (dict(levels=1, search=20), dict(levels=1, search=32), dict(levels=2, search=20), dict(levels=3, search=20),
           dict(levels=4, search=20), dict(levels=3, search=8))


def event_times(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dt.append(e0.elapsed_time(e1))
    return float(np.median(dt)), min(dt), max(dt)


def candidates(levels, search, refine=1):
    """candidates per level-0 cell, averaged: the top level's window shared by 4^(levels - 1) cells, 5 (2 r + 1)^2 below"""
    c = (2 * search + 1) ** 2 / 4.0 ** (levels - 1)
    return c + sum(5 * (2 * refine + 1) ** 2 / 4.0 ** l for l in range(levels - 1))


def main():
    from _hmatch_ref import exact_share, wide_pan_scene
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Hierarchical block matching on one %s device.  One uint8 NHWC pair (C = 3) per size, a pan by %r pixels; both "
        "directions (two items); stride 2, patch 3, refine 1.  Event times: median (min, max) of %d after warm-up, in ms." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], PAN, REPS))
    os.environ.pop("PAPOF_MATCH_STAGED", None)
    bar = {}
    for H, W in SIZES:
        im1, im2, _, _ = wide_pan_scene(3, PAN, H, W, pad=64)
        a, b = torch.from_numpy(im1[None]).to(dev), torch.from_numpy(im2[None]).to(dev)
        say()
        say("%dx%d (%d x %d cells):" % (W, H, W // 2, H // 2))
        for cfg in CONFIGS:
            for staged in ((True,) if cfg["levels"] == 1 else (True, False)):
                if staged:
                    os.environ.pop("PAPOF_MATCH_STAGED", None)
                else:
                    os.environ["PAPOF_MATCH_STAGED"] = "0"
                fn = lambda: match_pairs(a, b, layout="NHWC", stride=2, patch=3, refine=1, **cfg)  # noqa: E731
                t = event_times(fn)
                share = exact_share(fn().disp_fw[0].cpu().numpy(), PAN, 2, (H, W))
                os.environ.pop("PAPOF_MATCH_STAGED", None)
                what = "flat" if cfg["levels"] == 1 else "levels %d" % cfg["levels"]
                say("  %-8s search %2d%s: %7.3f (%.3f, %.3f) ms; reach %3d px; %6.1f candidates per cell; exact %.4f" % (
                    what, cfg["search"], "" if staged else ", PAPOF_MATCH_STAGED=0", *t, (2 << (cfg["levels"] - 1)) * cfg["search"],
                    candidates(cfg["levels"], cfg["search"]), share))
                if staged and (H, W) == SIZES[0] and cfg["search"] == 20 and cfg["levels"] in (1, 3):
                    bar[cfg["levels"]] = t[0]
    say()
    say("The bar at 1920x1080: levels 3 at search 20 takes %.3f ms = %.3f of the flat search 20's %.3f ms (at most 0.5): %s" % (
        bar[3], bar[3] / bar[1], bar[1], "met" if bar[3] <= 0.5 * bar[1] else "MISSED"))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
