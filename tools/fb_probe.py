#!/usr/bin/env python3
"""ms per pair of flow_video_fb (both directions of every consecutive pair in one launch chain, with the occlusion mask)
against flow_video(frames) + flow_video(frames.flip(0)) (two calls: every pyramid, feature plane and derivative plane built
twice, two launch chains), uint8 NHWC device frames, reference schedule, after warm-up, the two ways alternated in one
process.  Every call returns with its results written.  The first round also checks that the two ways give the same bits
(backward pair i of flow_video_fb = pair T - 2 - i of the reversed video).

usage: fb_probe.py [--sizes 240:17,480:9] [--levels 5] [--reps 8]
       fb_probe.py --check 1920 [--reps 20]   (fb_consistency alone on two 1080p flows: the run under
                                               `rocprofv3 --kernel-trace --stats` that prices k_fb_check)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cases  # noqa: E402
from papteam_opticalflow_amd.tensors import fb_consistency, flow_video, flow_video_fb  # noqa: E402


def video(res, n):
    """n frames that all differ: the two decoded frames of the reference's collection, shifted copies of them"""
    a, b = cases.load_frame_u8(res, 1), cases.load_frame_u8(res, 2)
    return np.stack([np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(n)])


def same(a, b):
    return np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))


def probe_check(res, reps):
    a = cases.load_frame_u8(res, 1)
    H, W = a.shape[:2]
    g = torch.Generator().manual_seed(5)
    fw = (torch.randn(1, 2, H // 8 + 1, W // 8 + 1, generator=g, dtype=torch.float64) * 3).cuda()
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(1, 2, H, W, generator=g, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m = fb_consistency(fw, bw)
        torch.cuda.synchronize()
        dt.append(time.perf_counter() - t0)
    print("fb_consistency on one %dx%d float64 flow pair: %d calls, median wall %.1f us (call + sync), occluded %.3f" % (
        W, H, reps, 1e6 * float(np.median(dt)), float(m.float().mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="240:17,480:9", help="res:frames,...")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--check", default=None, help="res: time fb_consistency alone")
    args = ap.parse_args()
    if args.check:
        probe_check(args.check, args.reps)
        return
    print("consecutive pairs of a video, uint8 NHWC frames, %d levels, reference schedule; ms per pair (both directions), "
          "%d timed calls per way, alternated" % (args.levels, args.reps))
    print("%10s %6s %10s %14s %8s %s" % ("size", "pairs", "fb", "two calls", "fb / 2", "bits"))
    for spec in args.sizes.split(","):
        res, nf = spec.split(":")
        nf = int(nf)
        n = nf - 1
        dev = torch.from_numpy(video(res, nf)).cuda()
        torch.cuda.synchronize()

        def two():
            return flow_video(dev, args.levels, layout="NHWC"), flow_video(dev.flip(0), args.levels, layout="NHWC")

        run = {"fb": lambda: flow_video_fb(dev, args.levels, layout="NHWC"), "two": two}
        got = {p: run[p]() for p in run}  # warm-up: arenas, counters, scratch
        for p in run:
            run[p]()
        fb, (fwd, rev) = got["fb"], got["two"]
        ok = same(fb.flow_fw, fwd[0]) and same(fb.warpI2_fw, fwd[1]) and same(fb.flow_bw, rev[0].flip(0)) and \
            same(fb.warpI2_bw, rev[1].flip(0))
        dt = {p: [] for p in run}
        for _ in range(args.reps):
            for p in run:
                t0 = time.perf_counter()
                run[p]()
                dt[p].append(time.perf_counter() - t0)
        ms = {p: 1e3 * float(np.median(dt[p])) / n for p in run}
        h, w = dev.shape[1:3]
        print("%10s %6d %10.3f %14.3f %8.3f %s" % ("%dx%d" % (w, h), n, ms["fb"], ms["two"], ms["fb"] / ms["two"],
                                                 "identical" if ok else "DIFFER"), flush=True)
        for p in run:
            print("%10s %6s   %s: median of per-call ms per pair; min %.3f max %.3f" % (
                "", "", p, 1e3 * min(dt[p]) / n, 1e3 * max(dt[p]) / n))


if __name__ == "__main__":
    main()
