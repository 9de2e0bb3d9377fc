#!/usr/bin/env python3
"""ms per pair of flow_video on device uint8 frames (papof_flow_batch_tensor: frames read in HBM, float64 flow tensors out)
against Papof.flow_batch on the same frames from host memory (papof_flow_batch_u8: uploads, float64 results downloaded into
page-locked arrays), consecutive pairs of a video, reference schedule, after warm-up, the two paths alternated in one process.
Both calls return with their results written.  The first timed round also checks that the two paths give the same bits.

usage: tensor_batch_probe.py [--sizes 240:32,480:16,1920:4] [--levels 5] [--reps 8] [--paths tensor,host]
(`--paths tensor` alone: the run under `rocprofv3 --kernel-trace --stats` that prices k_ingest_frames / k_emit_outputs)"""
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
from papteam_opticalflow_amd import Papof  # noqa: E402
from papteam_opticalflow_amd.tensors import flow_video  # noqa: E402


def video(res, n):
    """n frames that all differ: the two decoded frames of the reference's collection, shifted copies of them"""
    a, b = cases.load_frame_u8(res, 1), cases.load_frame_u8(res, 2)
    return np.stack([np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="240:32,480:16,1920:4", help="res:pairs,...")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--paths", default="tensor,host")
    args = ap.parse_args()
    paths = args.paths.split(",")
    host = Papof(0) if "host" in paths else None
    print("consecutive pairs of a video, uint8 frames, %d levels, reference schedule; ms per pair (%d timed calls per path, "
          "alternated)" % (args.levels, args.reps))
    print("%10s %6s %12s %12s %8s %s" % ("size", "pairs", "tensor", "host", "t / h", "bits"))
    for spec in args.sizes.split(","):
        res, n = spec.split(":")
        n = int(n)
        frames = video(res, n + 1)
        dev = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        run = {"tensor": lambda: flow_video(dev, args.levels, layout="NHWC"),
               "host": lambda: host.flow_batch(frames, args.levels)}
        got = {p: run[p]() for p in paths}  # warm-up: arenas, counters, scratch
        for p in paths:
            run[p]()
        bits = "-"
        if len(paths) == 2:
            flow, warp, _ = got["tensor"]
            out, _ = got["host"]
            uv = np.stack([np.stack(o[:2]) for o in out])
            wi = np.stack([o[2] for o in out])
            same = np.array_equal(flow.cpu().numpy().view(np.int64), uv.view(np.int64)) and \
                np.array_equal(warp.cpu().numpy().view(np.int64), wi.view(np.int64))
            bits = "identical" if same else "DIFFER"
        dt = {p: [] for p in paths}
        for _ in range(args.reps):
            for p in paths:
                t0 = time.perf_counter()
                run[p]()
                dt[p].append(time.perf_counter() - t0)
        ms = {p: 1e3 * float(np.median(dt[p])) / n for p in paths}
        h, w = frames.shape[1:3]
        print("%10s %6d %12s %12s %8s %s" % (
            "%dx%d" % (w, h), n, "%.3f" % ms["tensor"] if "tensor" in ms else "-", "%.3f" % ms["host"] if "host" in ms else "-",
            "%.3f" % (ms["tensor"] / ms["host"]) if len(ms) == 2 else "-", bits), flush=True)
        for p in paths:
            print("%10s %6s   %s: median of per-call ms per pair; min %.3f max %.3f" % (
                "", "", p, 1e3 * min(dt[p]) / n, 1e3 * max(dt[p]) / n))


if __name__ == "__main__":
    main()
