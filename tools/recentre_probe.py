#!/usr/bin/env python3
"""Cost of the re-centred block search (tensors.match_pairs with recentre -> papof_match_recentre_tensor: the hierarchical
chain down to level 0, k_match_origin, k_match_recentre) against the hierarchical search alone and against the flat search,
in ONE run on the shipped build.

Frames: uint8 NHWC pairs (C = 3) of tests/_recentre_ref.py's scene -- a 24 x 24 object that moves by (34, -14) against a
pan of (70, 26) -- one pair of 1920x1080 and 32 pairs of 240x135 (texture seeds 4 .. 35).  Both directions, stride 2, patch
3, search 20, refine 1.  Per case: recentre=20 at 3 levels, levels=3 alone, and the flat search at search=20.  The time is
the device time between two events around the call, median (min, max) of 11 after two warm-up calls; the shares are those
of the first pair's forward cells that hold the true vector exactly (background / object, as the tests count them).

The share of k_match_origin in the re-centred call comes from the kernel trace of a second run:

    rocprofv3 --kernel-trace -f csv -d DIR -o recentre -- python3 tools/recentre_probe.py --kernel-only
    python3 tools/recentre_probe.py --kernel-trace DIR --out profiles/recentre_probe.txt"""
import argparse
import csv
import glob
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import match_pairs  # noqa: E402

PAN, REL, ORIGIN = (70, 26), (34, -14), (100, 60)
REPS = 11
CASES = (("1920x1080, 1 pair", 1080, 1920, 1), ("240x135, 32 pairs", 135, 240, 32))
CONFIGS = (("recentre 20, levels 3", dict(levels=3, recentre=20)), ("levels 3", dict(levels=3)), ("flat, search 20", dict()))
KERNELS = ("k_match_prepare", "k_match_refine", "k_match_origin", "k_match_recentre", "k_match")  # (the longest names first)


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


def kernel_shares(path):
    """per case {kernel: microseconds per call} of the --kernel-only run, from rocprofv3's kernel trace: a call ends with
    its k_match_recentre dispatch, and every case makes REPS calls"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        for k in KERNELS:
            if k in name:
                rows.append((int(row["start_timestamp"]), k, (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
                break
    rows.sort()
    out, done = [{} for _ in CASES], 0
    for _, k, us in rows:
        case = done // REPS
        if case < len(CASES):
            out[case][k] = out[case].get(k, 0.0) + us / REPS
        done += k == "k_match_recentre"
    return out


def main():
    from _recentre_ref import pan_object_scene, shares
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true", help="run the re-centred calls only, %d per case (for rocprofv3)" % REPS)
    ap.add_argument("--kernel-trace", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    kernels = kernel_shares(args.kernel_trace) if args.kernel_trace else None
    moved = (PAN[0] + REL[0], PAN[1] + REL[1])
    if not args.kernel_only:
        say("Re-centred block search on one %s device.  uint8 NHWC pairs (C = 3): a 24 x 24 object moving by %r against a pan of "
            "%r; both directions; stride 2, patch 3, search 20, refine 1.  Event times: median (min, max) of %d after warm-up, "
            "in ms.  Shares: background / object cells of the first pair's forward field with the exact vector." % (
                torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], REL, PAN, REPS))
    for i, (what, H, W, n) in enumerate(CASES):
        scenes = [pan_object_scene(4 + k, PAN, REL, ORIGIN, H, W) for k in range(n)]
        a = torch.from_numpy(np.stack([s[0] for s in scenes])).to(dev)
        b = torch.from_numpy(np.stack([s[1] for s in scenes])).to(dev)
        if args.kernel_only:
            for _ in range(REPS):
                match_pairs(a, b, layout="NHWC", **CONFIGS[0][1])
            torch.cuda.synchronize()
            continue
        say()
        say("%s (%d x %d cells, %d tiles of 32 x 8):" % (what, W // 2, H // 2, -(-(W // 2) // 32) * -(-(H // 2) // 8)))
        times = {}
        for name, kw in CONFIGS:
            got = match_pairs(a, b, layout="NHWC", **kw)
            sh = shares(got.disp_fw[0].cpu().numpy(), PAN, moved, scenes[0][2], scenes[0][3], 2)
            times[name] = event_times(lambda: match_pairs(a, b, layout="NHWC", **kw))
            say("  %-22s %8.3f ms (%.3f, %.3f)   shares %.4f / %.4f" % (name, *times[name], *sh))
        say("  re-centred / levels 3: %.2f x;  re-centred / flat: %.2f x" % (
            times[CONFIGS[0][0]][0] / times[CONFIGS[1][0]][0], times[CONFIGS[0][0]][0] / times[CONFIGS[2][0]][0]))
        if kernels:
            total = sum(kernels[i].values())
            say("  kernels of the re-centred call (kernel trace of a second run, per call): %s; total %.1f us" % (
                ", ".join("%s %.1f us" % (k, v) for k, v in sorted(kernels[i].items())), total))
            say("  k_match_origin: %.2f %% of the call's kernel time" % (100.0 * kernels[i].get("k_match_origin", 0.0) / total))
    if args.out and not args.kernel_only:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
