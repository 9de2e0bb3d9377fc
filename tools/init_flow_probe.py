#!/usr/bin/env python3
"""Cost and use of an initial flow (tensors.flow_pairs / flow_video init_flow -> papof_flow_batch_tensor_init).

1. Reduction cost, from rocprofv3's kernel trace of a --kernel-only run: the kernels an initial flow adds to a call --
   k_init_check (the refusal check behind the entry wait), then at the coarsest level the init's k_ingest_frames,
   k_init_sanitize and the pyramid steps (k_filter_hv*, k_resize) along the coarsest level's ancestors -- for 32 pairs of
   240x135 at 5 and 15 levels (the batched chain) and one 1920x1080 pair at 5 levels (the single call).  In dispatch order
   the init's ingest directly precedes k_init_sanitize and its pyramid steps directly follow it.
       rocprofv3 --kernel-trace --stats -f csv -d DIR -o init -- python3 tools/init_flow_probe.py --kernel-only
       python3 tools/init_flow_probe.py --kernel-stats DIR --out profiles/init_flow_probe.txt
2. End to end: wall time per pair with no init, an all-zero init and a non-zero init, alternating in one process
   (call + synchronise; median and min / max over --reps rounds).
3. What a warm start buys, on the committed triples (240x135, 480x270): frame 2 interpolated at t = 0.5 from frames 1 and
   3 (interpolate, flows of flow_pairs_fb, its occlusion mask), the flows either from the cold 5-level call, or from a
   cold 4-level call at half resolution, up-sampled x2 (bilinear, flow x 2) and refined at full resolution with
   pyramidLevels 1 or 2 from it.  Reported only."""
import argparse
import csv
import glob
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cases as golden  # noqa: E402
from papteam_opticalflow_amd.tensors import flow_pairs_fb, flow_video, interpolate  # noqa: E402


def smooth_init(B, H, W, dev):
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = torch.zeros((B, 2, H, W), dtype=torch.float64)
    for p in range(B):
        out[p, 0] = 2.5 * torch.sin(2 * np.pi * x / W + 0.7 * p) + 0.5
        out[p, 1] = -1.5 * torch.cos(2 * np.pi * (x + y) / (W + H) + 0.3 * p)
    return out.to(dev)


def video_240(n, dev):
    a, b = golden.load_frame_u8("240", 1), golden.load_frame_u8("240", 2)
    fr = [np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(n)]
    return torch.from_numpy(np.stack(fr)).to(dev)


def make_cases(dev):
    v = video_240(33, dev)
    g = torch.Generator().manual_seed(3)
    big = torch.randint(0, 256, (2, 1080, 1920, 3), generator=g, dtype=torch.uint8)
    big[1] = torch.roll(big[0], 2, dims=1)
    big = big.to(dev)
    out = []
    for what, frames, levels in (("240x135, 32 pairs (a video of 33 frames), 5 levels", v, 5),
                                 ("240x135, 32 pairs (a video of 33 frames), 15 levels", v, 15),
                                 ("1920x1080, 1 pair, 5 levels", big, 5)):
        B, H, W = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
        out.append((what, frames, levels, B, torch.zeros((B, 2, H, W), dtype=torch.float64, device=dev),
                    smooth_init(B, H, W, dev)))
    return out


def reduction_times(path, n_cases, reps):
    """per case and call: (us of the init's kernels, their names) from rocprofv3's kernel trace, in dispatch order"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        order = int(row.get("correlation_id") or row.get("dispatch_id") or row["start_timestamp"])
        rows.append((order, name, (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    rows.sort()
    calls = []  # [us, kernels] per call, a call starting at its k_init_check
    for i, (_, name, us) in enumerate(rows):
        if "k_init_check" in name:
            calls.append([us, 1])
        elif "k_init_sanitize" in name and calls:
            calls[-1][0] += us
            calls[-1][1] += 1
            j = i - 1
            while j >= 0 and "ingest_frames" in rows[j][1]:
                calls[-1][0] += rows[j][2]
                calls[-1][1] += 1
                j -= 1
            j = i + 1
            while j < len(rows) and ("filter" in rows[j][1] or "k_resize" in rows[j][1]):
                calls[-1][0] += rows[j][2]
                calls[-1][1] += 1
                j += 1
    calls = calls[n_cases:]  # the warm-up: one call with an init per case
    if len(calls) != n_cases * reps:
        raise SystemExit("expected %d calls with an init after the warm-up, found %d" % (n_cases * reps, len(calls)))
    return [calls[i * reps:(i + 1) * reps] for i in range(n_cases)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def call(frames, levels, init):
    return flow_video(frames, levels, layout="NHWC", init_flow=init)


def warm_start(res, say):
    dev = torch.device("cuda", 0)
    f = [torch.from_numpy(golden.load_frame_u8(res, i)).to(dev)[None] for i in (1, 2, 3)]
    H, W = f[0].shape[1:3]
    truth = f[1].double()

    def err(fb):
        mid = interpolate(f[0], f[2], fb.flow_fw, fb.flow_bw, [0.5], occlusion=fb.occlusion, layout="NHWC",
                          out_dtype=torch.float64)[:, 0]
        return float((mid * 255 - truth).abs().mean())

    def half(x):
        return torch.nn.functional.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=0.5, mode="bilinear",
                                               align_corners=False, antialias=True).permute(0, 2, 3, 1).contiguous()

    def up(flow):
        u = torch.nn.functional.interpolate(flow, size=(H, W), mode="bilinear", align_corners=False)
        u[:, 0] *= W / flow.shape[3]
        u[:, 1] *= H / flow.shape[2]
        return u.contiguous()

    runs = {}
    h1, h3 = half(f[0]) / 255, half(f[2]) / 255
    for rep in range(4):  # the first round warms up
        t = {}
        t["cold, 5 levels"] = wall(lambda: runs.__setitem__("cold", flow_pairs_fb(f[0], f[2], 5, layout="NHWC")))
        for lv in (1, 2):
            def warm():
                hb = flow_pairs_fb(h1, h3, 4, layout="NHWC", consistency=None)
                runs[lv] = flow_pairs_fb(f[0], f[2], lv, layout="NHWC", init_flow=up(hb.flow_fw),
                                         init_flow_bw=up(hb.flow_bw))
            t["half-res 4 levels, x2, refine %d level%s" % (lv, "s" if lv > 1 else "")] = wall(warm)
        if rep == 1:
            times = {k: [v] for k, v in t.items()}
        elif rep > 1:
            for k, v in t.items():
                times[k].append(v)
    errs = {"cold, 5 levels": err(runs["cold"]), "half-res 4 levels, x2, refine 1 level": err(runs[1]),
            "half-res 4 levels, x2, refine 2 levels": err(runs[2])}
    blend = float(((f[0].double() + f[2].double()) / 2 - truth).abs().mean())
    say("  %s (%dx%d), frame 2 from frames 1 and 3 (t = 0.5); the plain blend's error %.3f" % (res, W, H, blend))
    for k in errs:
        say("    %-40s %8.2f ms (both directions)   mean |interpolated - frame 2| %.3f (of 255)" % (
            k, 1e3 * float(np.median(times[k])), errs[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run the calls with a non-zero init only (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cs = make_cases(dev)
    for _, frames, levels, _, zero, init in cs:  # warm-up: arena, counters, handles
        call(frames, levels, None)
        call(frames, levels, init)
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, frames, levels, _, _, init in cs:
            for _ in range(args.reps):
                call(frames, levels, init)
        torch.cuda.synchronize()
        return
    ks = reduction_times(args.kernel_stats, len(cs), args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Initial flows on one %s device (tensors.flow_video with init_flow; uint8 NHWC frames, float64 inits)." %
        torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    for i, (what, frames, levels, B, zero, init) in enumerate(cs):
        say()
        say("%s" % what)
        t = {"no init": [], "zero init": [], "non-zero init": []}
        for _ in range(args.reps):
            t["no init"].append(wall(lambda: call(frames, levels, None)))
            t["zero init"].append(wall(lambda: call(frames, levels, zero)))
            t["non-zero init"].append(wall(lambda: call(frames, levels, init)))
        for k, v in t.items():
            v = np.array(v) / B * 1e3
            say("  %-14s %8.3f ms per pair  (min %.3f, max %.3f; %d rounds, alternating)" % (
                k, float(np.median(v)), float(v.min()), float(v.max()), args.reps))
        if ks:
            us = np.array([c[0] for c in ks[i]])
            n = ks[i][0][1]
            call_ms = float(np.median(t["non-zero init"])) * 1e3
            say("  init kernels (rocprofv3 --kernel-trace, %d per call: the check, ingest, sanitize, pyramid steps): "
                "%.1f us per call (min %.1f, max %.1f) = %.2f us per pair = %.2f %% of the call's %.3f ms" % (
                    n, float(np.median(us)), float(us.min()), float(us.max()), float(np.median(us)) / B,
                    100 * float(np.median(us)) / 1e3 / call_ms, call_ms))
    say()
    say("What a warm start buys (reported, not asserted):")
    for res in ("240", "480"):
        warm_start(res, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
