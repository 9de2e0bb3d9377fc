#!/usr/bin/env python3
"""Cost and use of reduced-resolution flow (tensors.decimate, upsample_flow, flow_pairs_lr -> papof_decimate_tensor,
papof_upsample_flow_tensor).

1. The kernel: k_upsample_flow at 960x540 -> 1920x1080 and 120x68 -> 240x135, a uint8 RGB guide, float64 flows, the
   low-resolution mask, the defaults, from rocprofv3's kernel trace of a --kernel-only run:
       rocprofv3 --kernel-trace --stats -f csv -d DIR -o up -- python3 tools/upsample_probe.py --kernel-only
       python3 tools/upsample_probe.py --kernel-stats DIR --out profiles/upsample_probe.txt
   against its byte floor -- 16 B written and C B read per output pixel, the low-resolution planes (16 + 8 C + 1 B per
   cell) read once -- over 8 TB/s (spec) and 6.3 TB/s (a measured copy), and against the same rule written in torch
   operations (pad, unfold-like gathers of the 25 taps, exponentials, sums; float64; device events).
2. The feature: wall time per pair (call + synchronise, alternating in one process, median of --reps rounds) of
   flow_pairs_fb(pyramidLevels=5) against flow_pairs_lr at factor 2 and 4 with pyramidLevels 4, refine_levels 0 and 1, on
   one 1920x1080 pair and on 32 pairs of 240x135, and the parts of the factor-2 call timed one by one.  Every translation
   unit the full-resolution call runs is unchanged by the reduced-resolution path (upsample.hip is a translation unit of
   its own), so the full call of this build is the full call of the build before it.
3. Interpolation error on the committed triples (240x135, 480x270), tools/init_flow_probe.py's protocol: frame 2
   interpolated at t = 0.5 from frames 1 and 3 with the flows of the cold 5-level call, or of flow_pairs_lr at factor 2 with
   refine_levels 0 and 1.  Reported only."""
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
from papteam_opticalflow_amd import tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (decimate, fb_consistency, flow_pairs_fb, flow_pairs_lr, interpolate,  # noqa: E402
                                             upsample_flow)

SPEC_BW, COPY_BW = 8e12, 6.3e12
SIZES = ((1080, 1920), (135, 240))


def kernel_case(H, W, dev):
    g = torch.Generator().manual_seed(H)
    guide = torch.rand((1, 3, -(-H // 16), -(-W // 16)), generator=g)  # smooth blobs: random colours every 16 pixels, bicubic between
    guide = torch.nn.functional.interpolate(guide, size=(H, W), mode="bicubic").clamp(0, 1).permute(0, 2, 3, 1)
    guide = (255 * guide).round().to(torch.uint8).to(dev)
    h, w = -(-H // 2), -(-W // 2)
    flow = torch.randn((1, 2, h, w), generator=g, dtype=torch.float64).to(dev)
    occ = (torch.rand((1, h, w), generator=g) < 0.05).to(dev)
    return flow, guide, decimate(guide, 2, layout="NHWC"), occ


def torch_upsample(flow, guide, guide_lr, occ, f=2, r=2, sigma_s=1.0, sigma_c=0.05):
    """the same rule in torch operations, float weights: gathers of the (2 r + 1)^2 taps, exponentials, sums"""
    B, H, W, C = guide.shape
    h, w = flow.shape[2:]
    Y, X = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    cy, cx = Y // f, X // f
    oy, ox = (Y % f - (f - 1) / 2) / f, (X % f - (f - 1) / 2) / f
    g = guide.double() / 255.0
    live = torch.isfinite(flow).all(1) & ~occ
    su = torch.zeros((B, 2, H, W), dtype=torch.float64, device=flow.device)
    sw = torch.zeros((B, H, W), dtype=torch.float64, device=flow.device)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ty, tx = cy + dy, cx + dx
            ok = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            ty, tx = ty.clamp(0, h - 1), tx.clamp(0, w - 1)
            d2 = ((g - guide_lr[:, ty, tx]) ** 2).mean(-1)
            ay, ax = (dy - oy).abs(), (dx - ox).abs()
            tent = (1 - ax).clamp(min=0) * (1 - ay).clamp(min=0)
            wk = (15 / 16 * tent + 1 / 16 * torch.exp(-(ax * ax + ay * ay) / (2 * sigma_s ** 2))) * torch.exp(-d2 / (2 * sigma_c ** 2))
            wk = wk * (ok & live[:, ty, tx])
            su += wk[:, None] * torch.nan_to_num(flow[:, :, ty, tx])
            sw += wk
    return f * su / sw[:, None]


def kernel_times(path, reps):
    """per size: the durations in us of k_upsample_flow and k_decimate, in dispatch order, the warm-up call dropped"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        rows.append((int(row["start_timestamp"]), name, (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    rows.sort()
    n = len(SIZES)
    up, dec = ([u for _, name, u in rows if key in name] for key in ("k_upsample_flow", "k_decimate"))
    if len(up) != (reps + 1) * n or len(dec) != (reps + 1) * n:
        raise SystemExit("expected %d dispatches of each kernel, found %d and %d" % ((reps + 1) * n, len(up), len(dec)))
    # k_upsample_flow: per size a warm-up call and `reps`; k_decimate: kernel_case's of every size first, then `reps` per size
    return [[up[i * (reps + 1) + 1:(i + 1) * (reps + 1)] for i in range(n)], [dec[n + i * reps:n + (i + 1) * reps] for i in range(n)]]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out))


def video_240(n, dev):
    a, b = golden.load_frame_u8("240", 1), golden.load_frame_u8("240", 2)
    return torch.from_numpy(np.stack([np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(n)])).to(dev)


def feature(say, reps, dev):
    g = torch.Generator().manual_seed(3)
    big = torch.randint(0, 256, (1, 540, 960, 3), generator=g, dtype=torch.uint8)
    big = torch.nn.functional.interpolate(big.permute(0, 3, 1, 2).float(), size=(1080, 1920), mode="bicubic").clamp(0, 255)
    big = big.permute(0, 2, 3, 1).round().to(torch.uint8)  # texture with structure at the decimated scale too
    b1, b2 = big.to(dev), torch.roll(big, (1, 3), dims=(1, 2)).to(dev)
    v = video_240(33, dev)
    for what, im1, im2 in (("1920x1080, 1 pair", b1, b2), ("240x135, 32 pairs", v[:-1], v[1:])):
        B = im1.shape[0]
        runs = {"flow_pairs_fb, 5 levels (the full call)": lambda: flow_pairs_fb(im1, im2, 5, layout="NHWC")}
        for f, lv, rl in ((2, 4, 0), (2, 4, 1), (4, 4, 0), (4, 3, 0)):
            runs["flow_pairs_lr factor %d, %d levels, refine_levels %d" % (f, lv, rl)] = (
                lambda f=f, lv=lv, rl=rl: flow_pairs_lr(im1, im2, lv, factor=f, refine_levels=rl, layout="NHWC"))
        say()
        for k in list(runs):  # warm-up; a size the solver refuses is reported and left out
            try:
                runs[k]()
            except Exception as e:  # noqa: BLE001
                say("  %s: refused (%s)" % (k, e))
                del runs[k]
        t = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():
                t[k].append(wall(fn))
        say("%s (wall per pair, both directions and the mask; %d rounds, alternating)" % (what, reps))
        base = float(np.median(t["flow_pairs_fb, 5 levels (the full call)"]))
        for k, x in t.items():
            x = np.array(x)
            say("  %-52s %8.3f ms  (min %.3f, max %.3f)  %.2f of the full call" % (
                k, 1e3 * float(np.median(x)) / B, 1e3 * x.min() / B, 1e3 * x.max() / B, float(np.median(x)) / base))
        # the parts of the factor-2 call, one by one
        lo1, lo2 = decimate(im1, 2, layout="NHWC"), decimate(im2, 2, layout="NHWC")
        low = flow_pairs_fb(lo1, lo2, 4, layout="NHWC")
        up = [upsample_flow(low.flow_fw, im1, 2, guide_lr=lo1, occlusion=low.occlusion[:, 0], layout="NHWC"),
              upsample_flow(low.flow_bw, im2, 2, guide_lr=lo2, occlusion=low.occlusion[:, 1], layout="NHWC")]
        parts = {"decimate, both frames": lambda: (decimate(im1, 2, layout="NHWC"), decimate(im2, 2, layout="NHWC")),
                 "flow_pairs_fb on the decimated frames, 4 levels": lambda: flow_pairs_fb(lo1, lo2, 4, layout="NHWC"),
                 "upsample_flow, both directions": lambda: (
                     upsample_flow(low.flow_fw, im1, 2, guide_lr=lo1, occlusion=low.occlusion[:, 0], layout="NHWC"),
                     upsample_flow(low.flow_bw, im2, 2, guide_lr=lo2, occlusion=low.occlusion[:, 1], layout="NHWC")),
                 "fb_consistency at full resolution": lambda: fb_consistency(up[0], up[1])}
        for k, fn in parts.items():
            x = [wall(fn) for _ in range(reps)]
            say("    part: %-48s %8.3f ms per pair" % (k, 1e3 * float(np.median(x)) / B))


def interpolation(res, say, dev):
    f = [torch.from_numpy(golden.load_frame_u8(res, i)).to(dev)[None] for i in (1, 2, 3)]
    truth = f[1].double()

    def err(fb):
        mid = interpolate(f[0], f[2], fb.flow_fw, fb.flow_bw, [0.5], occlusion=fb.occlusion, layout="NHWC",
                          out_dtype=torch.float64)[:, 0]
        return float((mid * 255 - truth).abs().mean())
    runs = {"cold, 5 levels": lambda: flow_pairs_fb(f[0], f[2], 5, layout="NHWC"),
            "factor 2, 4 levels, refine_levels 0": lambda: flow_pairs_lr(f[0], f[2], 4, factor=2, layout="NHWC"),
            "factor 2, 4 levels, refine_levels 1": lambda: flow_pairs_lr(f[0], f[2], 4, factor=2, refine_levels=1, layout="NHWC")}
    blend = float(((f[0].double() + f[2].double()) / 2 - truth).abs().mean())
    say("  %s (%dx%d), frame 2 from frames 1 and 3 (t = 0.5); the plain blend's error %.3f" % (res, f[0].shape[2], f[0].shape[1], blend))
    for k, fn in runs.items():
        fn()
        x = [wall(fn) for _ in range(5)]
        say("    %-40s %8.2f ms   mean |interpolated - frame 2| %.3f (of 255)" % (k, 1e3 * float(np.median(x)), err(fn())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run the up-sampling calls only (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cs = [kernel_case(H, W, dev) for H, W in SIZES]
    if args.kernel_only:
        for flow, guide, lo, occ in cs:
            for _ in range(args.reps + 1):  # the first call warms up
                upsample_flow(flow, guide, 2, guide_lr=lo, occlusion=occ, layout="NHWC")
            for _ in range(args.reps):
                decimate(guide, 2, layout="NHWC")
        torch.cuda.synchronize()
        return
    ks = kernel_times(args.kernel_stats, args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Reduced-resolution flow on one %s device (uint8 NHWC frames, float64 flows, the defaults: radius %d, sigma_s %g, "
        "sigma_c %g)." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], tensors.UP_RADIUS, tensors.UP_SIGMA_S,
                          tensors.UP_SIGMA_C))
    for i, ((H, W), (flow, guide, lo, occ)) in enumerate(zip(SIZES, cs)):
        h, w = flow.shape[2:]
        nbytes = H * W * (16 + 3) + h * w * (16 + 8 * 3 + 1)
        say()
        say("k_upsample_flow %dx%d -> %dx%d" % (w, h, W, H))
        say("  byte floor: %.2f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (nbytes / 1e6, 1e6 * nbytes / SPEC_BW, 1e6 * nbytes / COPY_BW))
        ours = lambda: upsample_flow(flow, guide, 2, guide_lr=lo, occlusion=occ, layout="NHWC")  # noqa: E731
        theirs = lambda: torch_upsample(flow, guide, lo, occ)  # noqa: E731
        a, b = ours(), theirs()
        d = (a - b).abs()
        say("  the torch composition (float weights) against the kernel (integer tables): median |difference| %.2e, max %.2e" % (
            float(d.median()), float(d.max())))
        t_ours, t_torch = events(ours, args.reps), events(theirs, args.reps)
        say("  device events around the call: upsample_flow %.1f us, the torch composition %.1f us: %.1f x" % (
            t_ours, t_torch, t_torch / t_ours))
        if ks:
            us, dec = np.array(ks[0][i]), np.array(ks[1][i])
            say("  rocprofv3 --kernel-trace: k_upsample_flow %.1f us (min %.1f, max %.1f; %d dispatches) = %.2f x the 8 TB/s floor, "
                "%.2f x the 6.3 TB/s one; k_decimate of the guide %.1f us" % (
                    float(np.median(us)), us.min(), us.max(), len(us), float(np.median(us)) * 1e-6 * SPEC_BW / nbytes,
                    float(np.median(us)) * 1e-6 * COPY_BW / nbytes, float(np.median(dec))))
    feature(say, args.reps, dev)
    say()
    say("Interpolation error on the committed triples (reported, not asserted):")
    for res in ("240", "480"):
        interpolation(res, say, dev)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
