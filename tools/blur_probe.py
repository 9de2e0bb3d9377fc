#!/usr/bin/env python3
"""Cost of synthetic motion blur (tensors.motion_blur -> papof_motion_blur_tensor, one k_motion_blur launch) against the
composition it replaces, on one device.

The composition is what the library offered before: two `interpolate` calls on the video's pairs with float64 out (the
samples before each frame, the samples after it), and the weighted sum in torch -- each side's K / 2 frames reduced in one
multiply and one sum over the sample axis, the sums divided and converted to uint8 (a few launches, not one per sample).

Two videos, uint8 NHWC frames (3 channels), float64 flows, the mask of their forward-backward check, uint8 out, K = 16
samples of a centred box shutter of 0.5 frames:
  1080p   3 frames of 1920x1080 (the middle frame has both sides, the end frames one);
  240     32 frames of 240x135 made from the committed frames.
Each with two kinds of flows: smooth fields of about 2 pixels (a pixel's 8 samples on a side stay in one or two bilinear
cells: the held taps are reused) and independent uniform random flows of up to 40 pixels per component and pixel (most
samples in another cell, and no locality between neighbouring lanes).  The fused call is timed with the held taps (the
default) and with PAPOF_BLUR_REUSE=0 (every sample gathers its taps: the kernel before any gain from reuse).

Wall times are call + synchronise, median of --reps after warm-up.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o blur -- python3 tools/blur_probe.py --kernel-only
    python3 tools/blur_probe.py --kernel-stats DIR --out profiles/blur_probe.txt
(--kernel-only makes, per case, --reps fused calls with the held taps and --reps without, and after all of those --reps
compositions per case; --kernel-stats assigns the k_motion_blur dispatches in that order and, to each composition, its
equal share of the kernels dispatched after the last k_motion_blur.)"""
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

from papteam_opticalflow_amd.tensors import blur_schedule, fb_consistency, interpolate, motion_blur  # noqa: E402

SHUTTER, K = 0.5, 16


def smooth_flows(B, H, W, seed, amp=2.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(B, 2, H // 64 + 2, W // 64 + 2, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.05 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def random_flows(B, H, W, seed, amp=40.0):
    g = torch.Generator().manual_seed(seed)
    fw = (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) * 2 - 1) * amp
    bw = (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) * 2 - 1) * amp
    return fw, bw


def videos(dev):
    import cases
    g = torch.Generator().manual_seed(7)
    big = torch.randint(0, 256, (3, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    small = torch.from_numpy(np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(32)])).to(dev)
    out = []
    for name, v in (("1920x1080, 3 frames", big), ("240x135, 32 frames", small)):
        T, H, W, _ = v.shape
        for kind, make in (("smooth 2-pixel flows", smooth_flows), ("random 40-pixel flows", random_flows)):
            fw, bw = (f.to(dev) for f in make(T - 1, H, W, 8))
            out.append(("%s, %s" % (name, kind), v, fw, bw, fb_consistency(fw, bw)))
    return out


def fused(v, fw, bw, occ, reuse=True):
    if reuse:
        os.environ.pop("PAPOF_BLUR_REUSE", None)
    else:
        os.environ["PAPOF_BLUR_REUSE"] = "0"  # read by the library at every call
    try:
        return motion_blur(v, fw, bw, shutter=SHUTTER, samples=K, occlusion=occ, layout="NHWC")
    finally:
        os.environ.pop("PAPOF_BLUR_REUSE", None)


def composition(v, fw, bw, occ):
    """motion_blur's result from interpolate's float64 frames: uint8 NHWC in and out"""
    off, w = blur_schedule(SHUTTER, K)
    dev = v.device
    neg = [(1.0 + o, x) for o, x in zip(off, w) if o < 0]
    pos = [(o, x) for o, x in zip(off, w) if o > 0]
    mid = sum(x for o, x in zip(off, w) if o == 0)
    T = v.shape[0]
    acc = (v.double() / 255.0) * mid
    wsum = torch.full((T,), float(mid), dtype=torch.float64, device=dev)
    for side, sl in ((neg, slice(1, T)), (pos, slice(0, T - 1))):
        if not side:
            continue
        fr = interpolate(v[:-1], v[1:], fw, bw, [t for t, _ in side], occlusion=occ, layout="NHWC", out_dtype=torch.float64)
        ws = torch.tensor([x for _, x in side], dtype=torch.float64, device=dev)
        acc[sl] += (fr * ws.view(1, -1, 1, 1, 1)).sum(1)
        wsum[sl] += ws.sum()
    out = acc / wsum.view(-1, 1, 1, 1)
    return torch.clamp(torch.round(255.0 * out), 0, 255).to(torch.uint8)


def wall(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt.append(time.perf_counter() - t0)
    return float(np.median(dt)), min(dt), max(dt)


def kernel_times(path, n_cases, reps):
    """per case: (durations (us) of the fused dispatches with the held taps, without them, per-call sums of the
    composition's kernels, launches per composition), and the register counts of k_motion_blur"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        regs = tuple(row.get(k, "?") for k in ("vgpr_count", "accum_vgpr_count", "sgpr_count"))
        rows.append((int(row["start_timestamp"]), (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3,
                     "k_motion_blur" in name, regs))
    rows.sort()
    blur = [i for i, r in enumerate(rows) if r[2]]
    if len(blur) != 2 * n_cases * reps:
        raise SystemExit("expected %d k_motion_blur dispatches, found %d" % (2 * n_cases * reps, len(blur)))
    rest = [r[1] for r in rows[blur[-1] + 1:]]
    per, left = divmod(len(rest), n_cases * reps)
    if left or not per:
        raise SystemExit("%d kernels after the last k_motion_blur do not divide into %d compositions" % (len(rest), n_cases * reps))
    out = []
    for c in range(n_cases):
        d = [rows[i][1] for i in blur[2 * c * reps:2 * (c + 1) * reps]]
        comp = [sum(rest[(c * reps + j) * per:(c * reps + j + 1) * per]) for j in range(reps)]
        out.append((d[:reps], d[reps:], comp, per))
    return out, sorted({rows[i][3] for i in blur})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run the calls only, in the order --kernel-stats expects")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = videos(dev)
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, v, fw, bw, occ in cases:
            for reuse in (True, False):
                for _ in range(args.reps):
                    fused(v, fw, bw, occ, reuse)
                torch.cuda.synchronize()
        for _, v, fw, bw, occ in cases:
            for _ in range(args.reps):
                composition(v, fw, bw, occ)
            torch.cuda.synchronize()
        return
    ks, regs = kernel_times(args.kernel_stats, len(cases), args.reps) if args.kernel_stats else (None, None)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Motion blur on one %s device: motion_blur (one k_motion_blur launch) against the composition of two interpolate "
        "calls to float64 and the weighted sum in torch.  uint8 NHWC frames (C = 3), float64 flows, a mask, uint8 out, "
        "K = %d samples, shutter %.1f.  Wall: call + synchronise, median (min, max) of %d after warm-up." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], K, SHUTTER, args.reps))
    if regs:
        say("k_motion_blur<uint8, 3 channels> registers in the trace (VGPR_Count, Accum_VGPR_Count, SGPR_Count): %s" % (
            ", ".join("(%s)" % ", ".join(r) for r in regs)))
    for i, (what, v, fw, bw, occ) in enumerate(cases):
        say()
        say("%s: %d output pixels" % (what, v.shape[0] * v.shape[1] * v.shape[2]))
        res = {}
        on = wall(lambda: res.__setitem__("on", fused(v, fw, bw, occ, True)), args.reps)
        off = wall(lambda: res.__setitem__("off", fused(v, fw, bw, occ, False)), args.reps)
        comp = wall(lambda: res.__setitem__("c", composition(v, fw, bw, occ)), max(3, args.reps // 2))
        assert torch.equal(res["on"], res["off"])
        same = float((res["c"] == res["on"]).double().mean())
        say("  motion_blur, held taps     wall %9.1f us  (%.1f, %.1f)" % tuple(1e6 * x for x in on))
        say("  motion_blur, no reuse      wall %9.1f us  (%.1f, %.1f)   (the same bytes)" % tuple(1e6 * x for x in off))
        say("  composition                wall %9.1f us  (%.1f, %.1f)   (%.4f of the output bytes equal the kernel's)" % (
            tuple(1e6 * x for x in comp) + (same,)))
        say("  wall: fused / composition = %.3f with the held taps, %.3f without" % (on[0] / comp[0], off[0] / comp[0]))
        if ks:
            d_on, d_off, d_c, per = ks[i]
            a_on, a_off, a_c = float(np.mean(d_on)), float(np.mean(d_off)), float(np.mean(d_c))
            say("  rocprofv3 --kernel-trace, %d calls each: k_motion_blur %.1f us with the held taps (min %.1f, max %.1f), "
                "%.1f us without (min %.1f, max %.1f); the composition's %d kernels %.1f us (min %.1f, max %.1f)" % (
                    len(d_on), a_on, min(d_on), max(d_on), a_off, min(d_off), max(d_off), per, a_c, min(d_c), max(d_c)))
            say("  kernel time: fused / composition = %.3f with the held taps, %.3f without; reuse saves %.1f %% of the kernel"
                % (a_on / a_c, a_off / a_c, 100.0 * (1.0 - a_on / a_off)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
