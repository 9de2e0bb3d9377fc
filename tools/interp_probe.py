#!/usr/bin/env python3
"""Cost of frame interpolation (tensors.interpolate -> papof_interp_tensor, one k_interp launch) against its byte floor and
against the same rule written with PyTorch's grid_sample in float64, on one device.

Three cases, uint8 NHWC frames (3 channels), float64 flows, a mask, uint8 out:
  1080p K=1   one 1920x1080 pair, t = 0.5;
  1080p K=7   the same pair at t = 1/8 .. 7/8;
  240 B=32    32 pairs of 240x135 made from the committed frames, t = 0.5.
Flows are smooth random fields (bw = -fw + noise) of a few pixels, so that nearly every sample lands inside the image; the
mask is the forward-backward check of the flows (fb_consistency).

Byte floor per pixel and pair: both flows read once (32 B), both frames and both mask channels read once (2 C + 2 B), the
output written once (K C B); over 8 TB/s (spec) and over 6.3 TB/s (a measured copy).  Wall times are call + synchronise,
median of --reps after warm-up.  The grid_sample version computes the same weights and branches in float64 from the uint8
frames (bilinear, border padding, align_corners=True: positions agree with the kernel's rule inside the image, not bit for
bit); the share of its output bytes that equal the kernel's is printed.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o interp -- python3 tools/interp_probe.py --kernel-only
    python3 tools/interp_probe.py --kernel-stats DIR --out profiles/interp_probe.txt
(--kernel-stats: the directory rocprofv3 wrote, searched for *kernel_trace.csv; the dispatches of k_interp are assigned to
the cases in the order the --kernel-only run makes them: --reps per case.)"""
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

from papteam_opticalflow_amd.tensors import fb_consistency, interpolate  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12


def flows(B, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(B, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def case_1080(dev, K):
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 256, (1, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    b = torch.randint(0, 256, (1, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    fw, bw = (f.to(dev) for f in flows(1, 1080, 1920, 8))
    times = [0.5] if K == 1 else [(j + 1) / (K + 1) for j in range(K)]
    return "1920x1080, 1 pair, K = %d" % K, a, b, fw, bw, fb_consistency(fw, bw), times


def case_240(dev):
    import cases
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    fr = np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(33)])
    v = torch.from_numpy(fr).to(dev)
    fw, bw = (f.to(dev) for f in flows(32, 135, 240, 9))
    return "240x135, 32 pairs, K = 1", v[:-1], v[1:], fw, bw, fb_consistency(fw, bw), [0.5]


def floor_bytes(a, K):
    B, H, W, C = a.shape
    return B * H * W * (32 + 2 * C + 2 + K * C)


def torch_interp(a, b, fw, bw, occ, times):
    """the rule of papof_interp_tensor with grid_sample and elementwise ops, uint8 NHWC in, uint8 (B, K, H, W, C) out"""
    B, H, W, C = a.shape
    I0 = a.permute(0, 3, 1, 2).double() / 255.0
    I1 = b.permute(0, 3, 1, 2).double() / 255.0
    O = occ.double()
    y, x = torch.meshgrid(torch.arange(H, device=a.device, dtype=torch.float64),
                          torch.arange(W, device=a.device, dtype=torch.float64), indexing="ij")

    def sample(img, X, Y):
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (H - 1)) - 1], -1)
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    outs = []
    for t in times:
        s = 1.0 - t
        f0 = (t * t) * bw - (s * t) * fw
        f1 = (s * s) * fw - (s * t) * bw
        X0, Y0, X1, Y1 = x + f0[:, 0], y + f0[:, 1], x + f1[:, 0], y + f1[:, 1]
        in0 = ((X0 >= 0) & (X0 <= W - 1) & (Y0 >= 0) & (Y0 <= H - 1)).unsqueeze(1)
        in1 = ((X1 >= 0) & (X1 <= W - 1) & (Y1 >= 0) & (Y1 <= H - 1)).unsqueeze(1)
        g0, g1 = sample(I0, X0, Y0), sample(I1, X1, Y1)
        o0, o1 = sample(O[:, :1], X0, Y0), sample(O[:, 1:], X1, Y1)
        both = in0 & in1
        w0 = torch.where(in0, s * (1 - torch.where(both, o1, 0.0)), 0.0)
        w1 = torch.where(in1, t * (1 - torch.where(both, o0, 0.0)), 0.0)
        den = w0 + w1
        fall = (s * g0 * in0 + t * g1 * in1) / (s * in0 + t * in1)
        out = torch.where(den > 0, (w0 * g0 + w1 * g1) / den, torch.where(in0 | in1, fall, s * I0 + t * I1))
        outs.append(torch.clamp(torch.round(255.0 * out), 0, 255).to(torch.uint8).permute(0, 2, 3, 1))
    return torch.stack(outs, 1)


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
    """per case: the durations (us) of its k_interp dispatches, from rocprofv3's kernel trace in dispatch order"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        if "k_interp" in row.get("kernel_name", row.get("name", "")):
            rows.append((int(row["start_timestamp"]), (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    rows.sort()
    if len(rows) != n_cases * reps:
        raise SystemExit("expected %d k_interp dispatches, found %d" % (n_cases * reps, len(rows)))
    return [[d for _, d in rows[i * reps:(i + 1) * reps]] for i in range(n_cases)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="run interpolate only, --reps times per case (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = [case_1080(dev, 1), case_1080(dev, 7), case_240(dev)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, a, b, fw, bw, occ, times in cases:
            for _ in range(args.reps):
                interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC")
            torch.cuda.synchronize()
        return
    ks = kernel_times(args.kernel_stats, len(cases), args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Frame interpolation on one %s device: interpolate (one k_interp launch) against its byte floor and against the "
        "same rule with torch grid_sample in float64.  uint8 NHWC frames (C = 3), float64 flows, a mask, uint8 out.  Wall: "
        "call + synchronise, median (min, max) of %d after warm-up." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for i, (what, a, b, fw, bw, occ, times) in enumerate(cases):
        K = len(times)
        nbytes = floor_bytes(a, K)
        floor_us = 1e6 * nbytes / SPEC_BW
        say()
        say("%s: %d output pixels per time" % (what, a.shape[0] * a.shape[1] * a.shape[2]))
        say("  byte floor: %d B per pixel = %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (
            nbytes // (a.shape[0] * a.shape[1] * a.shape[2]), nbytes / 1e6, floor_us, 1e6 * nbytes / COPY_BW))
        res = {}
        med, lo, hi = wall(lambda: res.__setitem__("k", interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC")),
                           args.reps)
        say("  interpolate           wall %9.1f us  (%.1f, %.1f)" % (1e6 * med, 1e6 * lo, 1e6 * hi))
        med_t, lo_t, hi_t = wall(lambda: res.__setitem__("t", torch_interp(a, b, fw, bw, occ, times)),
                                 max(3, args.reps // 4))
        same = float((res["t"] == res["k"]).double().mean())
        say("  grid_sample, float64  wall %9.1f us  (%.1f, %.1f)   (%.1f x interpolate; %.4f of the output bytes equal)" % (
            1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, med_t / med, same))
        if ks:
            d = ks[i]
            avg = float(np.mean(d))
            say("  k_interp (rocprofv3 --kernel-trace, %d dispatches): average %.1f us (median %.1f, min %.1f, max %.1f) = "
                "%.2f x the 8 TB/s floor, %.2f x the 6.3 TB/s one; %.2f TB/s of floor bytes" % (
                    len(d), avg, float(np.median(d)), min(d), max(d), avg / floor_us, avg / (1e6 * nbytes / COPY_BW),
                    nbytes / (avg * 1e-6) / 1e12))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
