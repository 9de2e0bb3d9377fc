#!/usr/bin/env python3
"""Cost of motion-compensated temporal denoising (tensors.temporal_filter -> papof_temporal_filter_tensor, one
k_temporal_filter launch) against its byte floors and against the same rule written with PyTorch's grid_sample in float64,
on one device.

Three cases, uint8 NHWC frames (3 channels), float64 flows, sigma and the check at their defaults, uint8 out:
  1080p T=16 R=2   sixteen 1920x1080 frames, radius 2;
  1080p T=16 R=4   the same video, radius 4;
  240 T=101 R=2    101 frames of 240x135 made from the committed frames, radius 2.
Flows are smooth random fields (bw = -fw + noise) of a few pixels, so that nearly every chain survives its hops.

Byte floors per call: compulsory -- the frames and both flows read once, out and support written once
(T H W (2 C + 1) + 2 (T - 1) H W 16 bytes); (2R+1) reads -- what the lanes ask for without any reuse between them: each
frame read by the 2R + 1 pixels whose chains visit it (2R + 1 times), each pair's flows by the 2R chains that cross it
(2R times; the bilinear taps of one sample counted once), out and support once.  Both over 8 TB/s (spec) and 6.3 TB/s
(a measured copy).  Wall times are call + synchronise, median of --reps after warm-up.  The grid_sample version follows
the same chains in float64 with grid_sample (bilinear, border padding, align_corners=True: positions agree with the
kernel's rule inside the image, the arithmetic is not bit for bit the kernel's); the share of its output bytes that equal
the kernel's is printed.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o denoise -- python3 tools/denoise_probe.py --kernel-only
    python3 tools/denoise_probe.py --kernel-stats DIR --out profiles/denoise_probe.txt
(--kernel-stats: the directory rocprofv3 wrote, searched for *kernel_trace.csv; the dispatches of k_temporal_filter are
assigned to the cases in the order the --kernel-only run makes them: --reps per case.)"""
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

from papteam_opticalflow_amd.tensors import CONSISTENCY, temporal_filter  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12
SIGMA = temporal_filter.__kwdefaults__["sigma"]


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def case_1080(dev, R, video=[]):
    if not video:
        g = torch.Generator().manual_seed(7)
        v = torch.randint(0, 256, (16, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
        video.append((v,) + tuple(f.to(dev) for f in flows(15, 1080, 1920, 8)))
    v, fw, bw = video[0]
    return "1920x1080, T = 16, R = %d" % R, v, fw, bw, R


def case_240(dev):
    import cases
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    fr = np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(101)])
    fw, bw = (f.to(dev) for f in flows(100, 135, 240, 9))
    return "240x135, T = 101, R = 2", torch.from_numpy(fr).to(dev), fw, bw, 2


def floors(v, R):
    """(compulsory bytes, (2R+1)-reads bytes) of a call"""
    T, H, W, C = v.shape
    frames, fl, outs = T * H * W * C, 2 * (T - 1) * H * W * 16, T * H * W * (C + 1)
    return frames + fl + outs, (2 * R + 1) * frames + 2 * R * fl + outs


def torch_filter(v, fw, bw, R, sigma, alphas):
    """the rule of papof_temporal_filter_tensor with grid_sample and elementwise ops, uint8 NHWC in, uint8 NHWC out"""
    T, H, W, C = v.shape
    a1, a2 = alphas
    I = v.permute(0, 3, 1, 2).double() / 255.0
    y, x = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float64),
                          torch.arange(W, device=v.device, dtype=torch.float64), indexing="ij")

    def sample(img, X, Y):
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (H - 1)) - 1], -1)
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    num, den = I.clone(), torch.ones(T, 1, H, W, dtype=torch.float64, device=v.device)
    for d in (1, -1):
        X, Y = x.expand(T, H, W).clone(), y.expand(T, H, W).clone()
        alive = torch.ones(T, H, W, dtype=torch.bool, device=v.device)
        for j in range(1, R + 1):
            if T - j < 1:
                break
            ts = torch.arange(0, T - j, device=v.device) if d > 0 else torch.arange(j, T, device=v.device)
            pairs, src = (ts + j - 1, ts + j) if d > 0 else (ts - j, ts - j)
            f, b = (fw, bw) if d > 0 else (bw, fw)
            uv = sample(f[pairs], X[ts], Y[ts])
            nX, nY = X[ts] + uv[:, 0], Y[ts] + uv[:, 1]
            al = alive[ts] & (nX >= 0) & (nX <= W - 1) & (nY >= 0) & (nY <= H - 1)
            buv = sample(b[pairs], nX, nY)
            du, dv = uv[:, 0] + buv[:, 0], uv[:, 1] + buv[:, 1]
            mag = (uv * uv).sum(1) + (buv * buv).sum(1)
            al = al & (du * du + dv * dv <= a1 * mag + a2)
            g = sample(I[src], nX, nY)
            D = ((g - I[ts]) ** 2).mean(1, keepdim=True)
            w = torch.where(al.unsqueeze(1), 1.0 / (1.0 + D / (sigma * sigma)), 0.0)
            num[ts] += w * g
            den[ts] += w
            X[ts], Y[ts], alive[ts] = nX, nY, al
    return torch.clamp(torch.round(255.0 * (num / den)), 0, 255).to(torch.uint8).permute(0, 2, 3, 1)


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
    """per case: the durations (us) of its k_temporal_filter dispatches, from rocprofv3's kernel trace in dispatch order"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        if "k_temporal_filter" in row.get("kernel_name", row.get("name", "")):
            rows.append((int(row["start_timestamp"]), (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    rows.sort()
    if len(rows) != n_cases * reps:
        raise SystemExit("expected %d k_temporal_filter dispatches, found %d" % (n_cases * reps, len(rows)))
    return [[d for _, d in rows[i * reps:(i + 1) * reps]] for i in range(n_cases)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true",
                    help="run temporal_filter only, --reps times per case (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None,
                    help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = [case_1080(dev, 2), case_1080(dev, 4), case_240(dev)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, v, fw, bw, R in cases:
            for _ in range(args.reps):
                temporal_filter(v, fw, bw, radius=R, layout="NHWC")
            torch.cuda.synchronize()
        return
    ks = kernel_times(args.kernel_stats, len(cases), args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Temporal denoising on one %s device: temporal_filter (one k_temporal_filter launch) against its byte floors and "
        "against the same rule with torch grid_sample in float64.  uint8 NHWC frames (C = 3), float64 flows, sigma = %g, "
        "consistency %s, uint8 out.  Wall: call + synchronise, median (min, max) of %d after warm-up." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], SIGMA, CONSISTENCY, args.reps))
    for i, (what, v, fw, bw, R) in enumerate(cases):
        T, H, W, C = v.shape
        comp, reads = floors(v, R)
        say()
        say("%s: %d output pixels" % (what, T * H * W))
        for name, nb in (("compulsory", comp), ("(2R+1)-reads", reads)):
            say("  %-12s floor: %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (
                name, nb / 1e6, 1e6 * nb / SPEC_BW, 1e6 * nb / COPY_BW))
        res = {}
        med, lo, hi = wall(lambda: res.__setitem__("k", temporal_filter(v, fw, bw, radius=R, layout="NHWC").video),
                           args.reps)
        say("  temporal_filter       wall %10.1f us  (%.1f, %.1f)   %.1f us per frame" % (
            1e6 * med, 1e6 * lo, 1e6 * hi, 1e6 * med / T))
        med_t, lo_t, hi_t = wall(lambda: res.__setitem__("t", torch_filter(v, fw, bw, R, SIGMA, CONSISTENCY)),
                                 max(3, args.reps // 4))
        same = float((res["t"] == res["k"]).double().mean())
        say("  grid_sample, float64  wall %10.1f us  (%.1f, %.1f)   (%.1f x temporal_filter; not bit-exact: %.4f of the "
            "output bytes equal)" % (1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, med_t / med, same))
        if ks:
            d = ks[i]
            avg = float(np.mean(d))
            say("  k_temporal_filter (rocprofv3 --kernel-trace, %d dispatches): average %.1f us (median %.1f, min %.1f, "
                "max %.1f), %.1f us per frame" % (len(d), avg, float(np.median(d)), min(d), max(d), avg / T))
            for name, nb in (("compulsory", comp), ("(2R+1)-reads", reads)):
                say("    %-12s %.2f x the 8 TB/s floor, %.2f x the 6.3 TB/s one; %.2f TB/s of floor bytes" % (
                    name, avg / (1e6 * nb / SPEC_BW), avg / (1e6 * nb / COPY_BW), nb / (avg * 1e-6) / 1e12))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
