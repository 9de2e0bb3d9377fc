#!/usr/bin/env python3
"""Cost of video stabilization's two kernels (tensors.global_motion -> papof_motion_fit_tensor: k_motion_sums + k_motion_solve
per iteration; tensors.warp_affine -> papof_warp_affine_tensor: k_warp_affine) against their byte floors and against the same
rules written in PyTorch, on one device.

Three cases:
  fit 1080p    one 1920x1080 float64 flow with a mask, affine, 5 iterations;
  fit 240 x100 100 flows of 240x135, float64 with a mask, affine, 5 iterations;
  warp 1080p   16 uint8 NHWC 1920x1080 frames (C = 3), float64 matrices, uint8 out.
Byte floor: the fit reads 16 B of float64 flow and 1 B of mask per pixel and iteration; the warp reads each frame once and
writes each output once (6 B per pixel for 3 uint8 channels; the valid mask's byte is not counted).  Over 8 TB/s (spec) and
6.3 TB/s (a measured copy).  Wall times are call + synchronise, median of --reps after warm-up.  The torch versions: the fit as
an IRLS of torch.linalg.lstsq in float64 on the valid pixels (the same weights; not the same sums, so not the same bits);
the warp as affine_grid + grid_sample (bilinear, zeros padding, align_corners=True) in float32 on the frames / 255.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o stab -- python3 tools/stab_probe.py --kernel-only
    python3 tools/stab_probe.py --kernel-stats DIR --out profiles/stab_probe.txt"""
import argparse
import csv
import glob
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import global_motion, warp_affine  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12
ITERS = 5


def flows(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    f = torch.empty(B, 2, H, W, dtype=torch.float64)
    for i in range(B):
        L = torch.eye(2, dtype=torch.float64) + 0.01 * torch.randn(2, 2, generator=g, dtype=torch.float64)
        t = 2 * torch.randn(2, generator=g, dtype=torch.float64)
        f[i, 0] = L[0, 0] * x + L[0, 1] * y + t[0] - x
        f[i, 1] = L[1, 0] * x + L[1, 1] * y + t[1] - y
    f += 0.2 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    out = torch.rand(B, H, W, generator=g) < 0.2
    f[:, 0][out] += 30 * torch.rand(int(out.sum()), generator=g, dtype=torch.float64) - 15
    occ = (torch.rand(B, 2, H, W, generator=g) < 0.05)
    return f, occ


def torch_fit(f, occ, iters=ITERS, c=1.0):
    """the IRLS of papof_motion_fit_tensor (affine) with torch.linalg.lstsq in float64, pair by pair"""
    B, _, H, W = f.shape
    dev = f.device
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    cx, cy, s = (W - 1) / 2, (H - 1) / 2, max(W, H) / 2
    out = []
    for i in range(B):
        X, Y = x + f[i, 0], y + f[i, 1]
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1) & ~occ[i, 0]
        xs, ys, Xs, Ys = x[valid], y[valid], X[valid], Y[valid]
        A = torch.stack([(xs - cx) / s, (ys - cy) / s, torch.ones_like(xs)], 1)
        b = torch.stack([(Xs - cx) / s, (Ys - cy) / s], 1)
        w = torch.ones_like(xs)
        for _ in range(iters):
            sw = w.sqrt().unsqueeze(1)
            p = torch.linalg.lstsq(A * sw, b * sw).solution
            e2 = (s * (A @ p - b)).square().sum(1)
            w = 1.0 / (1.0 + e2 / (c * c))
        out.append(p)
    return torch.stack(out)


def torch_warp(fr, M):
    """affine_grid + grid_sample of uint8 NHWC frames by pixel matrices M, uint8 NHWC out"""
    B, H, W, C = fr.shape
    img = fr.permute(0, 3, 1, 2).float() / 255.0
    # pixel matrix -> normalised (align_corners=True): n = 2 p / (size - 1) - 1
    Sx, Sy = 2.0 / (W - 1), 2.0 / (H - 1)
    N = torch.tensor([[Sx, 0, -1], [0, Sy, -1], [0, 0, 1]], dtype=torch.float64, device=fr.device)
    Ni = torch.linalg.inv(N)
    Mh = torch.cat([M, torch.tensor([[[0, 0, 1.0]]], dtype=torch.float64, device=fr.device).expand(B, 1, 3)], 1)
    theta = (N @ Mh @ Ni)[:, :2].float()
    grid = torch.nn.functional.affine_grid(theta, (B, C, H, W), align_corners=True)
    out = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return torch.clamp(torch.round(255 * out), 0, 255).to(torch.uint8).permute(0, 2, 3, 1)


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


def kernel_times(path, names, n_cases, reps):
    """per case and kernel name: the durations (us) of its dispatches, from rocprofv3's kernel trace in dispatch order"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        for n in names:
            if n in name:
                rows.append((int(row["start_timestamp"]), n, (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    rows.sort()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="run the library calls only, --reps times per case")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    f1, o1 = (t.to(dev) for t in flows(1, 1080, 1920, 1))
    f2, o2 = (t.to(dev) for t in flows(100, 135, 240, 2))
    g = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 256, (16, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    th = 0.01 * torch.randn(16, generator=g, dtype=torch.float64)
    M = torch.zeros(16, 2, 3, dtype=torch.float64)
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = th.cos(), -th.sin(), th.sin(), th.cos()
    M[:, :, 2] = 3 * torch.randn(16, 2, generator=g, dtype=torch.float64)
    M = M.to(dev)
    cases = [("fit: 1920x1080, 1 pair, affine, %d iterations, float64 flow + mask" % ITERS,
              lambda: global_motion(f1, occlusion=o1, iters=ITERS), lambda: torch_fit(f1, o1), 1 * 1080 * 1920 * 17 * ITERS),
             ("fit: 240x135, 100 pairs, affine, %d iterations, float64 flow + mask" % ITERS,
              lambda: global_motion(f2, occlusion=o2, iters=ITERS), lambda: torch_fit(f2, o2), 100 * 135 * 240 * 17 * ITERS),
             ("warp: 16 uint8 NHWC frames of 1920x1080 (C = 3), float64 matrices, uint8 out",
              lambda: warp_affine(fr, M, layout="NHWC"), lambda: torch_warp(fr, M), 16 * 1080 * 1920 * 6)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, fn, _, _ in cases:
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
        return
    rows = kernel_times(args.kernel_stats, ["k_motion_sums", "k_motion_solve", "k_warp_affine"], len(cases),
                        args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Video stabilization kernels on one %s device against their byte floors and against PyTorch.  Wall: call + "
        "synchronise, median (min, max) of %d after warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
                                                                 args.reps))
    # the dispatches of the --kernel-only run, case by case: fit cases make 2 * ITERS launches per call, the warp one
    per_call = [2 * ITERS, 2 * ITERS, 1]
    at = 0
    for i, (what, fn, tfn, nbytes) in enumerate(cases):
        floor_us = 1e6 * nbytes / SPEC_BW
        say()
        say(what)
        say("  byte floor: %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (nbytes / 1e6, floor_us, 1e6 * nbytes / COPY_BW))
        med, lo, hi = wall(fn, args.reps)
        say("  library call          wall %9.1f us  (%.1f, %.1f)" % (1e6 * med, 1e6 * lo, 1e6 * hi))
        med_t, lo_t, hi_t = wall(tfn, max(3, args.reps // 4))
        say("  torch                 wall %9.1f us  (%.1f, %.1f)   (%.1f x the library call)" % (
            1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, med_t / med))
        if rows:
            n = per_call[i] * args.reps
            mine = rows[at:at + n]
            at += n
            by = {}
            for _, name, d in mine:
                by.setdefault(name, []).append(d)
            total = sum(d for _, _, d in mine) / args.reps
            for name, d in sorted(by.items()):
                say("  %-15s (rocprofv3 --kernel-trace, %d dispatches): average %.1f us (median %.1f, min %.1f, max %.1f)" % (
                    name, len(d), float(np.mean(d)), float(np.median(d)), min(d), max(d)))
            say("  kernels per call: %.1f us = %.2f x the 8 TB/s floor, %.2f x the 6.3 TB/s one" % (
                total, total / floor_us, total / (1e6 * nbytes / COPY_BW)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
