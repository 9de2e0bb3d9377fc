#!/usr/bin/env python3
"""Cost of multi-frame super-resolution (tensors.super_resolve -> papof_super_resolve_tensor: per round a clear,
k_sr_accumulate, k_sr_resolve and `iters` k_sr_backproject) against its byte floors and against the same pipeline written in
PyTorch (grid_sample chains, index_put_(accumulate=True) in float64, interpolate(bicubic) for the base, avg_pool2d /
interpolate(bilinear) for the back-projection).

Three cases, uint8 NHWC frames (3 channels) made from the committed frames, their own float64 flows (flow_video_fb), scale
2, radius 2, the default sigma, check and prior, uint8 out, each with iters 0 and 2:
  960x540 x 5 frames, 1920x1080 x 5 frames, 240x135 x 101 frames.

Bytes.  k_sr_accumulate, per round: every source frame (C bytes per pixel) and both flow fields of every pair it hops
through (2 x 16 bytes per pixel) once, plus the ADDED bytes: 4 taps x (C + 1) x 8 bytes per deposit, one deposit per (source
pixel, target within the radius) -- counted as if every chain lived.  k_sr_resolve, per fine pixel: (C + 1) x 8 read, 8
(coverage) and 8 C (X) or C (the typed output) written; the frame's C / S^2.  k_sr_backproject, per fine pixel and step: 8 C
read, 8 C or C written; the frame's C / S^2.  Floors are those bytes over 8 TB/s; the added bytes over the kernel's time
stand beside the 0.89 TB/s that k_splat reached (profiles/splat_probe.txt).  Wall times are call + synchronise, median of
--reps after warm-up, with the profiler off.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o sr -- python3 tools/superres_probe.py --kernel-only
    python3 tools/superres_probe.py --kernel-stats DIR --out profiles/superres_probe.txt
(--kernel-stats: the directory rocprofv3 wrote, searched for *kernel_trace.csv; the dispatches are assigned to the cases in
the order the --kernel-only run makes them: per case --reps calls with iters 0, then --reps with iters 2.)"""
import argparse
import csv
import glob
import io
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from papteam_opticalflow_amd import capi  # noqa: E402
from papteam_opticalflow_amd.tensors import flow_video_fb, super_resolve  # noqa: E402

SPEC_BW, SPLAT_RATE = 8.0e12, 0.89e12
S, R, C = 2, 2, 3
KERNELS = {"k_sr_accumulate": r"\bk_sr_accumulate<", "k_sr_resolve": r"\bk_sr_resolve<", "k_sr_backproject": r"\bk_sr_backproject<"}
ITERS = (0, 2)


def make_case(dev, res, T, levels):
    import cases
    a, b = cases.load_frame_u8(res, 1), cases.load_frame_u8(res, 2)
    v = torch.from_numpy(np.stack([np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(T)])).to(dev)
    fw, bw = [], []
    for t0 in range(0, T - 1, 32):  # (the flows in chunks of 32 pairs)
        fb = flow_video_fb(v[t0:t0 + 33], levels, layout="NHWC", consistency=None)
        fw.append(fb.flow_fw)
        bw.append(fb.flow_bw)
    return "%sx%s x %d frames" % (cases.SIZES[res][1], cases.SIZES[res][0], T), v, torch.cat(fw), torch.cat(bw)


def rounds(T, H, W, iters):
    """(targets per round, [(t0, t1)]) of the default workspace"""
    per = 8 * S * S * H * W * ((C + 1) + (2 * C if iters else 0))
    G = capi.load().papof_sr_workspace(T, H, W, C, S, iters) // per
    return G, [(t0, min(T, t0 + G)) for t0 in range(0, T, G)]


def accumulate_bytes(T, H, W, groups):
    """(bytes read at least once, bytes added) of k_sr_accumulate over the rounds"""
    read = added = 0
    for t0, t1 in groups:
        s0, s1 = max(0, t0 - R), min(T, t1 + R)
        read += (s1 - s0) * H * W * C + max(0, s1 - s0 - 1) * H * W * 32
        deposits = sum(min(T, t + R + 1) - max(0, t - R) for t in range(t0, t1))
        added += deposits * H * W * 4 * (C + 1) * 8
    return read, added


def _sample(img, X, Y):
    """img (1, K, H, W) sampled bilinearly at the points (X, Y) (H, W) -> (K, H, W)"""
    H, W = img.shape[-2:]
    grid = torch.stack((2 * X / max(W - 1, 1) - 1, 2 * Y / max(H - 1, 1) - 1), -1)[None]
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]


def torch_sr(v, fw, bw, iters, sigma=0.15, a1=0.01, a2=0.5, prior=0.05):
    """the pipeline in float64 torch operations (float atomics: the last bits change from run to run)"""
    T, H, W, _ = v.shape
    Y = (v.double() / 255.0).permute(0, 3, 1, 2)
    FH, FW = S * H, S * W
    num = torch.zeros(T, C, FH * FW, dtype=torch.float64, device=v.device)
    den = torch.zeros(T, FH * FW, dtype=torch.float64, device=v.device)
    ys, xs = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float64),
                            torch.arange(W, device=v.device, dtype=torch.float64), indexing="ij")

    def deposit(t, X, Y_, w, vals):
        QX, QY = S * (X + 0.5) - 0.5, S * (Y_ + 0.5) - 0.5
        x0, y0 = torch.floor(QX), torch.floor(QY)
        fx, fy = QX - x0, QY - y0
        x0, y0 = x0.long(), y0.long()
        for m in (0, 1):
            for n in (0, 1):
                tx, ty = x0 + n, y0 + m
                wb = w * ((fy if m else 1 - fy) * (fx if n else 1 - fx))
                keep = ((wb > 0) & (tx >= 0) & (tx < FW) & (ty >= 0) & (ty < FH)).reshape(-1)
                idx = (ty * FW + tx).reshape(-1)[keep]
                wk = wb.reshape(-1)[keep]
                den[t].index_put_((idx,), wk, accumulate=True)
                for c in range(C):
                    num[t, c].index_put_((idx,), wk * vals[c].reshape(-1)[keep], accumulate=True)

    for k in range(T):
        deposit(k, xs, ys, torch.ones_like(xs), Y[k])
        for d in (1, -1):
            X, Y_, alive = xs, ys, torch.ones_like(xs, dtype=torch.bool)
            for n in range(1, min(R, T - 1 - k if d > 0 else k) + 1):
                pair = k + n - 1 if d > 0 else k - n
                f, b = (fw, bw) if d > 0 else (bw, fw)
                uv = _sample(f[pair:pair + 1], X, Y_)
                X, Y_ = X + uv[0], Y_ + uv[1]
                alive = alive & (X >= 0) & (X <= W - 1) & (Y_ >= 0) & (Y_ <= H - 1)
                back = _sample(b[pair:pair + 1], X, Y_)
                e = (uv + back).pow(2).sum(0)
                alive = alive & (e <= a1 * (uv.pow(2).sum(0) + back.pow(2).sum(0)) + a2)
                g = _sample(Y[k + d * n:k + d * n + 1], X, Y_)
                w = 1.0 / (1.0 + (Y[k] - g).pow(2).mean(0) / (sigma * sigma))
                deposit(k + d * n, X, Y_, torch.where(alive, w, torch.zeros_like(w)), Y[k])
    base = F.interpolate(Y, scale_factor=S, mode="bicubic", align_corners=False)
    X = (num.view(T, C, FH, FW) + prior * base) / (den.view(T, 1, FH, FW) + prior)
    for _ in range(iters):
        X = X + F.interpolate(Y - F.avg_pool2d(X, S), scale_factor=S, mode="bilinear", align_corners=False)
    return (255.0 * X).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)


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


def kernel_times(path, counts, reps):
    """per kernel: for each (case, iters) in order the per-call sums (us) of its dispatches, from rocprofv3's kernel trace;
    counts[kernel]: dispatches per call for each (case, iters)"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        for k, pat in KERNELS.items():
            if re.search(pat, name):
                rows[k].append((int(row["start_timestamp"]), (int(row["end_timestamp"]) - int(row["start_timestamp"])) / 1e3))
    out = {}
    for k, r in rows.items():
        r = [d for _, d in sorted(r)]
        if len(r) != reps * sum(counts[k]):
            raise SystemExit("expected %d %s dispatches, found %d" % (reps * sum(counts[k]), k, len(r)))
        out[k], at = [], 0
        for n in counts[k]:
            out[k].append([sum(r[at + i * n:at + (i + 1) * n]) for i in range(reps)] if n else [])
            at += reps * n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run the calls only, --reps times per case (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases_ = [make_case(dev, "960", 5, 5), make_case(dev, "1920", 5, 5), make_case(dev, "240", 101, 4)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, v, fw, bw in cases_:
            for iters in ITERS:
                for _ in range(args.reps):
                    super_resolve(v, fw, bw, S, radius=R, iters=iters, layout="NHWC")
                torch.cuda.synchronize()
        return
    plan = [(v.shape[0], v.shape[1], v.shape[2], iters) for _, v, _, _ in cases_ for iters in ITERS]
    ks = None
    if args.kernel_stats:
        n_rounds = [len(rounds(*p)[1]) for p in plan]
        ks = kernel_times(args.kernel_stats, {"k_sr_accumulate": n_rounds, "k_sr_resolve": n_rounds,
                                              "k_sr_backproject": [n * p[3] for n, p in zip(n_rounds, plan)]}, args.reps)
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    def kernel_line(name, d, nbytes, added=None):
        avg = float(np.mean(d))
        s = "    %-16s per call: average %.1f us (median %.1f, min %.1f, max %.1f) = %.2f x its %.1f MB floor at 8 TB/s" % (
            name, avg, float(np.median(d)), min(d), max(d), avg / (1e6 * nbytes / SPEC_BW), nbytes / 1e6)
        if added:
            s += "; %.1f MB added = %.2f TB/s of added bytes (%.2f x k_splat's 0.89 TB/s)" % (
                added / 1e6, added / (avg * 1e-6) / 1e12, added / (avg * 1e-6) / SPLAT_RATE)
        say(s)
        return avg

    say("Multi-frame super-resolution on one %s device: super_resolve against its byte floors and against the same pipeline in "
        "float64 torch operations.  uint8 NHWC frames (C = 3), float64 flows of the frames themselves, scale 2, radius 2, "
        "sigma 0.15, check (0.01, 0.5), prior 0.05, uint8 out.  Wall: call + synchronise, median (min, max) of %d after "
        "warm-up, profiler off; kernel times from a rocprofv3 --kernel-trace run of their own."
        % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for i, (what, v, fw, bw) in enumerate(cases_):
        T, H, W, _ = v.shape
        fine = T * S * S * H * W
        say()
        say("%s -> %dx%d: %d source pixels, %d fine pixels" % (what, S * W, S * H, T * H * W, fine))
        for j, iters in enumerate(ITERS):
            G, groups = rounds(T, H, W, iters)
            walked = sum(min(T, t1 + R) - max(0, t0 - R) for t0, t1 in groups)
            med, lo, hi = wall(lambda: super_resolve(v, fw, bw, S, radius=R, iters=iters, layout="NHWC"), args.reps)
            say("  iters %d: rounds of %d targets (%d rounds; %d source frames walked for %d: chain work x %.2f), workspace "
                "%.0f MB" % (iters, G, len(groups), walked, T, walked / T,
                             capi.load().papof_sr_workspace(T, H, W, C, S, iters) / 1e6))
            say("    super_resolve        wall %10.1f us  (%.1f, %.1f) = %.1f us per frame" % (1e6 * med, 1e6 * lo, 1e6 * hi,
                                                                                             1e6 * med / T))
            med_t, lo_t, hi_t = wall(lambda: torch_sr(v, fw, bw, iters), max(2, args.reps // 5))
            say("    torch operations     wall %10.1f us  (%.1f, %.1f) = %.1f x super_resolve" % (1e6 * med_t, 1e6 * lo_t,
                                                                                                 1e6 * hi_t, med_t / med))
            if ks:
                read, added = accumulate_bytes(T, H, W, groups)
                t = kernel_line("k_sr_accumulate", ks["k_sr_accumulate"][2 * i + j], read + added, added)
                t += kernel_line("k_sr_resolve", ks["k_sr_resolve"][2 * i + j],
                                 fine * ((C + 1) * 8 + 8 + (8 * C if iters else C)) + T * H * W * C)
                if iters:
                    t += kernel_line("k_sr_backproject", ks["k_sr_backproject"][2 * i + j],
                                     fine * (8 * C * iters + 8 * C * (iters - 1) + C) + iters * T * H * W * C)
                say("    kernels per call %.1f us = %.1f us per frame (without the clear of %.0f MB per call)" % (
                    t, t / T, fine * (C + 1) * 8 / 1e6))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
