#!/usr/bin/env python3
"""Cost of forward warping (tensors.splat -> papof_splat_tensor: a clear, k_splat, k_splat_resolve) and of interpolation by
splatting (tensors.interpolate(method="splat") -> papof_interp_splat_tensor: a clear, two k_splat, k_interp_splat) against
their byte floors, against the same accumulation written with torch.Tensor.index_put_(accumulate=True) in float64, and
against k_interp on the same inputs; and the interpolation error of both methods on the committed frame triples.

Three cases, uint8 NHWC frames (3 channels), float64 flows and weights, uint8 out:
  1080p K=1   the committed 1920x1080 pair (frames 1 and 2) and its own flows (flow_pairs_fb, 5 levels), t = 0.5;
  1080p K=7   the same at t = 1/8 .. 7/8;
  240 B=32    32 pairs of 240x135 made from the committed frames and their own flows (4 levels), t = 0.5.
The weights are splat_weights of the flow call's warped frames.

Bytes per source pixel of k_splat: flow 16 + weight 8 + C read; 4 taps x (C + 1) x 8 B of atomic adds per time.  Per target
pixel of k_splat_resolve: (C + 1) x 8 read, C + 8 (coverage) written per time; of k_interp_splat: 2 x (C + 1) x 8 read, C
written per time.  Floors are those bytes over 8 TB/s (spec) and 6.3 TB/s (a measured copy); the atomic bytes over the
kernel's time are set against the 1.3 TB/s measured for 4-byte float atomics.  Wall times are call + synchronise, median of
--reps after warm-up.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o splat -- python3 tools/splat_probe.py --kernel-only
    python3 tools/splat_probe.py --kernel-stats DIR --out profiles/splat_probe.txt
(--kernel-stats: the directory rocprofv3 wrote, searched for *kernel_trace.csv; the dispatches are assigned to the cases in
the order the --kernel-only run makes them: per case --reps splat calls, --reps interpolations by splatting, --reps by
gathering.)"""
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

from papteam_opticalflow_amd.tensors import flow_pairs_fb, interpolate, interpolate_pairs, splat, splat_weights  # noqa: E402

SPEC_BW, COPY_BW, ATOMIC_BW = 8.0e12, 6.3e12, 1.3e12
KERNELS = {"k_splat": r"\bk_splat<", "k_splat_resolve": r"\bk_splat_resolve\b", "k_interp_splat": r"\bk_interp_splat<",
           "k_interp": r"\bk_interp<"}


def make_case(what, a, b, levels, times):
    fb = flow_pairs_fb(a, b, levels, layout="NHWC")
    ws = (splat_weights(a, fb.warpI2_fw, layout="NHWC"), splat_weights(b, fb.warpI2_bw, layout="NHWC"))
    return what, a, b, fb.flow_fw, fb.flow_bw, fb.occlusion, ws, times


def case_1080(dev, K, cache={}):
    import cases
    if "fb" not in cache:
        a, b = (torch.from_numpy(cases.load_frame_u8("1920", i)[None]).to(dev) for i in (1, 2))
        cache["fb"] = make_case("", a, b, 5, None)
    times = [0.5] if K == 1 else [(j + 1) / (K + 1) for j in range(K)]
    return ("1920x1080, 1 pair, K = %d" % K,) + cache["fb"][1:-1] + (times,)


def case_240(dev):
    import cases
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    fr = np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(33)])
    v = torch.from_numpy(fr).to(dev)
    return make_case("240x135, 32 pairs, K = 1", v[:-1], v[1:], 4, [0.5])


def torch_splat(x, flow, w, t):
    """the accumulation of papof_splat_tensor with index_put_(accumulate=True) in float64 (float atomics: the last bits
    change from run to run), uint8 NHWC in -> (num (B H W, C), den (B H W))"""
    B, H, W, C = x.shape
    xs = (x.double() / 255.0).reshape(-1, C)
    ys, xg = torch.meshgrid(torch.arange(H, device=x.device, dtype=torch.float64),
                            torch.arange(W, device=x.device, dtype=torch.float64), indexing="ij")
    X, Y = xg + t * flow[:, 0], ys + t * flow[:, 1]
    ok = (X > -1) & (X < W) & (Y > -1) & (Y < H) & (w > 0)
    x0, y0 = torch.floor(X), torch.floor(Y)
    fx, fy = X - x0, Y - y0
    x0, y0 = x0.long(), y0.long()
    base = torch.arange(B, device=x.device).view(B, 1, 1) * (H * W)
    num = torch.zeros(B * H * W, C, dtype=torch.float64, device=x.device)
    den = torch.zeros(B * H * W, dtype=torch.float64, device=x.device)
    for m in (0, 1):
        for n in (0, 1):
            tx, ty = x0 + n, y0 + m
            wb = w.clamp(max=1.0) * ((fy if m else 1 - fy) * (fx if n else 1 - fx))
            keep = (ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)).reshape(-1)
            idx = (base + ty * W + tx).reshape(-1)[keep]
            wk = wb.reshape(-1)[keep]
            den.index_put_((idx,), wk, accumulate=True)
            num.index_put_((idx,), wk[:, None] * xs[keep], accumulate=True)
    return num, den


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
    """per kernel and case: the durations (us) of its dispatches, from rocprofv3's kernel trace in dispatch order"""
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
    per = {"k_splat": 3, "k_splat_resolve": 1, "k_interp_splat": 1, "k_interp": 1}
    out = {}
    for k, r in rows.items():
        r = sorted(r)[-n_cases * reps * per[k]:]  # (the flow calls that make the inputs come first)
        if len(r) != n_cases * reps * per[k]:
            raise SystemExit("expected %d %s dispatches, found %d" % (n_cases * reps * per[k], k, len(r)))
        n = reps * per[k]
        out[k] = [[d for _, d in r[i * n:(i + 1) * n]] for i in range(n_cases)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="run the calls only, --reps times per case (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory (or kernel_trace.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases_ = [case_1080(dev, 1), case_1080(dev, 7), case_240(dev)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, a, b, fw, bw, occ, ws, times in cases_:
            for _ in range(args.reps):
                splat(a, fw, times, weight=ws[0], layout="NHWC")
            for _ in range(args.reps):
                interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC", method="splat", weights=ws)
            for _ in range(args.reps):
                interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC")
            torch.cuda.synchronize()
        return
    ks = kernel_times(args.kernel_stats, len(cases_), args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    def kernel_line(name, d, nbytes, atomic=None):
        avg = float(np.mean(d))
        s = "  %-15s (%d dispatches): average %.1f us (median %.1f, min %.1f, max %.1f) = %.2f x its %.1f MB floor at 8 TB/s, " \
            "%.2f x at 6.3 TB/s" % (name, len(d), avg, float(np.median(d)), min(d), max(d), avg / (1e6 * nbytes / SPEC_BW),
                                    nbytes / 1e6, avg / (1e6 * nbytes / COPY_BW))
        if atomic:
            s += "; %.1f MB of atomic adds = %.2f TB/s (%.2f x the 1.3 TB/s of float atomics)" % (
                atomic / 1e6, atomic / (avg * 1e-6) / 1e12, atomic / (avg * 1e-6) / ATOMIC_BW)
        say(s)
        return avg

    say("Forward warping on one %s device: splat and interpolate(method=\"splat\") against their byte floors, against "
        "index_put_(accumulate=True) in float64 and against interpolate(method=\"gather\").  uint8 NHWC frames (C = 3), "
        "float64 flows of the frames themselves, float64 weights, uint8 out.  Wall: call + synchronise, median (min, max) of "
        "%d after warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for i, (what, a, b, fw, bw, occ, ws, times) in enumerate(cases_):
        K = len(times)
        B, H, W, C = a.shape
        P = B * H * W
        say()
        say("%s: %d pixels per time" % (what, P))
        res = {}
        med, lo, hi = wall(lambda: res.__setitem__("s", splat(a, fw, times, weight=ws[0], layout="NHWC")), args.reps)
        say("  splat                  wall %9.1f us  (%.1f, %.1f)   holes: %.4f of the targets" % (
            1e6 * med, 1e6 * lo, 1e6 * hi, float((res["s"].coverage < 2.0 ** -24).double().mean())))
        med_t, lo_t, hi_t = wall(lambda: [torch_splat(a, fw, ws[0], t) for t in times], max(3, args.reps // 4))
        say("  index_put_, float64    wall %9.1f us  (%.1f, %.1f)   (%.1f x splat, without the division and the store)" % (
            1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, med_t / med))
        med_i, lo_i, hi_i = wall(lambda: interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC", method="splat",
                                                     weights=ws), args.reps)
        med_g, lo_g, hi_g = wall(lambda: interpolate(a, b, fw, bw, times, occlusion=occ, layout="NHWC"), args.reps)
        say("  interpolate, splat     wall %9.1f us  (%.1f, %.1f)" % (1e6 * med_i, 1e6 * lo_i, 1e6 * hi_i))
        say("  interpolate, gather    wall %9.1f us  (%.1f, %.1f)   (splat: %.2f x)" % (1e6 * med_g, 1e6 * lo_g, 1e6 * hi_g,
                                                                                       med_i / med_g))
        if ks:
            atomic = P * K * 4 * (C + 1) * 8
            d = ks["k_splat"][i]
            kernel_line("k_splat", d[:args.reps], P * (24 + C) + atomic, atomic)
            t_fb = kernel_line("k_splat x 2", [x + y for x, y in zip(d[args.reps::2], d[args.reps + 1::2])],
                               2 * (P * (24 + C) + atomic), 2 * atomic)
            kernel_line("k_splat_resolve", ks["k_splat_resolve"][i], P * K * ((C + 1) * 8 + C + 8))
            t_is = kernel_line("k_interp_splat", ks["k_interp_splat"][i], P * K * (2 * (C + 1) * 8 + C))
            t_g = kernel_line("k_interp", ks["k_interp"][i], P * (32 + 2 * C + 2 + K * C))
            say("  kernels of the interpolation by splatting (2 k_splat + k_interp_splat, without the clear of %.0f MB): "
                "%.1f us = %.2f x k_interp" % (2 * P * K * (C + 1) * 8 / 1e6, t_fb + t_is, (t_fb + t_is) / t_g))
    say()
    say("Interpolation error (mean absolute, [0, 1]): frame 2 of the committed triples from frames 1 and 3 at t = 0.5, "
        "5 levels, the device's flows")
    import cases
    for r in ("240", "480"):
        f1, f2, f3 = (cases.load_frame_u8(r, i) for i in (1, 2, 3))
        t1, t3 = torch.from_numpy(f1[None]).to(dev), torch.from_numpy(f3[None]).to(dev)
        truth = f2.astype(np.float64) / 255.0
        err = {}
        for method in ("gather", "splat"):
            ip = interpolate_pairs(t1, t3, 5, 0.5, layout="NHWC", out_dtype=torch.float64, method=method)
            err[method] = float(np.abs(ip.frames[0, 0].cpu().numpy() - truth).mean())
        ones = interpolate_pairs(t1, t3, 5, 0.5, layout="NHWC", out_dtype=torch.float64, method="splat", alpha=0.0)
        blend = float(np.abs(0.5 * (f1.astype(np.float64) + f3.astype(np.float64)) / 255.0 - truth).mean())
        say("  %sx%s: gather %.6f   splat (alpha = 20) %.6f   splat (weights 1) %.6f   plain blend %.6f" % (
            cases.SIZES[r][1], cases.SIZES[r][0], err["gather"], err["splat"],
            float(np.abs(ones.frames[0, 0].cpu().numpy() - truth).mean()), blend))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
