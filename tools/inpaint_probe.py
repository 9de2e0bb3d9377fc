#!/usr/bin/env python3
"""Cost of flow-guided video completion's two device calls (tensors.fill_holes -> papof_fill_holes_tensor, the k_fill_*
chain; tensors.propagate -> papof_propagate_tensor, one k_propagate launch) against their compulsory byte floors and
against the same rules written with PyTorch (avg_pool2d / interpolate pull-push, grid_sample chains) in float64.

Cases, uint8 NHWC frames (3 channels), float64 flows, the defaults (relax 0, no check, R = T - 1), uint8 out:
  1080p T=16 5 %    sixteen 1920x1080 frames, a moving rectangle hole of about 5 % of the frame;
  1080p T=16 25 %   the same video, a hole of about 25 %;
  240 T=101 5 %     101 frames of 240x135 made from the committed frames.
Flows are smooth random fields (bw = -fw + noise) of a few pixels.  Each case also times fill_holes with relax = 8.

Compulsory bytes: fill -- x and the mask read once, out written once (n H W (2 C + 1)); propagate -- the frames, the masks
and both flows read once, out and status written once (T H W (2 C + 2) + 2 (T - 1) H W 16).  Over 8 TB/s (spec) and 6.3 TB/s
(a measured copy).  Wall times are call + synchronise, median of --reps after warm-up.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o inpaint -- python3 tools/inpaint_probe.py --kernel-only
    python3 tools/inpaint_probe.py --kernel-stats DIR --out profiles/inpaint_probe.txt
(the dispatches are assigned to the cases in the order the --kernel-only run makes them: per case, --reps times fill_holes
with relax 0, then --reps times propagate)."""
import argparse
import collections
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
import torch.nn.functional as Fn  # noqa: E402

from papteam_opticalflow_amd.tensors import fill_holes, propagate  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = Fn.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def moving_masks(T, H, W, share):
    """a rectangle of about `share` of the frame moving right by W / 100 per frame"""
    m = torch.zeros(T, H, W, dtype=torch.bool)
    h, w = int(H * share ** 0.5), int(W * share ** 0.5)
    for t in range(T):
        x0 = (W // 8 + t * (W // 100)) % (W - w)
        m[t, H // 4:H // 4 + h, x0:x0 + w] = True
    return m


def make_cases(dev):
    g = torch.Generator().manual_seed(7)
    v = torch.randint(0, 256, (16, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    fw, bw = (f.to(dev) for f in flows(15, 1080, 1920, 8))
    out = [("1920x1080, T = 16, hole %d %%" % int(100 * s), v, moving_masks(16, 1080, 1920, s).to(dev), fw, bw)
           for s in (0.05, 0.25)]
    import cases
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    fr = np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(101)])
    fw, bw = (f.to(dev) for f in flows(100, 135, 240, 9))
    out.append(("240x135, T = 101, hole 5 %", torch.from_numpy(fr).to(dev), moving_masks(101, 135, 240, 0.05).to(dev), fw,
                bw))
    return out


def levels(H, W):
    n = 1
    while H > 1 or W > 1:
        H, W, n = (H + 1) // 2, (W + 1) // 2, n + 1
    return n


def torch_fill(v, m):
    """pull-push with avg_pool2d and interpolate in float64, uint8 NHWC in and out (relax 0)"""
    x = v.permute(0, 3, 1, 2).double() / 255.0
    k = (~m).unsqueeze(1).double()
    pyr = [(x * k, k)]
    while pyr[-1][0].shape[-2:] != (1, 1):
        s, n = pyr[-1]
        s2 = Fn.avg_pool2d(s, 2, ceil_mode=True, divisor_override=1)
        n2 = Fn.avg_pool2d(n, 2, ceil_mode=True, divisor_override=1)
        pyr.append((torch.where(n2 > 0, s2 / n2.clamp(min=1), 0.0), (n2 > 0).double()))
    val = pyr[-1][0]
    for l in range(len(pyr) - 2, -1, -1):
        s, n = pyr[l]
        up = Fn.interpolate(val, size=s.shape[-2:], mode="bilinear", align_corners=False)
        val = torch.where(n > 0, s, up)
    return torch.clamp(torch.round(255.0 * val), 0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def torch_propagate(v, m, fw, bw, R):
    """the chains of papof_propagate_tensor with grid_sample in float64 (no check), uint8 NHWC in and out"""
    T, H, W, C = v.shape
    I = v.permute(0, 3, 1, 2).double() / 255.0
    M = m.unsqueeze(1).double()
    y, x = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float64),
                          torch.arange(W, device=v.device, dtype=torch.float64), indexing="ij")

    def sample(img, X, Y):
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (H - 1)) - 1], -1)
        return Fn.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    num, den = torch.zeros_like(I), torch.zeros(T, 1, H, W, dtype=torch.float64, device=v.device)
    for d in (1, -1):
        X, Y = x.expand(T, H, W).clone(), y.expand(T, H, W).clone()
        alive = m.clone()
        for j in range(1, R + 1):
            if T - j < 1:
                break
            ts = torch.arange(0, T - j, device=v.device) if d > 0 else torch.arange(j, T, device=v.device)
            pairs, src = (ts + j - 1, ts + j) if d > 0 else (ts - j, ts - j)
            uv = sample((fw if d > 0 else bw)[pairs], X[ts], Y[ts])
            nX, nY = X[ts] + uv[:, 0], Y[ts] + uv[:, 1]
            al = alive[ts] & (nX >= 0) & (nX <= W - 1) & (nY >= 0) & (nY <= H - 1)
            clear = al & (sample(M[src], nX, nY)[:, 0] == 0)
            g = sample(I[src], nX, nY)
            w = torch.where(clear, 1.0 / j, 0.0).unsqueeze(1)
            num[ts] += w * g
            den[ts] += w
            X[ts], Y[ts], alive[ts] = nX, nY, al & ~clear
    out = torch.where(den > 0, num / den.clamp(min=1e-300), I)
    return torch.clamp(torch.round(255.0 * out), 0, 255).to(torch.uint8).permute(0, 2, 3, 1)


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
    """per case: {kernel name: [durations (us) per rep]} from rocprofv3's kernel trace in dispatch order; counts[i] =
    (dispatches of one fill, of one propagate) of case i"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    rows = []
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("kernel_name", row.get("name", ""))
        if "k_fill_" in name or "k_propagate" in name:
            short = next(k for k in ("k_fill_base", "k_fill_pull", "k_fill_push", "k_fill_relax", "k_fill_store",
                                     "k_propagate") if k in name)
            rows.append((int(row["start_timestamp"]), int(row["end_timestamp"]), short))
    rows.sort()
    need = sum(reps * (f + p) for f, p in counts)
    if len(rows) != need:
        raise SystemExit("expected %d dispatches, found %d" % (need, len(rows)))
    out, i = [], 0
    for f, p in counts:
        per = collections.defaultdict(float)
        fill_span = []
        for _ in range(reps):
            chunk = rows[i:i + f]
            fill_span.append((chunk[-1][1] - chunk[0][0]) / 1e3)
            for s, e, k in chunk:
                per[k] += (e - s) / 1e3 / reps
            i += f
        for _ in range(reps):
            for s, e, k in rows[i:i + p]:
                per[k] += (e - s) / 1e3 / reps
            i += p
        out.append((dict(per), float(np.median(fill_span))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run fill_holes and propagate only (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 output directory of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = make_cases(dev)
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, v, m, fw, bw in cases:
            for _ in range(args.reps):
                fill_holes(v, m, layout="NHWC")
            for _ in range(args.reps):
                propagate(v, m, fw, bw, layout="NHWC")
            torch.cuda.synchronize()
        return
    counts = [(2 + 2 * (levels(*v.shape[1:3]) - 1), 1) for _, v, _, _, _ in cases]
    ks = kernel_times(args.kernel_stats, counts, args.reps) if args.kernel_stats else None
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Video completion on one %s device: fill_holes (the k_fill_* chain) and propagate (one k_propagate launch) against "
        "their compulsory byte floors and against PyTorch compositions in float64.  uint8 NHWC frames (C = 3), float64 "
        "flows, relax 0, no check, R = T - 1, uint8 out.  Wall: call + synchronise, median (min, max) of %d after warm-up." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for i, (what, v, m, fw, bw) in enumerate(cases):
        T, H, W, C = v.shape
        L = levels(H, W) - 1
        fill_bytes = T * H * W * (2 * C + 1)
        prop_bytes = T * H * W * (2 * C + 2) + 2 * (T - 1) * H * W * 16
        say()
        say("%s: %d pixels, %.1f %% of them holes; %d levels below the frame" % (what, T * H * W,
                                                                              100 * float(m.double().mean()), L))
        for name, nb in (("fill", fill_bytes), ("propagate", prop_bytes)):
            say("  %-9s compulsory floor: %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (
                name, nb / 1e6, 1e6 * nb / SPEC_BW, 1e6 * nb / COPY_BW))
        res = {}
        for relax in (0, 8):
            med, lo, hi = wall(lambda: res.__setitem__("f", fill_holes(v, m, layout="NHWC", relax=relax)), args.reps)
            say("  fill_holes relax %d   wall %10.1f us  (%.1f, %.1f)   %d launches" % (relax, 1e6 * med, 1e6 * lo, 1e6 * hi,
                                                                                   2 + L * (2 + relax)))
            if relax == 0:
                med_f = med
        med_t, lo_t, hi_t = wall(lambda: res.__setitem__("tf", torch_fill(v, m)), max(3, args.reps // 2))
        say("  torch pull-push       wall %10.1f us  (%.1f, %.1f)   (%.1f x fill_holes relax 0)" % (
            1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, med_t / med_f))
        med_p, lo_p, hi_p = wall(lambda: res.__setitem__("p", propagate(v, m, fw, bw, layout="NHWC")), args.reps)
        st = res["p"].status
        say("  propagate             wall %10.1f us  (%.1f, %.1f)   %.1f %% of the holes filled" % (
            1e6 * med_p, 1e6 * lo_p, 1e6 * hi_p, 100 * float((st == 1).sum()) / max(1, int((st > 0).sum()))))
        med_g, lo_g, hi_g = wall(lambda: res.__setitem__("tp", torch_propagate(v, m, fw, bw, T - 1)), max(3, args.reps // 2))
        say("  grid_sample chains    wall %10.1f us  (%.1f, %.1f)   (%.1f x propagate)" % (
            1e6 * med_g, 1e6 * lo_g, 1e6 * hi_g, med_g / med_p))
        if ks:
            per, span = ks[i]
            fill_k = sum(t for k, t in per.items() if k.startswith("k_fill"))
            say("  rocprofv3 --kernel-trace, average per call (us): " + ", ".join(
                "%s %.1f" % (k, t) for k, t in sorted(per.items())))
            say("    fill: %.1f us of kernels in a %.1f us span (first start to last end, median), %.2f x its 8 TB/s "
                "floor" % (fill_k, span, fill_k / (1e6 * fill_bytes / SPEC_BW)))
            say("    propagate: %.1f us, %.2f x its 8 TB/s floor, %.2f x the 6.3 TB/s one" % (
                per["k_propagate"], per["k_propagate"] / (1e6 * prop_bytes / SPEC_BW),
                per["k_propagate"] / (1e6 * prop_bytes / COPY_BW)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
