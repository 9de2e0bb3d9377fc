#!/usr/bin/env python3
"""Cost of the ray rule (tensors.mosaic_rays, mosaic_overlap_rays) on one device, against the projective calls on identical
inputs in the same run -- never against itself.

Cases:
  (a) plane     tools/homography_probe.py's panorama: a 3840x1400 canvas from 32 uint8 1080p sources under mildly projective
                matrices, "mean", "median" and "feather", culling on and off: mosaic_rays on the plane's tables cols = (x, 1),
                rows = (y, 1) -- the same bytes -- against mosaic_homography: three more multiplies per source and pixel, two
                table loads per pixel, and the interval culling in place of the corner test;
  (b) cylinder  a canvas of the same size around a camera of focal length 1100 px (200 degrees by 73): 32 uint8 1080p
                sources that yaw over 118 degrees, the same modes, culling on and off;
  (c) overlap   mosaic_overlap_rays against mosaic_overlap_homography on (a) at steps 1, 2 and 4, and on (b).
Times are device time between two events around the call (the launches included), median (min, max) of --reps after warm-up.

    python3 tools/wide_probe.py --out profiles/wide_probe.txt"""
import argparse
import io
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from blend_probe import pano  # noqa: E402
from homography_probe import embedded  # noqa: E402
from mosaic_probe import no_cull, timed  # noqa: E402
from papteam_opticalflow_amd import tensors  # noqa: E402


def cylinder(N, H, W, Hc, Wc, focal, dev):
    """(matrices (1, N, 3, 3), cols, rows) of N cameras K R_k that yaw evenly over the part of an Hc x Wc cylinder canvas
    (one pixel is 1 / focal) that their field of view leaves, with a little pitch and roll each"""
    K = np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    half = (Wc - 1) / 2.0 / focal - math.atan((W - 1) / 2.0 / focal)
    M = np.empty((1, N, 3, 3))
    for k in range(N):
        a, p, r = half * (2.0 * k / (N - 1) - 1.0), 0.05 * math.sin(k), 0.002 * (k - N / 2)
        Ry = np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
        Rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(p), -math.sin(p)], [0.0, math.sin(p), math.cos(p)]])
        Rz = np.array([[math.cos(r), -math.sin(r), 0.0], [math.sin(r), math.cos(r), 0.0], [0.0, 0.0, 1.0]])
        M[0, k] = K @ Rz @ Rx @ Ry
    th = (np.arange(Wc) - (Wc - 1) / 2.0) / focal
    cols = np.stack([np.sin(th), np.cos(th)], 1)
    rows = np.stack([(np.arange(Hc) - (Hc - 1) / 2.0) / focal, np.ones(Hc)], 1)
    return tuple(torch.from_numpy(a).to(dev) for a in (M, cols, rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    def line(name, fn, base=None, what=""):
        med, lo, hi = timed(fn, args.reps)
        say("  %-44s %10.1f us  (%.1f, %.1f)%s" % (name, med, lo, hi, "" if base is None else "   %.2f x %s" % (med / base, what)))
        return med

    say("The ray calls on one %s device.  Device time between events around the call, median (min, max) of %d after warm-up."
        % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    N, H, W, Hc, Wc = 32, 1080, 1920, 1400, 3840
    frames, _, M = pano(N, H, W, Hc, Wc, dev, 2)
    tp = torch.from_numpy(embedded(M, 1e-5)).to(dev)
    x, y = torch.arange(Wc, dtype=torch.float64, device=dev), torch.arange(Hc, dtype=torch.float64, device=dev)
    pc, pr = torch.stack([x, torch.ones_like(x)], 1), torch.stack([y, torch.ones_like(y)], 1)
    a = tensors.mosaic_homography(frames, None, tp, (Hc, Wc), mode="feather", layout="NHWC")
    b = tensors.mosaic_rays(frames, None, tp, pc, pr, mode="feather", layout="NHWC")
    assert torch.equal(a.out, b.out) and torch.equal(a.count, b.count)
    say()
    say("(a) plane tables: %dx%d canvas, %d uint8 %dx%d sources, last rows (+-1e-5, -+5e-6, 1); the same bytes (checked)"
        % (Wc, Hc, N, W, H))
    ratios = []
    for mode in ("mean", "median", "feather"):
        hom = lambda: tensors.mosaic_homography(frames, None, tp, (Hc, Wc), mode=mode, layout="NHWC")  # noqa: E731
        ray = lambda: tensors.mosaic_rays(frames, None, tp, pc, pr, mode=mode, layout="NHWC")  # noqa: E731
        base = line("mosaic_homography %s" % mode, hom)
        on = line("mosaic_rays %s, plane tables" % mode, ray, base, "mosaic_homography")
        ratios.append(on / base)
        base0 = line("  mosaic_homography, PAPOF_MOSAIC_CULL=0", no_cull(hom), base, "with culling")
        line("  mosaic_rays, PAPOF_MOSAIC_CULL=0", no_cull(ray), base0, "mosaic_homography without culling")
    say("  plane-table ratio, mean / median / feather: %s" % " / ".join("%.2f" % r for r in ratios))
    focal = 1100.0
    cm, cc, cr = cylinder(N, H, W, Hc, Wc, focal, dev)
    cnt = tensors.mosaic_rays(frames, None, cm, cc, cr, mode="first", layout="NHWC").count
    say()
    say("(b) cylinder: the same canvas at focal length %.0f px (%.0f x %.0f degrees), %d sources yawing over %.0f degrees; "
        "%.1f live sources per pixel on average, %.1f %% of the canvas covered"
        % (focal, math.degrees((Wc - 1) / focal), math.degrees(2 * math.atan((Hc - 1) / 2 / focal)), N,
           math.degrees((Wc - 1) / focal - 2 * math.atan((W - 1) / 2 / focal)), float(cnt.float().mean()),
           100.0 * float((cnt > 0).float().mean())))
    for mode in ("mean", "median", "feather"):
        ray = lambda: tensors.mosaic_rays(frames, None, cm, cc, cr, mode=mode, layout="NHWC")  # noqa: E731
        on = line("mosaic_rays %s, cylinder" % mode, ray)
        line("  the same, PAPOF_MOSAIC_CULL=0", no_cull(ray), on, "with culling")
    say()
    say("(c) overlap")
    for step in (1, 2, 4):
        base = line("mosaic_overlap_homography, step %d" % step,
                    lambda: tensors.mosaic_overlap_homography(frames, None, tp, (Hc, Wc), step=step, layout="NHWC"))
        line("mosaic_overlap_rays, plane tables",
             lambda: tensors.mosaic_overlap_rays(frames, None, tp, pc, pr, step=step, layout="NHWC"), base, "mosaic_overlap_homography")
        line("mosaic_overlap_rays, cylinder",
             lambda: tensors.mosaic_overlap_rays(frames, None, cm, cc, cr, step=step, layout="NHWC"))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
