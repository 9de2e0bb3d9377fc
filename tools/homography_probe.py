#!/usr/bin/env python3
"""Cost of the homography model (tensors.global_homography, warp_homography, mosaic_homography, mosaic_overlap_homography)
on one device, each against its affine twin on the same inputs in the same run -- never against itself.

Cases:
  (a) fit       one 1080p pair and 100 pairs of 240x135, float64 flows, 5 iterations: global_homography against
                global_motion(model="affine"), and against the bytes of the flow read once per iteration over 8 TB/s (spec)
                and 6.3 TB/s (a measured copy);
  (b) warp      8 frames of 1080p x 3 uint8: warp_homography against warp_affine;
  (c) mosaic    tools/mosaic_probe.py's panorama: a 3840x1400 canvas from 32 uint8 1080p sources, "mean", "median" and
                "feather": the projective call on the affine matrices with a last row (0, 0, 1) against the affine call (the
                two divisions and the looser culling); the same matrices with a mild perspective, culling on and off; and a
                torch composition (grid_sample over a projective grid into a float32 stack, nanmean / nanmedian);
  (d) overlap   mosaic_overlap_homography against mosaic_overlap on that panorama at steps 1, 2 and 4.
Times are device time between two events around the call (the launches included), median (min, max) of --reps after warm-up.

    python3 tools/homography_probe.py --out profiles/homography_probe.txt"""
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
from mosaic_probe import no_cull, timed  # noqa: E402
from papteam_opticalflow_amd import tensors  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12


def flows(B, H, W, dev, seed):
    """B float64 flows of random mild homographies plus noise and 20 % gross outliers"""
    rng = np.random.default_rng(seed)
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.empty((B, 2, H, W))
    for i in range(B):
        m = np.eye(3)
        m[:2, :2] += rng.normal(0, 0.01, (2, 2))
        m[:2, 2] = rng.normal(0, 2, 2)
        m[2, :2] = rng.normal(0, 2e-4 * 240 / W, 2)
        d = m[2, 0] * x + m[2, 1] * r + 1.0
        f[i, 0] = (m[0, 0] * x + m[0, 1] * r + m[0, 2]) / d - x
        f[i, 1] = (m[1, 0] * x + m[1, 1] * r + m[1, 2]) / d - r
    f += rng.normal(0, 0.2, f.shape)
    bad = rng.random((B, H, W)) < 0.2
    f[:, 0][bad] += rng.uniform(-15, 15, int(bad.sum()))
    return torch.from_numpy(f).to(dev)


def embedded(M, perspective=0.0):
    """(1, N, 2, 3) -> (1, N, 3, 3) with last rows (p_k, -p_k / 2, 1), p_k alternating in sign"""
    N = M.shape[1]
    M3 = np.zeros((1, N, 3, 3))
    M3[:, :, :2] = M
    M3[:, :, 2, 2] = 1.0
    for k in range(N):
        M3[0, k, 2, :2] = (perspective * (-1) ** k, -0.5 * perspective * (-1) ** k)
    return M3


def torch_stack(frames, M3, Hc, Wc):
    """the sources resampled through their 3 x 3 matrices into a float32 stack (N, 3, Hc, Wc), NaN where not live"""
    N, H, W, _ = frames.shape
    dev = frames.device
    img = frames.permute(0, 3, 1, 2)
    r, x = torch.meshgrid(torch.arange(Hc, device=dev, dtype=torch.float32), torch.arange(Wc, device=dev, dtype=torch.float32),
                          indexing="ij")
    st = torch.empty((N, 3, Hc, Wc), dtype=torch.float32, device=dev)
    for k in range(N):
        m = M3[k]
        D = m[2, 0] * x + m[2, 1] * r + m[2, 2]
        X, Y = (m[0, 0] * x + m[0, 1] * r + m[0, 2]) / D, (m[1, 0] * x + m[1, 1] * r + m[1, 2]) / D
        grid = torch.stack([2 * X / (W - 1) - 1, 2 * Y / (H - 1) - 1], -1)[None]
        inside = (D > 0) & (grid.abs() <= 1).all(-1)[0]
        w = torch.nn.functional.grid_sample(img[k:k + 1].float() / 255.0, grid, mode="bilinear", padding_mode="zeros",
                                            align_corners=True)
        st[k] = torch.where(inside[None], w[0], torch.full_like(w[0], math.nan))
    return st


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

    say("The homography calls on one %s device.  Device time between events around the call, median (min, max) of %d after"
        " warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    say()
    say("(a) fit: float64 flows, 5 iterations")
    for B, H, W, seed in ((1, 1080, 1920, 1), (100, 135, 240, 2)):
        f = flows(B, H, W, dev, seed)
        nbytes = 5 * f.numel() * 8
        say(" %d pair(s) of %dx%d; the flow read once per iteration: %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (
            B, W, H, nbytes / 1e6, 1e6 * nbytes / SPEC_BW, 1e6 * nbytes / COPY_BW))
        base = line("global_motion(model=\"affine\")", lambda: tensors.global_motion(f, model="affine"))
        med = line("global_homography", lambda: tensors.global_homography(f), base, "the affine fit")
        one = line("global_homography, 1 iteration", lambda: tensors.global_homography(f, iters=1))
        say("    %.2f x the 6.3 TB/s floor; per iteration %.1f us" % (med / (1e6 * nbytes / COPY_BW), (med - one) / 4))
        del f
    say()
    say("(b) warp: 8 frames of 1920x1080 x 3 uint8")
    g = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 256, (8, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    th = 0.01
    M2 = np.tile(np.array([[math.cos(th), -math.sin(th), 12.0], [math.sin(th), math.cos(th), -7.0]]), (8, 1, 1))
    M3 = embedded(M2[None], 1e-5)[0]
    t2, t3 = torch.from_numpy(M2).to(dev), torch.from_numpy(M3).to(dev)
    base = line("warp_affine", lambda: tensors.warp_affine(fr, t2, layout="NHWC"))
    line("warp_homography", lambda: tensors.warp_homography(fr, t3, layout="NHWC"), base, "warp_affine")
    del fr
    torch.cuda.empty_cache()
    N, H, W, Hc, Wc = 32, 1080, 1920, 1400, 3840
    frames, tm, M = pano(N, H, W, Hc, Wc, dev, 2)
    te = torch.from_numpy(embedded(M)).to(dev)
    tp = torch.from_numpy(embedded(M, 1e-5)).to(dev)
    say()
    say("(c) mosaic: %dx%d canvas, %d uint8 %dx%d sources; 'embedded': last rows (0, 0, 1); 'perspective': (+-1e-5, -+5e-6, 1)"
        % (Wc, Hc, N, W, H))
    for mode in ("mean", "median", "feather"):
        base = line("mosaic %s" % mode, lambda: tensors.mosaic(frames, None, tm, (Hc, Wc), mode=mode, layout="NHWC"))
        line("mosaic_homography %s, embedded" % mode,
             lambda: tensors.mosaic_homography(frames, None, te, (Hc, Wc), mode=mode, layout="NHWC"), base, "the affine call")
        run = lambda: tensors.mosaic_homography(frames, None, tp, (Hc, Wc), mode=mode, layout="NHWC")  # noqa: E731
        on = line("mosaic_homography %s, perspective" % mode, run, base, "the affine call")
        line("  the same, PAPOF_MOSAIC_CULL=0", no_cull(run), on, "with culling")
        if mode != "feather":
            red = (lambda s: torch.nanmean(s, 0)) if mode == "mean" else (lambda s: torch.nanmedian(s, 0).values)
            line("torch: grid_sample stack + nan%s" % mode, lambda: red(torch_stack(frames, tp[0].float(), Hc, Wc)), on,
                 "the kernel")
            torch.cuda.empty_cache()
    say()
    say("(d) overlap: the same panorama")
    for step in (1, 2, 4):
        base = line("mosaic_overlap, step %d" % step,
                    lambda: tensors.mosaic_overlap(frames, None, tm, (Hc, Wc), step=step, layout="NHWC"))
        line("mosaic_overlap_homography, embedded",
             lambda: tensors.mosaic_overlap_homography(frames, None, te, (Hc, Wc), step=step, layout="NHWC"), base, "the affine call")
        line("mosaic_overlap_homography, perspective",
             lambda: tensors.mosaic_overlap_homography(frames, None, tp, (Hc, Wc), step=step, layout="NHWC"), base, "the affine call")
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
