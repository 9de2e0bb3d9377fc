#!/usr/bin/env python3
"""Cost of the seamless mosaics (tensors.mosaic with gains / mode "feather" -> papof_mosaic_blend_tensor; tensors.mosaic_overlap
-> papof_mosaic_overlap_tensor) on one device.  The yardsticks are the plain mosaic on the same inputs (papof_mosaic_tensor:
the instances of the commit before, unchanged) and, for the statistics, their composition in PyTorch -- never the kernels
themselves.

Cases:
  (a) blend 1080p     tools/mosaic_probe.py's panorama (b): a 3840x1400 canvas from 32 uint8 1080p sources; "feather" against
                      "mean", and "first", "mean" and "median" with gains against without;
  (b) overlap 1080p   mosaic_overlap on that panorama at step 1, 2 and 4, against the same statistics in torch (grid_sample of
                      every source at the sampled pixels alone into a stack, a live mask, two einsums -- float32 samples, float64
                      sums: not the same integers); and the bytes of its atomic adds (16 B per (tile, i, j) with a pixel in
                      common, counted from the torch live mask) over its time, against the 1.3 TB/s the chip adds at;
  (c) 240x135         both on a 480x175 canvas from 32 uint8 240x135 sources.
Times are device time between two events around the call (the launch included), median (min, max) of --reps after warm-up.

    python3 tools/blend_probe.py --out profiles/blend_probe.txt"""
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

from mosaic_probe import timed  # noqa: E402
from papteam_opticalflow_amd import tensors  # noqa: E402

ATOMIC_BW = 1.3e12  # bytes of atomic adds per second, chip-wide


def pano(N, H, W, Hc, Wc, dev, seed):
    """mosaic_probe.pano_case's inputs: frames (N, H, W, 3) uint8, matrices (1, N, 2, 3) on the device and on the host"""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    M = np.empty((1, N, 2, 3))
    for k in range(N):
        th, s = 0.002 * (k - N / 2), 1.0 + 0.001 * k
        L = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        c = np.array([(W - 1) / 2 + (Wc - W) * k / (N - 1), (Hc - 1) / 2 + 0.2 * (Hc - H) * math.sin(k)])
        M[0, k, :, :2], M[0, k, :, 2] = L, np.array([(W - 1) / 2, (H - 1) / 2]) - L @ c
    return frames, torch.from_numpy(M).to(dev), M


def sampled_theta(M, H, W, Hc, Wc, step, dev):
    """affine_grid's thetas for the SAMPLED canvas alone -- pixel (sx, sr) of a ceil(Hc / step) x ceil(Wc / step) grid is
    canvas pixel (sx step, sr step) --, so that the composition pays for no pixel it does not use"""
    Hs, Ws = (Hc - 1) // step + 1, (Wc - 1) // step + 1
    Nf = np.array([[2.0 / (W - 1), 0, -1], [0, 2.0 / (H - 1), -1], [0, 0, 1.0]])
    Ns = np.linalg.inv(np.array([[2.0 / (Ws - 1), 0, -1], [0, 2.0 / (Hs - 1), -1], [0, 0, 1.0]]))
    S = np.diag([float(step), float(step), 1.0])
    th = np.stack([(Nf @ np.vstack([M[0, k], [0, 0, 1]]) @ S @ Ns)[:2] for k in range(M.shape[1])])
    return torch.from_numpy(th).float().to(dev), (Hs, Ws)


def torch_overlap(frames, theta, size):
    """(sums, counts, live (N, Hs, Ws)) of the statistics composed in torch at the sampled pixels"""
    N = frames.shape[0]
    Hs, Ws = size
    img = frames.permute(0, 3, 1, 2)
    lum, live = [], []
    for k in range(N):
        grid = torch.nn.functional.affine_grid(theta[k:k + 1], (1, 3, Hs, Ws), align_corners=True)
        inside = (grid.abs() <= 1).all(-1)[0]
        w = torch.nn.functional.grid_sample(img[k:k + 1].float() / 255.0, grid, mode="bilinear", padding_mode="zeros",
                                            align_corners=True)
        lum.append(w[0].mean(0))
        live.append(inside)
    live = torch.stack(live)
    L = live.reshape(N, -1).double()
    Q = torch.round(torch.stack(lum).reshape(N, -1).clamp(0, 1).double() * tensors.OVERLAP_ONE)
    return torch.einsum("ip,jp->ij", L * Q, L), torch.einsum("ip,jp->ij", L, L), live


def atomic_bytes(live):
    """16 B for every (64 x 2 tile of sampled pixels, i, j) with a pixel in common"""
    N, Hs, Ws = live.shape
    pad = torch.zeros((N, (Hs + 1) // 2 * 2, (Ws + 63) // 64 * 64), dtype=torch.float32, device=live.device)
    pad[:, :Hs, :Ws] = live
    t = pad.reshape(N, pad.shape[1] // 2, 2, pad.shape[2] // 64, 64).permute(1, 3, 0, 2, 4).reshape(-1, N, 128)
    total = 0
    for a in range(0, t.shape[0], 4096):
        total += int((torch.einsum("tip,tjp->tij", t[a:a + 4096], t[a:a + 4096]) > 0).sum())
    return 16 * total


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
        say("  %-34s %10.1f us  (%.1f, %.1f)%s" % (name, med, lo, hi, "" if base is None else "   %.2f x %s" % (med / base, what)))
        return med

    say("The blend and overlap kernels on one %s device.  Device time between events around the call, median (min, max) of %d"
        " after warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for tag, (N, H, W, Hc, Wc, seed) in (("1080p", (32, 1080, 1920, 1400, 3840, 2)), ("240x135", (32, 135, 240, 175, 480, 5))):
        frames, tm, M = pano(N, H, W, Hc, Wc, dev, seed)
        gains = torch.from_numpy(np.exp(np.random.default_rng(3).uniform(math.log(0.75), 0.0, (1, N)))).to(dev)

        def run(mode, g=None):
            return lambda: tensors.mosaic(frames, None, tm, (Hc, Wc), mode=mode, layout="NHWC", gains=g)

        say()
        say("(%s) blend %s: %dx%d canvas, %d uint8 %dx%d sources" % ("a" if tag == "1080p" else "c", tag, Wc, Hc, N, W, H))
        base = {}
        for mode in ("mean", "first", "median"):
            base[mode] = line("%s (papof_mosaic_tensor)" % mode, run(mode))
            line("%s with gains" % mode, run(mode, gains), base[mode], "without")
        line("feather", run("feather"), base["mean"], "mean")
        line("feather with gains", run("feather", gains), base["mean"], "mean")

        say()
        say("(%s) overlap %s: the same panorama" % ("b" if tag == "1080p" else "c", tag))
        for step in (1, 2, 4):
            theta, size = sampled_theta(M, H, W, Hc, Wc, step, dev)
            med = line("mosaic_overlap, step %d" % step,
                       lambda: tensors.mosaic_overlap(frames, None, tm, (Hc, Wc), step=step, layout="NHWC"))
            line("torch: grid_sample + 2 einsums", lambda: torch_overlap(frames, theta, size), med, "the kernel")
            ts, tc, live = torch_overlap(frames, theta, size)
            ov = tensors.mosaic_overlap(frames, None, tm, (Hc, Wc), step=step, layout="NHWC")
            cnt_off = float((ov.counts[0].double() - tc).abs().max() / tc.max())
            mean_off = float(((ov.sums[0].double() / ov.counts[0].clamp(min=1)) - ts / tc.clamp(min=1)).abs().max() / tensors.OVERLAP_ONE)
            b = atomic_bytes(live)
            say("    against torch: counts differ by at most %.1e of the largest, mean luminances by %.1e;" % (cnt_off, mean_off))
            say("    atomic adds: %.2f MB -> %.1f GB/s, %.4f of the chip's %.1f TB/s" % (
                b / 1e6, b / med / 1e3, b / (med * 1e-6) / ATOMIC_BW, ATOMIC_BW / 1e12))
            del ts, tc, live, ov
        del frames, tm, theta, M
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
