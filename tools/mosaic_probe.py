#!/usr/bin/env python3
"""Cost of the mosaic kernel (tensors.mosaic -> papof_mosaic_tensor: k_mosaic) against the same result composed from what the
library and PyTorch had before it, on one device.  The yardstick is that composition on the same machine, never the kernel
itself.

Three cases:
  (a) fill 1080p   stabilize_video_full's mosaic: 8 stabilized 1920x1080x3 uint8 frames, fill radius 15 (31 sources each),
                   mode "first" with the count; against warp_affine of the 8 frames alone (what stabilize_video pays) and
                   against 31 warp_affine calls + torch.where (the same pixels without the kernel); and the second launch
                   of stabilize_video_full, slot 0 alone on one channel, whose count is `valid`;
  (b) panorama     a 3840x1400 canvas from 32 uint8 1080p sources, "median" and "mean"; against grid_sample of every source
                   into a float32 stack + nanmedian / nanmean (not the same bits: float32, another bilinear rule at the edge);
  (b64) the same   with 64 sources, "median": the kernel's instance for 33 .. 64 samples, one wave per SIMD;
  (c) fill 240     as (a) at 240x135, 32 frames.
In (a) and (c) every neighbour exists, so slot k of all outputs is one slice of the video and the composition reads it in place.
Times are device time between two events around the call (the launch included), median (min, max) of --reps after warm-up;
every case also with tile-level culling switched off (PAPOF_MOSAIC_CULL=0).  Byte floor: every source frame that the outputs
touch read once plus every output (and its count) written once, over 8 TB/s (spec) and 6.3 TB/s (a measured copy).

    python3 tools/mosaic_probe.py --out profiles/mosaic_probe.txt"""
import argparse
import io
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd import tensors  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12


def shaky_motion(T, H, W, seed):
    """pair motions of a slow pan with shake of about 1 % of the frame and 0.01 rad, as a (T - 1, 2, 3) float64 tensor"""
    rng = np.random.default_rng(seed)
    K = []
    for t in range(T):
        th = rng.normal(0, 0.01)
        tx, ty = 0.002 * W * t + rng.normal(0, 0.01 * W), rng.normal(0, 0.01 * H)
        c, s = math.cos(th), math.sin(th)
        cx, cy = (W - 1) / 2, (H - 1) / 2
        K.append(np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1.0]]))
    return torch.from_numpy(np.array([(np.linalg.inv(K[t + 1]) @ K[t])[:2] for t in range(T - 1)]))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        dt.append(a.elapsed_time(b) * 1e3)
    return float(np.median(dt)), min(dt), max(dt)


def no_cull(fn):
    def run():
        os.environ["PAPOF_MOSAIC_CULL"] = "0"
        try:
            fn()
        finally:
            del os.environ["PAPOF_MOSAIC_CULL"]
    return run


def fill_case(T, H, W, outs, radius, dev, seed):
    """(mosaic, warp alone, composition, floor bytes) of stabilize_video_full's last step for the output frames `outs`"""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    A = shaky_motion(T, H, W, seed)
    M = tensors.stabilizing_transforms(A, 15)
    src, mats = tensors.neighbour_transforms(M, A, radius)
    src, mats = src[outs].contiguous(), mats[outs].contiguous().to(dev)
    assert int(src.min()) >= 0  # every neighbour exists: slot k of all outputs is one slice of the video, read in place
    src_host = src.numpy()
    own = frames[outs[0]:outs[-1] + 1]
    Mo = M[outs].to(dev)
    slot = [mats[:, k].contiguous() for k in range(src.shape[1])]

    def composed():
        out, have = tensors.warp_affine(own, Mo, layout="NHWC")
        for k in range(1, src.shape[1]):
            s0 = int(src_host[0, k])
            w, v = tensors.warp_affine(frames[s0:s0 + len(outs)], slot[k], layout="NHWC")
            v = v & ~have
            out = torch.where(v.unsqueeze(-1), w, out)
            have = have | v
        return out

    touched = len(set(int(s) for s in src.reshape(-1).tolist() if s >= 0))
    floor = touched * H * W * 3 + len(outs) * H * W * 4
    one, first = frames[..., :1], mats[:, :1].contiguous()  # stabilize_video_full's second launch: slot 0 alone, for `valid`
    return (lambda: tensors.mosaic(frames, src_host, mats, (H, W), mode="first", layout="NHWC"),
            lambda: tensors.warp_affine(own, Mo, layout="NHWC"), composed, floor,
            lambda: tensors.mosaic(one, src_host[:, :1], first, (H, W), mode="first", layout="NHWC"))


def pano_case(N, H, W, Hc, Wc, dev, seed):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    M = np.empty((1, N, 2, 3))
    for k in range(N):  # a pan across the canvas with a little rotation and zoom
        th, s = 0.002 * (k - N / 2), 1.0 + 0.001 * k
        L = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        c = np.array([(W - 1) / 2 + (Wc - W) * k / (N - 1), (Hc - 1) / 2 + 0.2 * (Hc - H) * math.sin(k)])
        M[0, k, :, :2], M[0, k, :, 2] = L, np.array([(W - 1) / 2, (H - 1) / 2]) - L @ c
    tm = torch.from_numpy(M).to(dev)
    img = frames.permute(0, 3, 1, 2)
    Sx, Sy = 2.0 / (W - 1), 2.0 / (H - 1)
    Nf = np.array([[Sx, 0, -1], [0, Sy, -1], [0, 0, 1.0]])
    Nc = np.linalg.inv(np.array([[2.0 / (Wc - 1), 0, -1], [0, 2.0 / (Hc - 1), -1], [0, 0, 1.0]]))
    theta = torch.from_numpy(np.stack([(Nf @ np.vstack([M[0, k], [0, 0, 1]]) @ Nc)[:2] for k in range(N)])).float().to(dev)

    def stack():
        st = torch.empty((N, 3, Hc, Wc), dtype=torch.float32, device=dev)
        for k in range(N):
            grid = torch.nn.functional.affine_grid(theta[k:k + 1], (1, 3, Hc, Wc), align_corners=True)
            inside = (grid.abs() <= 1).all(-1)
            w = torch.nn.functional.grid_sample(img[k:k + 1].float() / 255.0, grid, mode="bilinear", padding_mode="zeros",
                                                align_corners=True)
            st[k] = torch.where(inside.unsqueeze(1), w, torch.full_like(w, math.nan))[0]
        return st

    def to_u8(x):
        return torch.clamp(torch.round(255 * torch.nan_to_num(x)), 0, 255).to(torch.uint8)

    floor = N * H * W * 3 + Hc * Wc * 4
    return {mode: (lambda mode=mode: tensors.mosaic(frames, None, tm, (Hc, Wc), mode=mode, layout="NHWC"),
                   (lambda: to_u8(stack().nanmedian(0).values)) if mode == "median" else (lambda: to_u8(stack().nanmean(0))))
            for mode in ("median", "mean")}, floor


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

    def report(what, floor, mine, others):
        say()
        say(what)
        say("  byte floor: %.1f MB: %.1f us at 8 TB/s, %.1f us at 6.3 TB/s" % (floor / 1e6, 1e6 * floor / SPEC_BW, 1e6 * floor / COPY_BW))
        med, lo, hi = timed(mine, args.reps)
        say("  mosaic                         %10.1f us  (%.1f, %.1f)   %.1f x the 6.3 TB/s floor" % (
            med, lo, hi, med / (1e6 * floor / COPY_BW)))
        m2, lo2, hi2 = timed(no_cull(mine), args.reps)
        say("  mosaic, culling off            %10.1f us  (%.1f, %.1f)   %.2f x with culling" % (m2, lo2, hi2, m2 / med))
        for name, fn in others:
            mo, loo, hio = timed(fn, args.reps)
            say("  %-30s %10.1f us  (%.1f, %.1f)   %.2f x the mosaic" % (name, mo, loo, hio, mo / med))

    say("The mosaic kernel on one %s device against the composition it replaces.  Device time between events around the call,"
        " median (min, max) of %d after warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    mine, warp, composed, floor, own_cover = fill_case(48, 1080, 1920, list(range(20, 28)), 15, dev, 1)
    report("(a) border fill: 8 frames of 1920x1080x3 uint8, fill radius 15 (31 sources), mode first + count", floor, mine,
           [("warp_affine alone (no fill)", warp), ("31 warp_affine + torch.where", composed),
            ("the launch that makes `valid`", own_cover)])
    del mine, warp, composed, own_cover
    torch.cuda.empty_cache()
    both, floor = pano_case(32, 1080, 1920, 1400, 3840, dev, 2)
    for mode in ("median", "mean"):
        report("(b) panorama: 3840x1400 canvas, 32 uint8 1080p sources, mode %s" % mode, floor, both[mode][0],
               [("grid_sample stack + nan%s" % mode, both[mode][1])])
    del both
    torch.cuda.empty_cache()
    both, floor = pano_case(64, 1080, 1920, 1400, 3840, dev, 4)  # the instance that holds 64 samples: one wave per SIMD
    report("(b64) panorama: 3840x1400 canvas, 64 uint8 1080p sources, mode median", floor, both["median"][0],
           [("grid_sample stack + nanmedian", both["median"][1])])
    del both
    torch.cuda.empty_cache()
    mine, warp, composed, floor, own_cover = fill_case(64, 135, 240, list(range(16, 48)), 15, dev, 3)
    report("(c) border fill: 32 frames of 240x135x3 uint8, fill radius 15 (31 sources), mode first + count", floor, mine,
           [("warp_affine alone (no fill)", warp), ("31 warp_affine + torch.where", composed),
            ("the launch that makes `valid`", own_cover)])
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
