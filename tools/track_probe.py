#!/usr/bin/env python3
"""Cost of point tracking (tensors.track_points -> papof_track_tensor, one k_track launch) against its byte floor and
against the same steps written with PyTorch's grid_sample in float64, on one device.

Two cases:
  dense   every pixel of frame 0 of a 1920x1080 clip of 16 frames (smooth random float64 flows, bw = -fw + noise, so
          that most points stay visible and keep gathering: a lost point only stores);
  sparse  1024 queries on the 240x135 clip of 101 frames made from the committed frames, flows from flow_video_fb
          (float64, consistency=None); every query starts at t0 = 0, so each one is followed through all 100 steps.

Byte floor: every flow plane read once (both directions, float64), tracks (16 B) and visible (1 B) written once per frame
and point, over 8 TB/s (spec) and over 6.3 TB/s (a measured copy).  Wall times are call + synchronise, median of --reps
after warm-up.  The grid_sample version follows the same points forward with the same test (bilinear, border padding,
align_corners=True: positions agree with the kernel's rule inside the image, not bit for bit); its visible count is
printed next to the kernel's.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o track -- python3 tools/track_probe.py --kernel-only
    python3 tools/track_probe.py --kernel-stats DIR --out profiles/track_probe.txt
(--kernel-stats: the directory rocprofv3 wrote, searched for *kernel_stats.csv; k_track<true> is the dense case,
k_track<false> the sparse one.)"""
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

from papteam_opticalflow_amd.tensors import CONSISTENCY, flow_video_fb, track_points  # noqa: E402

SPEC_BW, COPY_BW = 8.0e12, 6.3e12


def video(res, n):
    """n frames that all differ: the two decoded frames of the reference's collection, shifted copies of them"""
    import cases
    a, b = cases.load_frame_u8(res, 1), cases.load_frame_u8(res, 2)
    return np.stack([np.roll(a if i % 2 == 0 else b, (i // 2) * 3, axis=1) for i in range(n)])


def dense_case(dev):
    T, H, W = 16, 1080, 1920
    g = torch.Generator().manual_seed(5)
    fw = (torch.randn(T - 1, 2, H // 32 + 1, W // 32 + 1, generator=g, dtype=torch.float64) * 1.5).to(dev)
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.05 * torch.randn(T - 1, 2, H, W, generator=g, dtype=torch.float64).to(dev)
    return "dense 1920x1080, T = 16", fw.contiguous(), bw.contiguous(), None


def sparse_case(dev):
    frames = torch.from_numpy(video("240", 101)).to(dev)
    fb = flow_video_fb(frames, 5, layout="NHWC", consistency=None)
    T, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    g = torch.Generator().manual_seed(6)
    q = torch.stack([torch.zeros(1024, dtype=torch.float64), torch.rand(1024, generator=g, dtype=torch.float64) * (W - 1),
                     torch.rand(1024, generator=g, dtype=torch.float64) * (H - 1)], 1).to(dev)
    return "sparse N = 1024, 240x135, T = %d" % T, fb.flow_fw, fb.flow_bw, q


def floor_bytes(fw, n_points):
    T = fw.shape[0] + 1
    flows = 2 * fw.numel() * 8
    return flows, T * n_points * 17


def torch_track(fw, bw, x, y, alpha1=CONSISTENCY[0], alpha2=CONSISTENCY[1]):
    """the forward steps from frame 0 with grid_sample: per step two gathers, the bounds test and the consistency test"""
    T, H, W = fw.shape[0] + 1, fw.shape[2], fw.shape[3]
    N = x.numel()
    tracks = torch.empty((T, N, 2), dtype=torch.float64, device=fw.device)
    vis = torch.empty((T, N), dtype=torch.bool, device=fw.device)
    alive = torch.ones(N, dtype=torch.bool, device=fw.device)
    tracks[0, :, 0], tracks[0, :, 1], vis[0] = x, y, alive
    sx, sy = 2.0 / (W - 1) if W > 1 else 0.0, 2.0 / (H - 1) if H > 1 else 0.0

    def sample(f, px, py):
        grid = torch.stack([px * sx - 1, py * sy - 1], -1).view(1, 1, N, 2)
        s = torch.nn.functional.grid_sample(f.unsqueeze(0), grid, mode="bilinear", padding_mode="border",
                                            align_corners=True)
        return s[0, 0, 0], s[0, 1, 0]

    for t in range(T - 1):
        u, v = sample(fw[t], x, y)
        X, Y = x + u, y + v
        ok = alive & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        bu, bv = sample(bw[t], X.nan_to_num(0.0), Y.nan_to_num(0.0))
        e = (u + bu) ** 2 + (v + bv) ** 2
        m = (u * u + v * v) + (bu * bu + bv * bv)
        alive = ok & (e <= alpha1 * m + alpha2)
        x, y = torch.where(alive, X, float("nan")), torch.where(alive, Y, float("nan"))
        tracks[t + 1, :, 0], tracks[t + 1, :, 1], vis[t + 1] = x, y, alive
    return tracks, vis


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


def kernel_stats(path):
    """{'dense' | 'sparse': (calls, average us)} from rocprofv3's kernel statistics CSV"""
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True) if os.path.isdir(path) else [path]
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % path)
    out = {}
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        name = row.get("name", row.get("kernel_name", ""))
        if "k_track" not in name:
            continue
        case = "dense" if "k_track<true>" in name else "sparse"
        us = [float(row.get(k, "nan")) / 1e3 for k in ("averagens", "minns", "maxns")]
        out[case] = (int(row.get("calls", 0)), us[0], us[1], us[2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="run track_points only, --reps times per case (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None,
                    help="rocprofv3 output directory (or kernel_stats.csv) of a --kernel-only run")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = [dense_case(dev), sparse_case(dev)]
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, fw, bw, q in cases:
            for _ in range(args.reps):
                track_points(fw, bw, q)
            torch.cuda.synchronize()
        return
    ks = kernel_stats(args.kernel_stats) if args.kernel_stats else {}
    rep = io.StringIO()

    def say(s=""):
        print(s)
        rep.write(s + "\n")

    say("Point tracking on one %s device: track_points (one k_track launch) against its byte floor and against the same "
        "forward steps with torch grid_sample in float64.  Wall: call + synchronise, median (min, max) of %d after "
        "warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for key, (what, fw, bw, q) in zip(("dense", "sparse"), cases):
        T, H, W = fw.shape[0] + 1, fw.shape[2], fw.shape[3]
        N = q.shape[0] if q is not None else H * W
        flows, outs = floor_bytes(fw, N)
        floor_us = 1e6 * (flows + outs) / SPEC_BW
        say()
        say("%s: %d points, %d steps" % (what, N, T - 1))
        say("  byte floor: flow planes %.1f MB read once + tracks and visible %.1f MB written once = %.1f MB: %.1f us at 8 TB/s, "
            "%.1f us at 6.3 TB/s" % (flows / 1e6, outs / 1e6, (flows + outs) / 1e6, floor_us, 1e6 * (flows + outs) / COPY_BW))
        res = {}
        med, lo, hi = wall(lambda: res.__setitem__("k", track_points(fw, bw, q)), args.reps)
        say("  track_points          wall %10.1f us  (%.1f, %.1f)   visible at the last frame %d, over all frames %.3f" % (
            1e6 * med, 1e6 * lo, 1e6 * hi, int(res["k"].visible[-1].sum()), float(res["k"].visible.double().mean())))
        if q is not None:
            x, y = q[:, 1].contiguous(), q[:, 2].contiguous()
        else:
            n = torch.arange(H * W, device=fw.device)
            x, y = (n % W).double(), (n // W).double()
        med_t, lo_t, hi_t = wall(lambda: res.__setitem__("t", torch_track(fw, bw, x, y)), max(3, args.reps // 4))
        say("  grid_sample, float64  wall %10.1f us  (%.1f, %.1f)   visible at the last frame %d   (%.1f x track_points)" % (
            1e6 * med_t, 1e6 * lo_t, 1e6 * hi_t, int(res["t"][1][-1].sum()), med_t / med))
        if key in ks:
            calls, avg, kmin, kmax = ks[key]
            say("  k_track (rocprofv3 --kernel-trace --stats, %d dispatches): average %.1f us (min %.1f, max %.1f) = %.2f x "
                "the 8 TB/s floor, %.2f x the 6.3 TB/s one; %.2f TB/s of floor bytes" % (
                    calls, avg, kmin, kmax, avg / floor_us, avg / (1e6 * (flows + outs) / COPY_BW),
                    (flows + outs) / (avg * 1e-6) / 1e12))
            if key == "sparse":
                say("  per dependent gather round trip (2 per step, %d steps): %.2f us" % (T - 1, avg / (2 * (T - 1))))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
