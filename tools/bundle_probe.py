#!/usr/bin/env python3
"""Cost of the bundle adjustment's device half (tensors.bundle_sums -> k_bundle_sums, k_bundle_reduce) on one device, against
what the parent had in the same run -- never against itself.

Cases:
  (a) sums      8 links of 1080p float64 flows (a 3 degree yaw each, 0.3 px of noise): bundle_sums at steps 1, 2 and 4 against
                ONE iteration of global_homography on the same flows.  Both read a flow once and reduce it to a few fp64
                sums per pair in a fixed order (twenty against twenty-five); k_homography_sums is the yardstick.  Reported per
                sampled link-pixel and per pair-pixel.  bundle_sums' time includes the copy of the links' ten doubles to the
                device; the line "rows on the device" leaves it out.
  (b) evaluate  one evaluation of bundle_adjust -- bundle_sums and the copy of (L, 20) doubles to the host, with the wait --
                against the same twenty sums written in torch operations (float64, one reduction per sum) and copied likewise.
The two sides of a comparison alternate inside one loop.  Times are host wall time around work that ends in a device
synchronise, median (min, max) of --reps after warm-up.

    python3 tools/bundle_probe.py --out profiles/bundle_probe.txt"""
import argparse
import io
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd import capi, tensors  # noqa: E402

TRI = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


def yaw(a):
    return np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])


def scene(L, H, W, f, dev):
    """(flows (L, 2, H, W) float64 on dev, R (L, 3, 3) numpy): the flows of a 3 degree yaw with 0.3 px of noise"""
    R = np.stack([yaw(math.radians(3.0 + 0.1 * l)) for l in range(L)])
    g = torch.Generator(device="cpu").manual_seed(1)
    flow = tensors._rotation_flow(torch.from_numpy(R).to(dev), H, W, f, dev)
    return flow + 0.3 * torch.randn(flow.shape, generator=g, dtype=torch.float64).to(dev), R


def torch_sums(flow, R, f, scale=1.0):
    """bundle_sums' twenty sums in torch operations (its order of additions aside)"""
    L, _, H, W = flow.shape
    dev = flow.device
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    x = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    r = R.view(L, 9, 1, 1)
    X, Y = x + flow[:, 0], y + flow[:, 1]
    px, py = (x - cx) / f, (y - cy) / f
    qx, qy, qz = (r[:, 0] * px + r[:, 1] * py) + r[:, 2], (r[:, 3] * px + r[:, 4] * py) + r[:, 5], (r[:, 6] * px + r[:, 7] * py) + r[:, 8]
    valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1) & (qz > tensors.MIN_DEN)
    gx, gy = qx / qz, qy / qz
    ex, ey = X - (f * gx + cx), Y - (f * gy + cy)
    e2 = ex * ex + ey * ey
    w = torch.where(valid, 1.0 / (1.0 + e2 / (scale * scale)), torch.zeros((), dtype=torch.float64, device=dev))
    Jx = [-(f * gx * gy), f + f * gx * gx, -(f * gy), gx + (r[:, 2] - gx * r[:, 8]) / qz]
    Jy = [-(f + f * gy * gy), f * gx * gy, f * gx, gy + (r[:, 5] - gy * r[:, 8]) / qz]
    z = torch.zeros((), dtype=torch.float64, device=dev)
    terms = [w * (Jx[a] * Jx[b] + Jy[a] * Jy[b]) for a, b in TRI] + [w * (Jx[a] * ex + Jy[a] * ey) for a in range(4)]
    terms += [w * e2, w, valid.to(torch.float64), torch.where(valid, e2, z)]
    S = torch.stack([torch.where(valid, t, z).sum((1, 2)) for t in terms], 1)
    return torch.cat([S, torch.zeros((L, 2), dtype=torch.float64, device=dev)], 1)


def alternate(fns, reps):
    """[(median, min, max)] in microseconds of each function, called in turn inside one loop, each ending in a synchronise"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dt = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt[k].append((time.perf_counter() - t0) * 1e6)
    return [(float(np.median(d)), min(d), max(d)) for d in dt]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--links", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    L, H, W, f = args.links, 1080, 1920, 1700.0
    flow, R = scene(L, H, W, f, dev)
    Rt = torch.from_numpy(R)
    rows = torch.from_numpy(np.concatenate([R.reshape(L, 9), np.full((L, 1), f)], 1)).to(dev)
    say("Bundle adjustment's device half on one %s device: %d links of %d x %d float64 flows.  Host wall time around work that "
        "ends in a synchronise, median (min, max) of %d after warm-up, the sides of a comparison alternating in one loop."
        % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], L, W, H, args.reps))
    a, b = tensors.bundle_sums(flow, Rt, f).cpu().numpy(), torch_sums(flow, rows[:, :9].contiguous(), f).cpu().numpy()
    say("bundle_sums against the torch operations: largest relative difference of a sum %.2e, valid samples %d of %d"
        % (float(np.abs(a - b).max() / np.abs(b).max()), int(a[:, 16].sum()), L * H * W))
    say()
    say("(a) sums: per pixel read")
    for step in (1, 2, 4):
        n = L * ((H - 1) // step + 1) * ((W - 1) // step + 1)
        t = alternate([lambda: tensors.bundle_sums(flow, Rt, f, step=step),
                       lambda: tensors._bundle_sums(flow, capi.DTYPE_F64, None, rows, step, 1.0),
                       lambda: tensors.global_homography(flow, iters=1)], args.reps)
        say("  step %d: bundle_sums %9.1f us (%.1f, %.1f) = %.3f ns per sampled link-pixel; rows on the device %9.1f us (%.1f, %.1f) = "
            "%.3f ns" % (step, t[0][0], t[0][1], t[0][2], 1e3 * t[0][0] / n, t[1][0], t[1][1], t[1][2], 1e3 * t[1][0] / n))
        say("          global_homography, 1 iteration %9.1f us (%.1f, %.1f) = %.3f ns per pair-pixel; bundle_sums / it %.2f x"
            % (t[2][0], t[2][1], t[2][2], 1e3 * t[2][0] / (L * H * W), t[0][0] / t[2][0]))
    say()
    say("(b) one evaluation of bundle_adjust, the copy to the host included")
    t = alternate([lambda: tensors.bundle_sums(flow, Rt, f).cpu(),
                   lambda: torch_sums(flow, rows[:, :9].contiguous(), f).cpu()], args.reps)
    say("  bundle_sums + copy %9.1f us (%.1f, %.1f);  torch operations + copy %9.1f us (%.1f, %.1f): %.1f x"
        % (t[0] + t[1] + (t[1][0] / t[0][0],)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(rep.getvalue())


if __name__ == "__main__":
    main()
