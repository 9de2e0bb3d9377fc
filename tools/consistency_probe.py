#!/usr/bin/env python3
"""Cost of blind video temporal consistency (tensors.temporal_consistency -> papof_temporal_consistency_tensor: per frame
k_tc_setup, the k_tc_pull / k_tc_push pull-push and ceil(iters / depth) launches of k_tc_jacobi) against its compulsory byte
floor and against the same rule written with PyTorch (grid_sample hop, avg_pool2d / interpolate pull-push, conv2d Jacobi)
in float64.

Cases, uint8 NHWC frames and processed video (3 channels each), float64 flows, the defaults (lambda 4, sigma 0.05, 20
sweeps, the check on), uint8 out:
  240 T=101     101 frames of 240x135;
  1080p T=16    sixteen 1920x1080 frames.
Flows are smooth random fields (bw = -fw + noise) of a few pixels.  Each case also sweeps PAPOF_TC_DEPTH (sweeps per
k_tc_jacobi launch; the bits do not change) and times 0 and 100 sweeps.

Compulsory bytes per frame t >= 1: I_t and I_{t-1}, P_t, both flows of the pair (float64) and O_{t-1} read once, O_t written
once: H W (2 C_I + 2 C_P + 32) for uint8 frames and out; frame 0: P_0 read and O_0 written.  Over 8 TB/s (spec).  Wall
times are call + synchronise, median of --reps after warm-up.

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o consistency -- python3 tools/consistency_probe.py --kernel-only
(the kernel statistics file then holds the per-kernel totals of --reps calls per case)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from papteam_opticalflow_amd.tensors import ITERS, LAM, SIGMA, temporal_consistency  # noqa: E402

SPEC_BW = 8.0e12


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = Fn.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def make_case(T, H, W, dev, seed):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
    gain = 0.8 + 0.4 * torch.rand(T, 1, 1, 3, generator=g, dtype=torch.float64)
    proc = (frames.double() * gain + 25.0 * torch.rand(T, 1, 1, 3, generator=g, dtype=torch.float64)).clamp(0, 255)
    fw, bw = flows(T - 1, H, W, seed + 1)
    return frames.to(dev), proc.round().to(torch.uint8).to(dev), fw.to(dev), bw.to(dev)


def levels(H, W):
    n = 0
    while H > 1 or W > 1:
        H, W, n = (H + 1) // 2, (W + 1) // 2, n + 1
    return n


def torch_composition(frames, proc, fw, bw, lam, sigma, iters, alphas=(0.01, 0.5)):
    """the rule in PyTorch float64 (not bit-exact: grid_sample's taps, avg_pool2d's child weights and conv2d's sums)"""
    T, H, W, C = frames.shape
    I = frames.permute(0, 3, 1, 2).double() / 255.0
    P = proc.permute(0, 3, 1, 2).double() / 255.0
    ys, xs = torch.meshgrid(torch.arange(H, device=I.device, dtype=torch.float64),
                            torch.arange(W, device=I.device, dtype=torch.float64), indexing="ij")
    k = torch.tensor([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=torch.float64, device=I.device).view(1, 1, 3, 3).repeat(C, 1, 1, 1)
    n = Fn.conv2d(Fn.pad(torch.ones(1, 1, H, W, dtype=torch.float64, device=I.device), (1, 1, 1, 1)), k[:1])

    def sample(img, X, Y):
        grid = torch.stack((2 * X / max(W - 1, 1) - 1, 2 * Y / max(H - 1, 1) - 1), -1)[None]
        return Fn.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    O = [P[0:1]]
    for t in range(1, T):
        X, Y = xs + bw[t - 1, 0], ys + bw[t - 1, 1]
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        f = sample(fw[t - 1:t], X, Y)[0]
        e = (bw[t - 1, 0] + f[0]) ** 2 + (bw[t - 1, 1] + f[1]) ** 2
        valid &= e <= alphas[0] * ((bw[t - 1] ** 2).sum(0) + (f ** 2).sum(0)) + alphas[1]
        D = ((I[t:t + 1] - sample(I[t - 1:t], X, Y)) ** 2).mean(1, keepdim=True)
        w = torch.where(valid[None, None], lam / (1 + D / sigma ** 2), torch.zeros_like(D))
        r = torch.where(valid[None, None], sample(O[-1], X, Y) - P[t:t + 1], torch.zeros_like(P[:1]))
        a = w / lam
        pyr = [(r, a)]
        while pyr[-1][0].shape[-2:] != (1, 1):
            v, c = pyr[-1]
            A = Fn.avg_pool2d(c, 2, ceil_mode=True) * 4
            S = Fn.avg_pool2d(c * v, 2, ceil_mode=True) * 4
            pyr.append((torch.where(A > 0, S / A.clamp_min(1e-300), torch.zeros_like(S)), A.clamp(max=1)))
        v = pyr[-1][0]
        for vl, cl in reversed(pyr[:-1]):
            up = Fn.interpolate(v, size=vl.shape[-2:], mode="bilinear", align_corners=False)
            v = cl * vl + (1 - cl) * up
        d, den, wr = v, n + w, w * r
        for _ in range(iters):
            d = (Fn.conv2d(Fn.pad(d, (1, 1, 1, 1)), k, groups=C) + wr) / den
        O.append(((P[t:t + 1] + d) * 255).round().clamp(0, 255) / 255)
    return torch.cat(O)


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="the default calls only (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Temporal consistency on one gfx950 device: temporal_consistency (k_tc_* chain) against its compulsory byte floor "
        "and a PyTorch composition in float64.  uint8 NHWC frames and processed video (C = 3), float64 flows, lambda %g, "
        "sigma %g, %d sweeps, check on, uint8 out.  Wall: call + synchronise, median (min, max) of %d after warm-up."
        % (LAM, SIGMA, ITERS, args.reps))
    for T, H, W in ((101, 135, 240), (16, 1080, 1920)):
        frames, proc, fw, bw = make_case(T, H, W, dev, T)
        call = lambda iters=ITERS: temporal_consistency(frames, proc, fw, bw, layout="NHWC", iters=iters)  # noqa: E731
        if args.kernel_only:
            for _ in range(args.reps):
                call()
            torch.cuda.synchronize()
            continue
        L = levels(H, W)
        floor = (T - 1) * H * W * (2 * 3 + 2 * 3 + 32) + H * W * 6
        say()
        say("%dx%d, T = %d: %d levels below the frame; compulsory floor %.1f MB: %.1f us at 8 TB/s (%.2f us per frame)"
            % (W, H, T, L, floor / 1e6, floor / SPEC_BW * 1e6, floor / SPEC_BW * 1e6 / (T - 1)))
        for depth in ("1", "2", "4", "8", "15"):
            os.environ["PAPOF_TC_DEPTH"] = depth
            m, lo, hi = wall(call, args.reps)
            launches = 1 + (T - 1) * (1 + 2 * L + -(-ITERS // int(depth)))
            say("  PAPOF_TC_DEPTH %2s  wall %10.1f us  (%.1f, %.1f)  %7.1f us per frame, %d launches, %.1f x floor"
                % (depth, m, lo, hi, m / (T - 1), launches, m / (floor / SPEC_BW * 1e6)))
        os.environ.pop("PAPOF_TC_DEPTH")
        for iters in (0, 100):
            m, lo, hi = wall(lambda: call(iters), args.reps)
            say("  iters %3d (default depth)  wall %10.1f us  (%.1f, %.1f)  %7.1f us per frame" % (iters, m, lo, hi,
                                                                                             m / (T - 1)))
        m0, _, _ = wall(call, args.reps)
        reps = max(2, args.reps // 5)
        mt, lo, hi = wall(lambda: torch_composition(frames, proc, fw, bw, LAM, SIGMA, ITERS), reps)
        say("  torch composition    wall %10.1f us  (%.1f, %.1f)  %7.1f us per frame: %.1f x temporal_consistency"
            % (mt, lo, hi, mt / (T - 1), mt / m0))
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
