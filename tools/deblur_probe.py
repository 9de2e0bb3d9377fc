#!/usr/bin/env python3
"""Cost of video deblurring (tensors.deblur -> papof_deblur_tensor: k_deblur_ingest, then k_deblur_ratio and k_deblur_update
per iteration) on one device, against three yardsticks.

Cases, all uint8 NHWC frames of 3 channels, float64 flows, uint8 out, radius 1, 6 iterations, 16 samples of a centred box
shutter of 0.5 frames:
  1080p smooth   8 frames of 1920x1080, smooth flows of about 4 pixels (a pixel's 16 samples lie in two or three cells);
  1080p random   the same frames, independent uniform random flows of up to 20 pixels per component and pixel (no
                 locality between neighbouring lanes, and most chains fail the consistency test);
  240            32 frames of 240x135 made from the committed frames, smooth 4-pixel flows.

Yardsticks:
  torch          the same rule in PyTorch operations in float32: one grid_sample per sample, slot and pass over all targets
                 at once, one hop per neighbour with the consistency test, full-frame temporaries.  The kernels' reason to
                 exist is the launches and temporaries this takes; the bar is that they are faster.
  byte floor     of one iteration: L and the 2 R + 1 ratio images of every target written once and read once, both flows
                 read once, over the 6.3 TB/s that streaming kernels reach on this device.
  motion_blur    2 (2 R + 1) calls of tensors.motion_blur on the same frames and flows per iteration: the gather cost of as
                 many line integrals per pixel with the forward model's kernel (two frames per sample, uint8 taps).

All timings are device time between events around one call, median (min, max) of --reps (11) calls after two warm-up
calls, all in one run; the torch composition with --torch-reps (5)."""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import CONSISTENCY, blur_schedule, deblur, motion_blur  # noqa: E402

SHUTTER, K, R, ITERS = 0.5, 16, 1, 6
HBM = 6.3e12
EPS = 2.0 ** -10


def smooth_flows(B, H, W, seed, amp=4.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(B, 2, H // 64 + 2, W // 64 + 2, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.05 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def random_flows(B, H, W, seed, amp=20.0):
    g = torch.Generator().manual_seed(seed)
    fw = (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) * 2 - 1) * amp
    bw = (torch.rand(B, 2, H, W, generator=g, dtype=torch.float64) * 2 - 1) * amp
    return fw, bw


def videos(dev):
    import cases
    g = torch.Generator().manual_seed(7)
    big = torch.randint(0, 256, (8, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    small = torch.from_numpy(np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(32)])).to(dev)
    out = []
    for name, v, make in (("1920x1080, 8 frames, smooth 4-pixel flows", big, smooth_flows),
                          ("1920x1080, 8 frames, random 20-pixel flows", big, random_flows),
                          ("240x135, 32 frames, smooth 4-pixel flows", small, smooth_flows)):
        T, H, W, _ = v.shape
        fw, bw = (f.to(dev) for f in make(T - 1, H, W, 8))
        out.append((name, v, fw, bw))
    return out


# ---- the rule in PyTorch operations, float32, radius 1
def _sample(img, X, Y):
    """img (N, C, H, W) sampled bilinearly at the points (X, Y) (N, H, W), clamped into the image"""
    H, W = img.shape[2:]
    grid = torch.stack([2.0 * X / max(W - 1, 1) - 1.0, 2.0 * Y / max(H - 1, 1) - 1.0], -1)
    return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)


def _hop(f, b, X, Y, a1, a2):
    """the points (X, Y) (N, H, W) through the flows f (N, 2, H, W) read at the pixels, tested against b where they land"""
    H, W = X.shape[1:]
    u, v = f[:, 0], f[:, 1]
    nX, nY = X + u, Y + v
    alive = (nX >= 0) & (nX <= W - 1) & (nY >= 0) & (nY <= H - 1)
    back = _sample(b, nX.clamp(0, W - 1), nY.clamp(0, H - 1))
    du, dv = u + back[:, 0], v + back[:, 1]
    alive &= du * du + dv * dv <= a1 * ((u * u + v * v) + (back[:, 0] ** 2 + back[:, 1] ** 2)) + a2
    return nX, nY, alive


def _line(img, X, Y, vx, vy, table, sign):
    H, W = img.shape[2:]
    acc = torch.zeros_like(img)
    for tau, w in table:
        acc += w * _sample(img, (X + sign * tau * vx).clamp(0, W - 1), (Y + sign * tau * vy).clamp(0, H - 1))
    return acc


def composition(v, fw, bw):
    """deblur's result for radius 1 from PyTorch operations in float32: uint8 NHWC in and out"""
    off, w = blur_schedule(SHUTTER, K)
    table, wsum = list(zip(off, w)), float(sum(w))
    a1, a2 = CONSISTENCY
    b = (v.permute(0, 3, 1, 2).float() / 255.0).clamp_min(0.0)
    fw, bw = fw.float(), bw.float()
    T, _, H, W = b.shape
    vel = torch.empty((T, 2, H, W), dtype=torch.float32, device=v.device)
    vel[0], vel[-1], vel[1:-1] = fw[0], -bw[-1], 0.5 * (fw[1:] - bw[:-1])
    y, x = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float32),
                          torch.arange(W, device=v.device, dtype=torch.float32), indexing="ij")
    x, y = x.expand(T, H, W), y.expand(T, H, W)
    # slot d of the targets tg: the frames sl, the hop from a slot's pixel to the target and the hop back
    slots = ((slice(0, T), slice(0, T), None, None), (slice(0, T - 1), slice(1, T), (bw, fw), (fw, bw)),
             (slice(1, T), slice(0, T - 1), (fw, bw), (bw, fw)))
    L = b.clone()
    for _ in range(ITERS):
        corr, n = torch.zeros_like(L), torch.zeros((T, 1, H, W), dtype=torch.float32, device=v.device)
        for tg, sl, to_target, to_slot in slots:
            N = sl.stop - sl.start
            if to_target is None:
                X, Y, alive = x, y, torch.ones((T, H, W), dtype=torch.bool, device=v.device)
            else:
                X, Y, alive = _hop(to_target[0], to_target[1], x[:N], y[:N], a1, a2)
            est = _line(L[tg], X, Y, vel[sl, 0], vel[sl, 1], table, 1.0) / wsum
            ratio = torch.where(alive[:, None], b[sl] / est.clamp_min(EPS), torch.ones_like(est))
            if to_slot is None:
                X, Y, alive = x, y, torch.ones((T, H, W), dtype=torch.bool, device=v.device)
            else:
                X, Y, alive = _hop(to_slot[0], to_slot[1], x[:N], y[:N], a1, a2)
            vs = _sample(vel[sl], X.clamp(0, W - 1), Y.clamp(0, H - 1))
            cs = _line(ratio, X, Y, vs[:, 0], vs[:, 1], table, -1.0) / wsum
            corr[tg] += torch.where(alive[:, None], cs, torch.zeros_like(cs))
            n[tg] += alive[:, None].float()
        L = torch.where(n > 0, L * (corr / n.clamp_min(1.0)), L)
    return torch.clamp(torch.round(255.0 * L), 0, 255).to(torch.uint8).permute(0, 2, 3, 1)


def device_time(fn, reps):
    """(median, min, max) in ms of the device time between events around one call, after two warm-up calls"""
    fn()
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dt.append(e0.elapsed_time(e1))
    return float(np.median(dt)), min(dt), max(dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Video deblurring on one %s device: deblur (k_deblur_ingest, then k_deblur_ratio and k_deblur_update per iteration) "
        "against the same rule in PyTorch operations in float32, the byte floor of its iterations and as many motion_blur "
        "calls.  uint8 NHWC frames (C = 3), float64 flows, uint8 out, radius %d, %d iterations, %d samples, shutter %.1f.  "
        "Device time between events around one call, median (min, max) of %d calls (torch: %d) after two warm-up calls, in "
        "one run." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], R, ITERS, K, SHUTTER, args.reps, args.torch_reps))
    for what, v, fw, bw in videos(dev):
        T, H, W, C = v.shape
        say()
        say("%s: %d pixels per frame" % (what, H * W))
        res = {}
        ours = device_time(lambda: res.__setitem__("k", deblur(v, fw, bw, shutter=SHUTTER, samples=K, radius=R, iters=ITERS,
                                                               layout="NHWC").video), args.reps)
        comp = device_time(lambda: res.__setitem__("c", composition(v, fw, bw)), args.torch_reps)
        blur = device_time(lambda: [motion_blur(v, fw, bw, shutter=SHUTTER, samples=K, layout="NHWC")
                                    for _ in range(2 * (2 * R + 1) * ITERS)], args.reps)
        diff = (res["k"].int() - res["c"].int()).abs()
        floor = ITERS * (2 * T * 8 * C * H * W * (2 * R + 2) + 2 * (T - 1) * 2 * H * W * 8)
        say("  deblur                      %9.2f ms  (%.2f, %.2f)" % ours)
        say("  torch composition, float32  %9.2f ms  (%.2f, %.2f)   deblur takes %.3f of it; %.4f of the output bytes are equal, "
            "%.4f within one level" % (comp + (ours[0] / comp[0], float((diff == 0).double().mean()), float((diff <= 1).double().mean()))))
        say("  byte floor of %d iterations  %9.2f ms  (%.1f MB at %.1f TB/s)   deblur takes %.1f x that" % (
            ITERS, floor / HBM * 1e3, floor / 1e6, HBM / 1e12, ours[0] / (floor / HBM * 1e3)))
        say("  %d motion_blur calls        %9.2f ms  (%.2f, %.2f)   deblur takes %.3f of it" % (
            (2 * (2 * R + 1) * ITERS,) + blur + (ours[0] / blur[0],)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
