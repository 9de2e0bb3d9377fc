#!/usr/bin/env python3
"""Cost of dirt and dropout removal on one device: tensors.detect_defects (one k_defect_detect launch) and
tensors.dilate_masks (one k_mask_dilate launch) against the same rules written with PyTorch operations, and the split of
one tensors.restore_video call.

Kernels: eight 1920x1080 uint8 NHWC frames (3 channels), float64 flows -- smooth random fields of a few pixels, bw = -fw +
noise --, the detector's defaults (threshold 0.08, no check); the dilation on the detector's masks with radius 2 and 32.
The PyTorch detector follows the same hops with grid_sample in float64 (bilinear, border padding, align_corners=True:
positions agree with the kernel's rule inside the image, the arithmetic is not bit for bit the kernel's) and takes the
range with minimum / maximum; the PyTorch dilation is max_pool2d on a float32 copy of the mask.  Times are device times
between two events around one call, the median of --reps (11) after warm-up, both versions in the same run; the share of
output bytes that agree is printed.

Split: restore_video at its defaults on eight 480x270 frames made from the committed pair (shifted copies, six blotches
per frame), 4 pyramid levels; every step of both passes timed between events by running the public calls by hand.

    python3 tools/restore_probe.py --out profiles/restore_probe.txt"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd import tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (complete_flows, detect_defects, dilate_masks, fill_holes, flow_video_fb,  # noqa: E402
                                             propagate, restore_video)

THR = tensors.DEFECT_THRESHOLD


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def torch_detect(v, fw, bw, thr):
    """the rule of papof_defect_detect_tensor without the check, with grid_sample and elementwise ops: the mask (T, H, W)"""
    T, H, W, C = v.shape
    I = v.permute(0, 3, 1, 2).double() / 255.0
    y, x = torch.meshgrid(torch.arange(H, device=v.device, dtype=torch.float64),
                          torch.arange(W, device=v.device, dtype=torch.float64), indexing="ij")

    def sample(img, X, Y):
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (H - 1)) - 1], -1)
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    def hop(f, X, Y, alive):
        uv = sample(f, X, Y)
        nX, nY = X + uv[:, 0], Y + uv[:, 1]
        return nX, nY, alive & (nX >= 0) & (nX <= W - 1) & (nY >= 0) & (nY <= H - 1)

    def judge(c, g1, g2, both):
        lo, hi = torch.minimum(g1, g2), torch.maximum(g1, g2)
        s = torch.maximum(c - hi, lo - c).amax(1).clamp_min(0.0)
        return both & (s > thr)

    out = torch.empty((T, H, W), dtype=torch.bool, device=v.device)
    n = T - 2  # the frames inside the video: one hop back, one hop forward
    X, Y, ones = x.expand(n, H, W), y.expand(n, H, W), torch.ones(n, H, W, dtype=torch.bool, device=v.device)
    X1, Y1, a1 = hop(bw[:T - 2], X, Y, ones)
    X2, Y2, a2 = hop(fw[1:], X, Y, ones)
    out[1:T - 1] = judge(I[1:T - 1], sample(I[:T - 2], X1, Y1), sample(I[2:], X2, Y2), a1 & a2)
    for t, f, o in ((0, fw, 1), (T - 1, bw, -1)):  # the ends: one chain of two hops
        pairs = (0, 1) if o > 0 else (T - 2, T - 3)
        X, Y, ones = x[None], y[None], torch.ones(1, H, W, dtype=torch.bool, device=v.device)
        X1, Y1, a1 = hop(f[pairs[0]:pairs[0] + 1], X, Y, ones)
        X2, Y2, a2 = hop(f[pairs[1]:pairs[1] + 1], X1, Y1, a1)
        out[t] = judge(I[t:t + 1], sample(I[t + o:t + o + 1], X1, Y1), sample(I[t + 2 * o:t + 2 * o + 1], X2, Y2), a2)[0]
    return out


def torch_dilate(m, radius):
    return torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 2 * radius + 1, stride=1, padding=radius)[:, 0] > 0


def device_ms(fn, reps):
    """median device time of fn() in ms between two events, after two warm-up calls"""
    fn()
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        dt.append(a.elapsed_time(b))
    return float(np.median(dt))


def split_video(dev):
    import cases
    f1, f2 = cases.load_frame_u8("480", 1), cases.load_frame_u8("480", 2)
    fr = np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(8)])
    rng = np.random.default_rng(5)
    T, H, W, _ = fr.shape
    y, x = np.mgrid[0:H, 0:W]
    for t in range(T):
        for _ in range(6):
            cy, cx, (a, b) = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2.0, 9.0, 2)
            fr[t][((x - cx) / (a / 2)) ** 2 + ((y - cy) / (b / 2)) ** 2 <= 1.0] = rng.integers(0, 40) if rng.random() < 0.5 else rng.integers(215, 256)
    return torch.from_numpy(fr).to(dev)


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

    say("Dirt and dropout removal on one %s device.  Device time between two events around one call, median of %d after "
        "warm-up; the kernel and the PyTorch version timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    g = torch.Generator().manual_seed(7)
    T, H, W, C = 8, 1080, 1920, 3
    base = torch.randint(0, 256, (1, H // 8, W // 8, C), generator=g, dtype=torch.uint8)
    v = base.repeat_interleave(8, 1).repeat_interleave(8, 2).repeat(T, 1, 1, 1).contiguous()
    for t in range(T):  # sparkle that differs from frame to frame, so that the masks are not empty
        v[t, 5 * t::37, 7 * t::41] = 255
    v = v.to(dev)
    fw, bw = (f.to(dev) for f in flows(T - 1, H, W, 8))
    say()
    say("detector: %d uint8 NHWC frames of %d x %d x %d, float64 flows, threshold %g, no check" % (T, W, H, C, THR))
    res = {}
    k = device_ms(lambda: res.__setitem__("k", detect_defects(v, fw, bw, layout="NHWC").mask), args.reps)
    t = device_ms(lambda: res.__setitem__("t", torch_detect(v, fw, bw, THR)), args.reps)
    say("  detect_defects (k_defect_detect)         %9.3f ms   %.3f ms per frame" % (k, k / T))
    say("  grid_sample + minimum / maximum, float64 %9.3f ms   %.1f x the kernel; %.5f of the mask bytes agree, %.4f flagged" % (
        t, t / k, float((res["t"] == res["k"]).double().mean()), float(res["k"].double().mean())))
    mask = res["k"]
    for radius in (2, 32):
        k = device_ms(lambda: res.__setitem__("k", dilate_masks(mask, radius)), args.reps)
        t = device_ms(lambda: res.__setitem__("t", torch_dilate(mask, radius)), args.reps)
        say("dilation, radius %d, on those masks" % radius)
        say("  dilate_masks (k_mask_dilate)             %9.3f ms" % k)
        say("  max_pool2d on a float32 copy             %9.3f ms   %.1f x the kernel; all bytes agree: %s" % (
            t, t / k, bool(torch.equal(res["t"], res["k"]))))
    del v, fw, bw, mask, res
    v = split_video(dev)
    T, H, W, C = v.shape
    levels, dil = 4, tensors.DEFECT_DILATE
    total = device_ms(lambda: restore_video(v, levels, layout="NHWC"), 3)
    say()
    say("restore_video at its defaults (2 passes, threshold %g, dilate %d), %d frames of %d x %d, %d levels: %.2f ms in all"
        % (THR, dil, T, W, H, levels, total))
    steps = {}

    def timed(name, fn):
        out = []
        steps[name] = steps.get(name, 0.0) + device_ms(lambda: out.append(fn()), 3)
        return out[-1]

    video, known = v, None
    for p in range(2):
        fb = timed("flow_video_fb", lambda: flow_video_fb(video, levels, layout="NHWC", consistency=None))
        first = timed("detect_defects", lambda: detect_defects(v, fb.flow_fw, fb.flow_bw, layout="NHWC").mask)
        if known is not None:
            first = first | known
        grown = timed("dilate_masks", lambda: dilate_masks(first, dil))
        cf = timed("complete_flows", lambda: complete_flows(fb.flow_fw, fb.flow_bw, grown))
        detected = first | timed("detect_defects", lambda: detect_defects(v, cf.flow_fw, cf.flow_bw, layout="NHWC").mask)
        m = timed("dilate_masks", lambda: dilate_masks(detected, dil))
        cf = timed("complete_flows", lambda: complete_flows(fb.flow_fw, fb.flow_bw, m))
        pr = timed("propagate", lambda: propagate(v, m, cf.flow_fw, cf.flow_bw, layout="NHWC", out_dtype=torch.float64))
        video = timed("fill_holes", lambda: fill_holes(pr.video, pr.status == 2, layout="NHWC", out_dtype=torch.uint8))
        known = detected
    for name, ms in steps.items():
        say("  %-16s %9.3f ms   (%4.1f %% of the steps' sum)" % (name, ms, 100.0 * ms / sum(steps.values())))
    say("  the steps' sum   %9.3f ms; %.4f of the pixels repaired in the last pass" % (sum(steps.values()), float(m.double().mean())))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
