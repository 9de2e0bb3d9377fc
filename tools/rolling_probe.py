#!/usr/bin/env python3
"""Cost of rolling-shutter rectification on one device: tensors.rectify_frames with and without matrices (one k_rs_rectify
launch), tensors.rectify_flows (one k_rs_flow launch) and tensors.warp_affine on the same frames -- the floor of one gather
--, against the same rule composed of PyTorch operations, and the kernel's bytes against its byte floor.

Workloads: 8 frames of 1080 x 1920 x 3 and 32 frames of 135 x 240 x 3, uint8 NHWC, float64 flows: smooth random fields of a
few pixels, bw = -fw + noise; readout 0.8, anchor 0.5, 3 iterations.  The PyTorch composition is the rule without matrices,
in float64 and in float32: per iteration one grid_sample (bilinear, border padding, align_corners=True: positions agree with
the kernel's rule inside the image, the arithmetic is not bit for bit the kernel's) of the frame's two flows stacked as four
channels, the guards, the parabola's coefficients and the update as elementwise operations, and at the end one grid_sample
of a float copy of the frames, the mask and the conversion to uint8.  Times are device times between two events around one
call, the median of --reps (11) after warm-up, all versions in the same run; the share of output bytes that agree is printed.

Byte floor: both flow fields read once and the frames read and written once, over the 6.3 TB/s that streaming kernels reach
on this device.  Beside it the bytes the lanes ask for: per output pixel and iteration 2 x 4 flow taps of 16 bytes (4 on an
end frame), then 4 C frame bytes, C output bytes and the valid byte.

    python3 tools/rolling_probe.py --out profiles/rolling_probe.txt"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import rectify_flows, rectify_frames, warp_affine  # noqa: E402

HBM = 6.3e12  # bytes per second that streaming kernels reach
READOUT, ANCHOR, ITERS = 0.8, 0.5, 3


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def matrices(T, H, W, seed):
    """small rotations and shifts about the centre, (T, 2, 3) float64"""
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    M = np.empty((T, 2, 3))
    for i in range(T):
        th, t = rng.normal(0, 0.01), rng.normal(0, 4.0, 2)
        a, b = np.cos(th), np.sin(th)
        M[i] = [[a, -b, cx - a * cx + b * cy + t[0]], [b, a, cy - b * cx - a * cy + t[1]]]
    return torch.from_numpy(M)


class TorchRule:
    """papof_rs_rectify_tensor without matrices in PyTorch operations of `dtype`; what does not depend on the frames' values
    or on the iterate -- the stacked flows, the pixel grid, the frames' kinds -- is prepared once, outside the timed call"""

    def __init__(self, fw, bw, dtype):
        P, _, H, W = fw.shape
        T, dev = P + 1, fw.device
        z = torch.zeros((1, 2, H, W), dtype=dtype, device=dev)
        self.G = torch.cat([torch.cat([fw.to(dtype), z]), torch.cat([z, bw.to(dtype)])], 1)  # (T, 4, H, W): fw[t], bw[t - 1]
        y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=dtype), torch.arange(W, device=dev, dtype=dtype), indexing="ij")
        self.x, self.y = x.expand(T, H, W), y.expand(T, H, W)
        t = torch.arange(T, device=dev)[:, None, None]
        self.first, self.last = t == 0, t == T - 1
        self.T, self.H, self.W, self.dtype = T, H, W, dtype
        self.r, self.a = READOUT / H, ANCHOR * (H - 1)

    def sample(self, img, X, Y):
        grid = torch.stack([X * (2.0 / (self.W - 1)) - 1, Y * (2.0 / (self.H - 1)) - 1], -1)
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    def inside(self, X, Y):
        return (X >= 0) & (X <= self.W - 1) & (Y >= 0) & (Y <= self.H - 1)

    def __call__(self, v):
        """uint8 NHWC frames -> (uint8 NHWC video, valid)"""
        r = self.r
        Px, Py, alive = self.x, self.y, torch.ones_like(self.x, dtype=torch.bool)
        for _ in range(ITERS):
            s = (self.a - Py) * r
            Fu, Fv, Bu, Bv = self.sample(self.G, Px, Py).unbind(1)
            tf, tb = 1.0 + r * Fv, r * Bv - 1.0
            cF = torch.where(self.first, s / tf, (s * (s - tb)) / (tf * (tf - tb)))
            cB = torch.where(self.last, s / tb, (s * (s - tf)) / (tb * (tb - tf)))
            cF, cB = torch.where(self.last, torch.zeros_like(cF), cF), torch.where(self.first, torch.zeros_like(cB), cB)
            alive = alive & ((s == 0) | (((tf >= 0.5) | self.last) & ((tb <= -0.5) | self.first)))
            Px = torch.where(s == 0, self.x, self.x - (cF * Fu + cB * Bu))
            Py = torch.where(s == 0, self.y, self.y - (cF * Fv + cB * Bv))
            alive = alive & self.inside(Px, Py)
        img = v.permute(0, 3, 1, 2).to(self.dtype)
        out = torch.where(alive[:, None], self.sample(img, Px, Py), torch.zeros((), dtype=self.dtype, device=v.device))
        return out.round().clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1), alive


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


def frame_bytes(T, H, W, C):
    """(the byte floor, the bytes the lanes ask for) of one rectify_frames launch on uint8 frames and float64 flows"""
    px = H * W
    floor = 2 * (T - 1) * px * 16 + 2 * T * px * C
    asked = ITERS * ((T - 2) * 2 + 2) * px * 4 * 16 + T * px * (4 * C + C + 1)
    return floor, asked


def flow_bytes(T, H, W):
    """the same of one rectify_flows launch: the two flow fields read and written once; per output vector the solve's taps,
    the flow's own 4 and the 2 x 4 of the landing frame's displacement"""
    px, P = H * W, T - 1
    floor = 2 * 2 * P * px * 16
    asked = 2 * P * px * (ITERS * 2 * 4 * 16 + 4 * 16 + 2 * 4 * 16 + 16)
    return floor, asked


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

    say("Rolling-shutter rectification on one %s device: readout %g, anchor %g, %d iterations.  Device time between two events "
        "around one call, median of %d after warm-up; every version timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], READOUT, ANCHOR, ITERS, args.reps))
    for T, H, W, C in ((8, 1080, 1920, 3), (32, 135, 240, 3)):
        g = torch.Generator().manual_seed(T)
        v = torch.randint(0, 256, (T, H, W, C), generator=g, dtype=torch.uint8).to(dev)
        fw, bw = (f.to(dev) for f in flows(T - 1, H, W, 8))
        M = matrices(T, H, W, 9).to(dev)
        say()
        say("%d uint8 NHWC frames of %d x %d x %d, float64 flows" % (T, W, H, C))
        res = {}
        k = device_ms(lambda: res.__setitem__("k", rectify_frames(v, fw, bw, READOUT, anchor=ANCHOR, iters=ITERS, layout="NHWC")),
                      args.reps)
        km = device_ms(lambda: rectify_frames(v, fw, bw, READOUT, anchor=ANCHOR, iters=ITERS, matrices=M, layout="NHWC"), args.reps)
        kf = device_ms(lambda: rectify_flows(fw, bw, READOUT, anchor=ANCHOR, iters=ITERS), args.reps)
        w = device_ms(lambda: warp_affine(v, M, layout="NHWC"), args.reps)
        floor, asked = frame_bytes(T, H, W, C)
        say("  rectify_frames (k_rs_rectify)                 %9.3f ms   %.3f ms per frame; %.2f x warp_affine" % (k, k / T, k / w))
        say("  rectify_frames(matrices=M)                    %9.3f ms   %.2f x warp_affine" % (km, km / w))
        say("  warp_affine (k_warp_affine: one gather)       %9.3f ms" % w)
        say("    byte floor: %.1f MB (both flow fields and the frames read once, the video written once) = %.3f ms at %.1f TB/s: "
            "the kernel takes %.2f x that; the lanes ask for %.1f MB (%.2f TB/s)" % (
                floor / 1e6, floor / HBM * 1e3, HBM / 1e12, k / (floor / HBM * 1e3), asked / 1e6, asked / (k * 1e-3) / 1e12))
        floor, asked = flow_bytes(T, H, W)
        say("  rectify_flows (k_rs_flow, both directions)    %9.3f ms" % kf)
        say("    byte floor: %.1f MB = %.3f ms: the kernel takes %.2f x that; the lanes ask for %.1f MB (%.2f TB/s)" % (
            floor / 1e6, floor / HBM * 1e3, kf / (floor / HBM * 1e3), asked / 1e6, asked / (kf * 1e-3) / 1e12))
        for dtype in (torch.float64, torch.float32):
            rule = TorchRule(fw, bw, dtype)
            t = device_ms(lambda: res.__setitem__("t", rule(v)), args.reps)
            diff = (res["k"][0].int() - res["t"][0].int()).abs()
            say("  the rule in PyTorch operations, %-13s %9.3f ms   %.1f x the kernel; %.5f of the output bytes agree, %.5f "
                "within 1; valid agrees on %.5f" % (str(dtype).split(".")[1], t, t / k, float((diff == 0).double().mean()),
                                                    float((diff <= 1).double().mean()),
                                                    float((res["k"][1] == res["t"][1]).double().mean())))
            assert t > k, "the kernel must beat the composition"
            del rule
        say("  valid: %.4f of the pixels" % float(res["k"][1].double().mean()))
        del res, v, fw, bw
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
