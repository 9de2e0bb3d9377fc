#!/usr/bin/env python3
"""Cost of the per-row projective warp on one device: tensors.warp_rows (one k_warp_rows launch) at 17 knots and 3 iterations
and at 1 iteration; at one knot beside tensors.warp_homography on the same matrices -- the price of the path through the new
kernel --; tensors.rectify_frames(matrices=...) on the same frames, the flow-based way to stabilize and rectify in one
resampling; the same rule composed of PyTorch operations; and the kernel's bytes against its byte floor.

Workloads: 8 frames of 1080 x 1920 x 3 and 32 frames of 135 x 240 x 3, uint8 NHWC; float64 tables of a camera that shakes by
about 0.02 rad at a focal length of 0.9 W (tensors.rotation_rows of a random walk, smooth_rotations radius 6), readout 0.8.
The PyTorch composition is the rule in float64 and in float32: per iteration the clamp, the index, two torch.gather of the
table into full-frame temporaries of nine planes each, the lerp, the projection and two divisions, and at the end one
grid_sample (bilinear, border padding, align_corners=True: positions agree with the kernel's rule inside the image, the
arithmetic is not bit for bit the kernel's) of a float copy of the frames, the mask and the conversion to uint8.  Times are
device times between two events around one call, the median of --reps (11) after warm-up, all versions in the same run; the
share of output bytes that agree is printed.

Byte floor: the frames read once and the video and valid written once, over the 6.3 TB/s that streaming kernels reach on
this device.  Beside it the bytes the lanes ask for: per output pixel and iteration 2 x 9 table entries of 8 bytes (one
address per wave almost everywhere), then 4 C frame bytes, C output bytes and the valid byte.

    python3 tools/rows_probe.py --out profiles/rows_probe.txt"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import (rectify_frames, rotation_rows, smooth_rotations, warp_homography,  # noqa: E402
                                             warp_rows, _rodrigues)
from tools.rolling_probe import device_ms, flows, matrices  # noqa: E402

HBM = 6.3e12  # bytes per second that streaming kernels reach
READOUT, KNOTS, ITERS = 0.8, 17, 3


def tables(T, H, W, seed, readout, knots=KNOTS):
    """rotation_rows of a random walk of 0.02 rad per frame at f = 0.9 W, smoothed with radius 6: (T, Kn, 3, 3) float64"""
    rng = np.random.default_rng(seed)
    w = np.cumsum(rng.normal(0, 0.02 / np.sqrt(3), (T, 3)), 0)
    R = torch.from_numpy(np.stack([_rodrigues(x) for x in w]))
    return rotation_rows(R, smooth_rotations(R, 6), 0.9 * W, (H, W), readout, knots=knots)


class TorchRule:
    """papof_warp_rows_tensor in PyTorch operations of `dtype`; what does not depend on the frames' values or on the iterate --
    the table, the pixel grid -- is prepared once, outside the timed call"""

    def __init__(self, tab, H, W, iters, dtype):
        T, Kn = tab.shape[:2]
        dev = tab.device
        self.tab = tab.to(dtype).reshape(T, Kn, 9)
        y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=dtype), torch.arange(W, device=dev, dtype=dtype), indexing="ij")
        self.x, self.y = x.expand(T, H, W).reshape(T, -1), y.expand(T, H, W).reshape(T, -1)
        self.T, self.H, self.W, self.Kn, self.iters, self.dtype = T, H, W, Kn, iters, dtype
        self.g = (Kn - 1) / (H - 1)

    def __call__(self, v):
        """uint8 NHWC frames -> (uint8 NHWC video, valid)"""
        T, H, W = self.T, self.H, self.W
        x, r = self.x, self.y
        Y = r
        for _ in range(self.iters):
            Yc = torch.where(Y >= 0, Y.clamp(max=H - 1.0), torch.zeros_like(Y))
            s = Yc * self.g
            k = s.long().clamp(max=self.Kn - 2)
            f = (s - k.to(self.dtype))[..., None]
            ix = k[..., None].expand(T, H * W, 9)
            A, B = torch.gather(self.tab, 1, ix), torch.gather(self.tab, 1, ix + 1)
            m = A + f * (B - A)
            D = (m[..., 6] * x + m[..., 7] * r) + m[..., 8]
            X = ((m[..., 0] * x + m[..., 1] * r) + m[..., 2]) / D
            Y = ((m[..., 3] * x + m[..., 4] * r) + m[..., 5]) / D
        inside = ((D > 0) & (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)).reshape(T, H, W)
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (H - 1)) - 1], -1).reshape(T, H, W, 2)
        img = v.permute(0, 3, 1, 2).to(self.dtype)
        out = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)
        out = torch.where(inside[:, None], out, torch.zeros((), dtype=self.dtype, device=v.device))
        return out.round().clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1), inside


def warp_bytes(T, H, W, C, iters):
    """(the byte floor, the bytes the lanes ask for) of one warp_rows launch on uint8 frames and a float64 table"""
    px = H * W
    floor = T * px * (2 * C + 1)
    asked = iters * T * px * 2 * 9 * 8 + T * px * (4 * C + C + 1)
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

    say("The per-row projective warp on one %s device: readout %g, %d knots.  Device time between two events around one call, "
        "median of %d after warm-up; every version timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], READOUT, KNOTS, args.reps))
    for T, H, W, C in ((8, 1080, 1920, 3), (32, 135, 240, 3)):
        g = torch.Generator().manual_seed(T)
        v = torch.randint(0, 256, (T, H, W, C), generator=g, dtype=torch.uint8).to(dev)
        tab, one = tables(T, H, W, 7, READOUT).to(dev), tables(T, H, W, 7, 0.0).to(dev)
        fw, bw = (f.to(dev) for f in flows(T - 1, H, W, 8))
        M = matrices(T, H, W, 9).to(dev)
        say()
        say("%d uint8 NHWC frames of %d x %d x %d, float64 tables" % (T, W, H, C))
        res = {}
        k3 = device_ms(lambda: res.__setitem__("k", warp_rows(v, tab, iters=ITERS, layout="NHWC")), args.reps)
        k1 = device_ms(lambda: warp_rows(v, tab, iters=1, layout="NHWC"), args.reps)
        k8 = device_ms(lambda: warp_rows(v, tab, iters=8, layout="NHWC"), args.reps)
        ko = device_ms(lambda: res.__setitem__("o", warp_rows(v, one, layout="NHWC")), args.reps)
        wh = device_ms(lambda: res.__setitem__("h", warp_homography(v, one[:, 0], layout="NHWC")), args.reps)
        rs = device_ms(lambda: rectify_frames(v, fw, bw, READOUT, iters=ITERS, matrices=M, layout="NHWC"), args.reps)
        assert torch.equal(res["o"][0], res["h"][0]) and torch.equal(res["o"][1], res["h"][1])
        floor, asked = warp_bytes(T, H, W, C, ITERS)
        say("  warp_rows, %d knots, %d iterations (k_warp_rows)   %9.3f ms   %.3f ms per frame; %.2f x warp_homography" % (
            KNOTS, ITERS, k3, k3 / T, k3 / wh))
        say("  warp_rows, %d knots, 1 iteration                  %9.3f ms   8 iterations: %.3f ms" % (KNOTS, k1, k8))
        say("  warp_rows, 1 knot                                 %9.3f ms   %.2f x warp_homography, the same bytes" % (ko, ko / wh))
        say("  warp_homography (k_warp_projective: one gather)   %9.3f ms" % wh)
        say("  rectify_frames(matrices=M), %d iterations           %9.3f ms   (two flow fields read per iteration) %.2f x warp_rows" % (
            ITERS, rs, rs / k3))
        say("    byte floor: %.1f MB (the frames read once, the video and valid written once) = %.3f ms at %.1f TB/s: the kernel "
            "takes %.2f x that; the lanes ask for %.1f MB (%.2f TB/s)" % (
                floor / 1e6, floor / HBM * 1e3, HBM / 1e12, k3 / (floor / HBM * 1e3), asked / 1e6, asked / (k3 * 1e-3) / 1e12))
        for dtype in (torch.float64, torch.float32):
            rule = TorchRule(tab, H, W, ITERS, dtype)
            t = device_ms(lambda: res.__setitem__("t", rule(v)), args.reps)
            diff = (res["k"][0].int() - res["t"][0].int()).abs()
            say("  the rule in PyTorch operations, %-13s     %9.3f ms   %.1f x the kernel; %.5f of the output bytes agree, %.5f "
                "within 1; valid agrees on %.5f" % (str(dtype).split(".")[1], t, t / k3, float((diff == 0).double().mean()),
                                                    float((diff <= 1).double().mean()),
                                                    float((res["k"][1] == res["t"][1]).double().mean())))
            assert t > k3, "the kernel must beat the composition"
            del rule
        say("  valid: %.4f of the pixels" % float(res["k"][1].double().mean()))
        del res, v, fw, bw, tab, one
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
