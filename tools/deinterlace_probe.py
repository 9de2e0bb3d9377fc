#!/usr/bin/env python3
"""Cost of motion-compensated deinterlacing on one device: tensors.deinterlace_fields and tensors.bob_fields (one
k_deinterlace launch each, modes 1 and 0) against the same rule composed of PyTorch operations, the kernel's ratio to its
byte floor, the two ways of estimating the field flows, and flow estimation's share of one tensors.deinterlace_video call.

Kernels: eight fields of 540 x 1920 x 3 uint8 NHWC -- the committed 1080p frame panning by 3 px per field --, float64
flows: smooth random fields of a few pixels, bw = -fw + noise.  The PyTorch composition is the rule in float64: the cubic
from four row gathers, two grid_samples (bilinear, border padding, align_corners=True: positions agree with the kernel's
rule inside the image, the arithmetic is not bit for bit the kernel's), the phase and agreement weights, the blend, and
the weave into uint8 frames.  Times are device times between two events around one call, the median of --reps (11) after
warm-up, both versions in the same run; the share of output bytes that agree is printed.

Byte floor: per made pixel the four own taps, the eight neighbour taps (four on an end frame), the two flow vectors (one on
an end frame), the two output rows and the confidence, over the 6.3 TB/s that streaming kernels reach on this device.  The
bytes that are distinct -- every field byte once, however many taps read it -- are printed beside it.

Flows: tensors.field_flows (flow_pairs_fb on (fields[:-2], fields[2:]): independent pairs, each inner field's pyramid built
twice) against two flow_video_fb calls on the even and the odd fields (each pyramid built once), 4 levels, median of 3.

    python3 tools/deinterlace_probe.py --out profiles/deinterlace_probe.txt"""
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
from papteam_opticalflow_amd.tensors import (bob_fields, deinterlace_fields, deinterlace_video, field_flows,  # noqa: E402
                                             flow_video_fb)

SIGMA = tensors.DEINT_SIGMA
HBM = 6.3e12  # bytes per second that streaming kernels reach


def flows(P, H, W, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    fw = torch.randn(P, 2, H // 16 + 1, W // 16 + 1, generator=g, dtype=torch.float64) * amp
    fw = torch.nn.functional.interpolate(fw, size=(H, W), mode="bilinear", align_corners=False)
    bw = -fw + 0.1 * torch.randn(P, 2, H, W, generator=g, dtype=torch.float64)
    return fw.contiguous(), bw.contiguous()


def fields_1080p(T=8, step=3):
    import cases
    img = cases.load_frame_u8("1920", 1)
    return torch.from_numpy(np.stack([np.roll(img, -step * k, axis=1)[k & 1::2] for k in range(T)]))


def torch_cubic(I, first):
    """the bob's made lines (T, C, Hf, W) of I (T, C, Hf, W) float64"""
    T, _, Hf, _ = I.shape
    s = torch.empty_like(I)
    r = torch.arange(Hf, device=I.device)
    for par in (0, 1):  # the frames whose made lines have parity pm
        ts = [t for t in range(T) if 1 - ((t + first) & 1) == par]
        J = I[ts]
        a1, b1 = J[:, :, (r - 1 + par).clamp(0, Hf - 1)], J[:, :, (r + par).clamp(0, Hf - 1)]
        a3, b3 = J[:, :, (r - 2 + par).clamp(0, Hf - 1)], J[:, :, (r + 1 + par).clamp(0, Hf - 1)]
        s[ts] = (9.0 * (a1 + b1) - (a3 + b3)) * 0.0625
    return s


def weave(v, made, first):
    """kept lines of the uint8 fields v (T, Hf, W, C) and made lines (T, C, Hf, W) float64 as uint8 frames (T, 2 Hf, W, C)"""
    T, Hf, W, C = v.shape
    out = torch.empty((T, 2 * Hf, W, C), dtype=torch.uint8, device=v.device)
    m = (made.permute(0, 2, 3, 1) * 255.0).round().clamp(0.0, 255.0).to(torch.uint8)
    for t in range(T):
        p = (t + first) & 1
        out[t, p::2] = v[t]
        out[t, 1 - p::2] = m[t]
    return out


def torch_bob(v, first=0):
    return weave(v, torch_cubic(v.permute(0, 3, 1, 2).double() / 255.0, first), first)


def torch_deinterlace(v, fw, bw, first=0, sigma=SIGMA):
    """the rule of papof_deinterlace_tensor, mode 1, with grid_sample and elementwise operations: (video, confidence)"""
    T, Hf, W, C = v.shape
    I = v.permute(0, 3, 1, 2).double() / 255.0
    s = torch_cubic(I, first)
    y, x = torch.meshgrid(torch.arange(Hf, device=v.device, dtype=torch.float64),
                          torch.arange(W, device=v.device, dtype=torch.float64), indexing="ij")

    def sample(img, X, Y):
        grid = torch.stack([X * (2.0 / (W - 1)) - 1, Y * (2.0 / (Hf - 1)) - 1], -1)
        return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)

    def phase(X, Y):
        inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= Hf - 1)
        return torch.where(inside, 1.0 - 2.0 * (Y - Y.round()).abs(), torch.zeros_like(Y))

    q = torch.zeros((T, Hf, W), dtype=torch.float64, device=v.device)
    m = torch.zeros_like(I)
    u, w, bu, bv = fw[:, 0], fw[:, 1], bw[:, 0], bw[:, 1]
    X0, Y0 = x + (0.25 * bu - 0.25 * u), y + (0.25 * bv - 0.25 * w)
    X1, Y1 = x + (0.25 * u - 0.25 * bu), y + (0.25 * w - 0.25 * bv)
    c0, c1 = phase(X0, Y0), phase(X1, Y1)
    g0, g1 = sample(I[:-2], X0, Y0), sample(I[2:], X1, Y1)
    both, use0, use1 = (c0 > 0) & (c1 > 0), c0 > 0, c1 > 0
    D = ((g0 - g1) ** 2).mean(1)
    q[1:-1] = torch.where(both, torch.maximum(c0, c1) / (1.0 + D / (sigma * sigma)),
                          torch.where(use0, 0.5 * c0, torch.where(use1, 0.5 * c1, torch.zeros_like(c0))))
    den = torch.where(both, c0 + c1, torch.ones_like(c0))
    m[1:-1] = torch.where(both[:, None], (c0[:, None] * g0 + c1[:, None] * g1) / den[:, None],
                          torch.where(use0[:, None], g0, g1))
    for t, src, f in ((0, 1, fw[1]), (T - 1, T - 2, bw[T - 4])):  # the end frames: one sample
        X, Y = x + 0.5 * f[0], y + 0.5 * f[1]
        c = phase(X, Y)
        q[t] = 0.5 * c
        m[t] = sample(I[src:src + 1], X[None], Y[None])[0]
    qq = q[:, None]
    made = torch.where(qq != 0, (1.0 - qq) * s + qq * torch.nan_to_num(m), s)
    return weave(v, made, first), q


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


def floor_bytes(T, Hf, W, C, mode):
    """(bytes the lanes ask for, distinct bytes) of one launch on uint8 fields, float64 flows and confidence, uint8 video"""
    px = Hf * W
    if not mode:
        return T * px * (4 * C + 2 * C), T * px * (C + 2 * C)
    asked = (T - 2) * px * (4 * C + 8 * C + 2 * 16 + 2 * C + 8) + 2 * px * (4 * C + 4 * C + 16 + 2 * C + 8)
    return asked, T * px * (C + 2 * C + 8) + (T - 2) * px * 32


def even_odd_flows(v, levels):
    """the field flows from two flow_video_fb calls, on the even and on the odd fields: (flow_fw, flow_bw) (T - 2, 2, Hf, W)"""
    T = v.shape[0]
    e = flow_video_fb(v[0::2], levels, layout="NHWC", consistency=None)
    o = flow_video_fb(v[1::2], levels, layout="NHWC", consistency=None)
    fw = torch.empty((T - 2,) + tuple(e.flow_fw.shape[1:]), dtype=torch.float64, device=v.device)
    bw = torch.empty_like(fw)
    fw[0::2], fw[1::2], bw[0::2], bw[1::2] = e.flow_fw, o.flow_fw, e.flow_bw, o.flow_bw
    return fw, bw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--flow-reps", type=int, default=3)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Motion-compensated deinterlacing on one %s device.  Device time between two events around one call, median of %d "
        "after warm-up; the kernel and the PyTorch composition timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    v = fields_1080p().to(dev)
    T, Hf, W, C = v.shape
    fw, bw = (f.to(dev) for f in flows(T - 2, Hf, W, 8))
    say()
    say("kernel: %d uint8 NHWC fields of %d x %d x %d, float64 flows, sigma %g -> %d frames of %d x %d" % (
        T, W, Hf, C, SIGMA, T, W, 2 * Hf))
    res = {}
    for mode, name, kernel, composed in (
            (1, "deinterlace_fields (k_deinterlace, mode 1)", lambda: deinterlace_fields(v, fw, bw, layout="NHWC").video,
             lambda: torch_deinterlace(v, fw, bw)[0]),
            (0, "bob_fields (k_deinterlace, mode 0)", lambda: bob_fields(v, layout="NHWC"), lambda: torch_bob(v))):
        k = device_ms(lambda: res.__setitem__("k", kernel()), args.reps)
        t = device_ms(lambda: res.__setitem__("t", composed()), args.reps)
        asked, distinct = floor_bytes(T, Hf, W, C, mode)
        diff = (res["k"].int() - res["t"].int()).abs()
        say("  %-44s %9.3f ms   %.3f ms per frame" % (name, k, k / T))
        say("    byte floor: %.1f MB asked for by the lanes = %.3f ms at %.1f TB/s: the kernel takes %.2f x that (%.2f TB/s); "
            "%.1f MB distinct = %.3f ms" % (asked / 1e6, asked / HBM * 1e3, HBM / 1e12, k / (asked / HBM * 1e3),
                                            asked / (k * 1e-3) / 1e12, distinct / 1e6, distinct / HBM * 1e3))
        say("    the rule in PyTorch operations, float64     %9.3f ms   %.1f x the kernel; %.5f of the output bytes agree, "
            "%.5f within 1" % (t, t / k, float((diff == 0).double().mean()), float((diff <= 1).double().mean())))
    q = deinterlace_fields(v, fw, bw, layout="NHWC").confidence
    say("  confidence on these flows: mean %.3f, %.4f of the made pixels are the cubic alone" % (
        float(q.mean()), float((q == 0).double().mean())))
    del res, fw, bw, q

    say()
    say("field flows of those fields, %d levels, median of %d:" % (args.levels, args.flow_reps))
    out = {}
    a = device_ms(lambda: out.__setitem__("a", field_flows(v, args.levels, layout="NHWC")), args.flow_reps)
    b = device_ms(lambda: out.__setitem__("b", even_odd_flows(v, args.levels)), args.flow_reps)
    same = torch.equal(out["a"].flow_fw, out["b"][0]) and torch.equal(out["a"].flow_bw, out["b"][1])
    say("  field_flows: flow_pairs_fb(fields[:-2], fields[2:])         %9.2f ms" % a)
    say("  two flow_video_fb calls, even and odd fields, interleaved   %9.2f ms   %.3f x field_flows; the same bits: %s" % (
        b, b / a, same))
    del out
    total = device_ms(lambda: deinterlace_video(v, args.levels, layout="NHWC"), args.flow_reps)
    say("deinterlace_video, %d levels: %.2f ms in all; flow estimation is %.1f %% of it" % (args.levels, total, 100.0 * a / total))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
