#!/usr/bin/env python3
"""Cost of the high-bit-depth decoder-surface kernels on one device: tensors.ycc16_to_rgb (one k_ycc16_to_rgb /
k_ycc16_to_rgb_nv launch) and tensors.rgb_to_ycc16 (one k_rgb_to_ycc16 launch) against their byte floors, the 8-byte instance
of ycc16_to_rgb against the generic one on the same surface, the same integer rule composed of PyTorch operations (its bytes
must equal the kernels'), and the 8-bit call on an NV12 surface of the same frames in the same run.

Inputs: 8 P010 frames of 1920 x 1080 -- the committed 1080p frame rolled by 3 columns per frame, coded to 10 bits by
rgb_to_ycc16 itself -- to uint8 NHWC and to float32 NCHW, and back from float32 NCHW; 32 frames of 240 x 135 (the frame
decimated by 8); 8 NV12 frames of 1920 x 1080.  Pitches are multiples of 2048 bytes.  BT.709 limited, siting (left, center).
Byte floor: the planes and the frames moved once, over the 6.3 TB/s that streaming kernels reach on this device.  Times are
device times between two events around one call, the median of --reps (11) after warm-up, and per call of 20 calls back to
back; all versions in the same run.

    python3 tools/surface16_probe.py --out profiles/surface16_probe.txt
    python3 tools/surface16_probe.py --resources     # the kernels' registers from the build's assembly alone: needs no device"""
import argparse
import ctypes
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from surface_probe import HBM, SITING, h_taps, idx, resources, v_taps  # noqa: E402

PITCH = 2048  # bytes: every surface's rows are a multiple of this


def levels(words, d, shift):
    """the samples of a plane of words as int64"""
    return ((words.view(torch.int16).to(torch.int64) & 0xffff) >> shift) & ((1 << d) - 1)


def torch_forward(y, cb, cr, tab, d, shift, out_dtype, layout):
    """papof_ycc16_to_rgb_tensor's rule for siting (left, center) in PyTorch operations, 64-bit integers"""
    T, H, W = y.shape
    dev = y.device
    xa, xb, wxa, wxb = h_taps(W, SITING[0])
    ra, rb, wya, wyb = v_taps(H, SITING[1])
    xa, xb, ra, rb = idx(xa, dev), idx(xb, dev), idx(ra, dev), idx(rb, dev)
    wxa, wxb, wya, wyb = idx(wxa, dev).view(1, 1, W), idx(wxb, dev).view(1, 1, W), idx(wya, dev).view(1, H, 1), idx(wyb, dev).view(1, H, 1)

    def c32(c):
        c = levels(c, d, shift)
        rows = lambda r: wxa * c.index_select(1, r).index_select(2, xa) + wxb * c.index_select(1, r).index_select(2, xb)  # noqa: E731
        return wya * rows(ra) + wyb * rows(rb) - (1 << (d + 4))
    L = 32 * tab[1] * (levels(y, d, shift) - tab[0])
    U, V = c32(cb), c32(cr)
    N = torch.stack([L + tab[2] * V, L - tab[3] * U - tab[4] * V, L + tab[5] * U], -1 if layout == "NHWC" else 1)
    if out_dtype == torch.uint8:
        return ((N + (1 << (d + 10))) >> (d + 11)).clamp(0, 255).to(torch.uint8)
    one = tab[6] << (d + 11)
    return (N.clamp(0, one).to(torch.float64) / float(one)).to(out_dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--resources", action="store_true", help="print the kernels' registers from the build and stop")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
        return
    from papteam_opticalflow_amd import capi, tensors
    from papteam_opticalflow_amd.tensors import (new_nv12, new_p010, rgb_to_ycc, rgb_to_ycc16, ycc16_to_rgb, ycc_tables16,
                                                 ycc_to_rgb)
    dev = torch.device("cuda", 0)
    rep = io.StringIO()
    D, SHIFT = 10, 6

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    def device_ms(fn):
        fn()
        fn()
        torch.cuda.synchronize()
        dt = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            dt.append(a.elapsed_time(b))
        return float(np.median(dt))

    def burst_ms(fn, n=20):
        def many():
            for _ in range(n):
                fn()
        return device_ms(many) / n

    def launch_forward(planes, out, layout, tab):
        d = [tensors._plane_struct16(p) for p in planes] + [tensors._struct(out, *tensors.descriptor(out, layout)[1:])]
        refs = [ctypes.byref(x) for x in d]
        T, H, W = planes[0].shape
        tensors._launch(dev, "papof_ycc16_to_rgb_tensor", T, H, W, refs[0], refs[1], refs[2], D, SHIFT, 2, 0, 0, 0,
                        (ctypes.c_int * 7)(*tab), refs[3])
        return capi.load().papof_ycc16_to_rgb_fast(W, *refs)

    def floor_line(what, ms, nbytes):
        return "%s: %.2f MB = %.4f ms at %.1f TB/s; back to back the call takes %.1f x that (%.3f TB/s of distinct bytes)" % (
            what, nbytes / 1e6, nbytes / HBM * 1e3, HBM / 1e12, ms / (nbytes / HBM * 1e3), nbytes / (ms * 1e-3) / 1e12)

    import cases
    say("High-bit-depth decoder surfaces on one %s device.  Depth 10 in the high bits (P010), BT.709 limited, siting (left, "
        "center).  Device time between two events around one call, median of %d after warm-up; 'back to back': per call of 20 "
        "calls between two events.  Every version timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    img = cases.load_frame_u8("1920", 1)
    for T, dec in ((8, 1), (32, 8)):
        src = img[::dec, ::dec]
        frames = torch.from_numpy(np.stack([np.ascontiguousarray(np.roll(src, -3 * k, axis=1)) for k in range(T)])).to(dev)
        H, W = frames.shape[1:3]
        surface, planes = new_p010(T, H, W, dev, pitch=-(-2 * W // PITCH) * PITCH)
        rgb_to_ycc16(frames, depth=D, out=planes)
        pbytes = 2 * sum(p.numel() for p in planes)
        say()
        say("%d P010 frames of %d x %d at a pitch of %d bytes (%.2f MB of planes)" % (T, W, H, 2 * surface.shape[2], pbytes / 1e6))
        for out_dtype, layout in ((torch.uint8, "NHWC"), (torch.float32, "NCHW")):
            tab = ycc_tables16("bt709", "limited", D, peak=255 if out_dtype == torch.uint8 else None)
            res = {}
            fw = lambda: res.__setitem__("k", ycc16_to_rgb(*planes, depth=D, layout=layout, out_dtype=out_dtype))  # noqa: E731
            k, kb = device_ms(fw), burst_ms(fw)
            floor = pbytes + res["k"].numel() * res["k"].element_size()
            say("  ycc16_to_rgb -> %s %s" % (str(out_dtype).replace("torch.", ""), layout))
            say("    one call                                 %9.3f ms   %.4f ms per frame" % (k, k / T))
            say("    per call, 20 calls back to back          %9.3f ms   %.4f ms per frame" % (kb, kb / T))
            say("    " + floor_line("byte floor, planes + frames once", kb, floor))
            shape = res["k"].shape
            aligned = torch.empty(shape, dtype=out_dtype, device=dev)
            off = torch.empty(res["k"].numel() + 1, dtype=out_dtype, device=dev)[1:].view(shape)  # one element further
            which = launch_forward(planes, aligned, layout, tab)
            fa = burst_ms(lambda: launch_forward(planes, aligned, layout, tab))
            gen_which = launch_forward(planes, off, layout, tab)
            ga = burst_ms(lambda: launch_forward(planes, off, layout, tab))
            say("    instances on this surface, back to back: 8-byte instance (chosen: %d) %.3f ms, generic instance (output moved "
                "off its alignment; 8-byte instance chosen: %d) %.3f ms = %.2f x; the same bytes: %s" % (
                    which, fa, gen_which, ga, ga / fa, torch.equal(aligned, off) and torch.equal(aligned, res["k"])))
            t = device_ms(lambda: res.__setitem__("t", torch_forward(*planes, tab, D, SHIFT, out_dtype, layout)))
            say("    the rule in PyTorch operations, int64    %9.3f ms   %.1f x the kernel; the same bytes: %s" % (
                t, t / k, torch.equal(res["k"].view(torch.uint8), res["t"].contiguous().view(torch.uint8))))
        src_frames = res["k"]  # float32 NCHW
        rv = lambda: rgb_to_ycc16(src_frames, depth=D, layout="NCHW", out=planes)  # noqa: E731
        r, rb = device_ms(rv), burst_ms(rv)
        say("  rgb_to_ycc16 <- float32 NCHW, into the surface")
        say("    one call                                 %9.3f ms   %.4f ms per frame" % (r, r / T))
        say("    per call, 20 calls back to back          %9.3f ms   %.4f ms per frame" % (rb, rb / T))
        say("    " + floor_line("byte floor, frames + planes once", rb, pbytes + src_frames.numel() * 4))
        if dec == 1:
            s8, p8 = new_nv12(T, H, W, dev, pitch=-(-W // PITCH) * PITCH)
            rgb_to_ycc(frames, out=p8)
            b8 = sum(p.numel() for p in p8)
            say()
            say("%d NV12 frames of %d x %d at a pitch of %d bytes (%.2f MB of planes): the 8-bit call, in this run" % (
                T, W, H, s8.shape[2], b8 / 1e6))
            for out_dtype, layout in ((torch.uint8, "NHWC"), (torch.float32, "NCHW")):
                f8 = lambda: res.__setitem__("e", ycc_to_rgb(*p8, layout=layout, out_dtype=out_dtype))  # noqa: E731
                k8, kb8 = device_ms(f8), burst_ms(f8)
                say("  ycc_to_rgb -> %s %s: one call %.3f ms, back to back %.3f ms" % (str(out_dtype).replace("torch.", ""), layout, k8, kb8))
                say("    " + floor_line("byte floor, planes + frames once", kb8, b8 + res["e"].numel() * res["e"].element_size()))
    say()
    for line in resources():
        say(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
