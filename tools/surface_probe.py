#!/usr/bin/env python3
"""Cost of the decoder-surface kernels on one device: tensors.ycc_to_rgb (one k_ycc_to_rgb / k_ycc_to_rgb_nv launch) and
tensors.rgb_to_ycc (one k_rgb_to_ycc launch) against their byte floors, against the same integer rules composed of PyTorch
operations (index gathers, integer products, shifts, clamps -- their bytes must equal the kernels'), and against the usual
float composition (F.interpolate(bilinear) of the chroma plus a matrix product; avg_pool2d on the way out), whose result
differs by its own siting and rounding; and the dword instance of ycc_to_rgb against the generic one on the same surface.

Inputs: 8 NV12 frames of 1920 x 1080 at a pitch of 2048 -- the committed 1080p frame rolled by 3 columns per frame, coded by
rgb_to_ycc itself -- to uint8 NHWC and to float32 NCHW, and back; 32 frames of 240 x 135 (the frame decimated by 8) at a
pitch of 256.  BT.709 limited, siting (left, center); the float composition is compared at (center, center), which is what
F.interpolate's bilinear is.  Byte floor: the planes and the frames read or written once, over the 6.3 TB/s that streaming
kernels reach on this device.  Times are device times between two events around one call, the median of --reps (11) after
warm-up, and per call of 20 calls back to back; all versions in the same run.

    python3 tools/surface_probe.py --out profiles/surface_probe.txt
    python3 tools/surface_probe.py --resources     # the kernels' registers from the build's assembly alone: needs no device"""
import argparse
import ctypes
import glob
import io
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM = 6.3e12  # bytes per second that streaming kernels reach
SITING = ("left", "center")


def resources():
    """lines with the VGPRs, SGPRs, scratch and waves per SIMD of surface.hip's kernels, from the assembly the build keeps"""
    found = glob.glob(os.path.join(ROOT, "papteam_opticalflow_amd", "csrc", ".build", "surface", "*gfx950.s"))
    if not found:
        return ["registers: the build's assembly (csrc/.build/surface) is not here"]
    text = open(found[0]).read()
    out = []
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        f = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", m.group(2))}
        name = re.sub(r"^_ZN5papof12_GLOBAL__N_1\d+", "", m.group(1))
        name = re.sub(r"EvNS0_.*$", "", name).replace("ILi", "<").replace("ELb", ", ").replace("ELi", ", ").replace("EE", ">")
        waves = min(8, 512 // (-(-max(f["vgpr_count"], 1) // 8) * 8))
        out.append("  %-28s %3d VGPRs %3d SGPRs, scratch %d bytes, spills %d: %d waves per SIMD" % (
            name, f["vgpr_count"], f["sgpr_count"], f["private_segment_fixed_size"], f["vgpr_spill_count"], waves))
    return ["registers from the build (template arguments: dtype code 0 uint8 / 1 float32 / 2 float64[, NHWC]):"] + sorted(out)


def h_taps(W, siting):
    x = np.arange(W)
    k, odd = x >> 1, (x & 1) == 1
    if siting == "left":
        a, b, wa = k, k + odd, np.where(odd, 2, 4)
    else:
        a, b, wa = np.where(odd, k, k - 1), np.where(odd, k + 1, k), np.where(odd, 3, 1)
    Wc = -(-W // 2)
    return np.clip(a, 0, Wc - 1), np.clip(b, 0, Wc - 1), wa, 4 - wa


def v_taps(H, siting):
    y = np.arange(H)
    j, odd = y >> 1, (y & 1) == 1
    if siting == "center":
        a, b, wa = np.where(odd, j, j - 1), np.where(odd, j + 1, j), np.where(odd, 6, 2)
    else:
        a, b, wa = j, j + odd, np.where(odd, 4, 8)
    Hc = -(-H // 2)
    return np.clip(a, 0, Hc - 1), np.clip(b, 0, Hc - 1), wa, 8 - wa


def idx(a, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dev)


def w32(a, shape, dev):
    return torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev).reshape(shape)


def torch_forward(y, cb, cr, tab, siting, out_dtype, layout):
    """papof_ycc_to_rgb_tensor's rule in PyTorch operations"""
    T, H, W = y.shape
    dev = y.device
    xa, xb, wxa, wxb = h_taps(W, siting[0])
    ra, rb, wya, wyb = v_taps(H, siting[1])
    xa, xb, ra, rb = idx(xa, dev), idx(xb, dev), idx(ra, dev), idx(rb, dev)
    wxa, wxb, wya, wyb = w32(wxa, (1, 1, W), dev), w32(wxb, (1, 1, W), dev), w32(wya, (1, H, 1), dev), w32(wyb, (1, H, 1), dev)

    def c32(c):
        c = c.to(torch.int32)
        rows = lambda r: wxa * c.index_select(1, r).index_select(2, xa) + wxb * c.index_select(1, r).index_select(2, xb)  # noqa: E731
        return wya * rows(ra) + wyb * rows(rb) - 4096
    L = 32 * tab[1] * (y.to(torch.int32) - tab[0])
    U, V = c32(cb), c32(cr)
    N = torch.stack([L + tab[2] * V, L - tab[3] * U - tab[4] * V, L + tab[5] * U], -1 if layout == "NHWC" else 1)
    if out_dtype == torch.uint8:
        return ((N + (1 << 18)) >> 19).clamp(0, 255).to(torch.uint8)
    return (N.clamp(0, 255 << 19).to(torch.float64) / float(255 << 19)).to(out_dtype)


def matrix709(dev):
    """(Y - 16, Cb - 128, Cr - 128) to RGB levels, BT.709 limited, float32"""
    return torch.tensor([[255 / 219, 0.0, 2 * (1 - 0.2126) * 255 / 224],
                         [255 / 219, -2 * 0.0722 * (1 - 0.0722) / 0.7152 * 255 / 224, -2 * 0.2126 * (1 - 0.2126) / 0.7152 * 255 / 224],
                         [255 / 219, 2 * (1 - 0.0722) * 255 / 224, 0.0]], dtype=torch.float32, device=dev)


def float_forward(y, cb, cr, out_dtype, layout):
    """the usual composition: bilinear chroma (F.interpolate, align_corners=False: siting (center, center)), a matrix product"""
    T, H, W = y.shape
    c = F.interpolate(torch.stack([cb, cr], 1).float(), scale_factor=2, mode="bilinear", align_corners=False)[:, :, :H, :W]
    ycc = torch.cat([y[:, None].float() - 16.0, c - 128.0], 1)
    rgb = torch.einsum("oc,tchw->tohw" if layout == "NCHW" else "oc,tchw->thwo", matrix709(y.device), ycc)
    return rgb.round().clamp(0, 255).to(torch.uint8) if out_dtype == torch.uint8 else (rgb / 255.0).clamp(0, 1).to(out_dtype)


def torch_reverse(frames, rtab, layout):
    """papof_rgb_to_ycc_tensor's rule for siting (left, center) in PyTorch operations, 64-bit integers"""
    f = frames if layout == "NHWC" else frames.permute(0, 2, 3, 1)
    T, H, W, _ = f.shape
    dev = f.device
    if f.dtype == torch.uint8:
        q = f.to(torch.int64) * 257
    else:
        q = torch.nan_to_num(torch.round(65535.0 * f.to(torch.float64)), nan=0.0).clamp(0, 65535).to(torch.int64)
    R, G, B = q[..., 0], q[..., 1], q[..., 2]
    D = 257 << 14
    y = ((rtab[1] * R + rtab[2] * G + rtab[3] * B + rtab[0] * D + D // 2) // D).clamp(0, 255).to(torch.uint8)
    k, j = 2 * np.arange(-(-W // 2)), 2 * np.arange(-(-H // 2))
    cols = [idx(np.clip(k + d, 0, W - 1), dev) for d in (-1, 0, 1)]
    rows = [idx(np.clip(j + d, 0, H - 1), dev) for d in (0, 1)]
    out = []
    for N in ((rtab[4] + rtab[5]) * B - rtab[4] * R - rtab[5] * G, (rtab[6] + rtab[7]) * R - rtab[6] * G - rtab[7] * B):
        Nh = N.index_select(2, cols[0]) + 2 * N.index_select(2, cols[1]) + N.index_select(2, cols[2])
        S = 2 * Nh.index_select(1, rows[0]) + 2 * Nh.index_select(1, rows[1])
        out.append(torch.div(S + 128 * 16 * D + 8 * D, 16 * D, rounding_mode="floor").clamp(0, 255).to(torch.uint8))
    return y, out[0], out[1]


def float_reverse(frames, layout):
    """the usual composition on the way out: a matrix product, avg_pool2d of the chroma (siting (center, center))"""
    f = (frames if layout == "NCHW" else frames.permute(0, 3, 1, 2)).float()
    f = f if frames.dtype == torch.uint8 else 255.0 * f
    ycc = torch.einsum("oc,tchw->tohw", torch.linalg.inv(matrix709(f.device).double()).float(), f)
    H, W = ycc.shape[2:]
    c = F.avg_pool2d(F.pad(ycc[:, 1:], (0, W % 2, 0, H % 2), mode="replicate"), 2) + 128.0
    u8 = lambda t: t.round().clamp(0, 255).to(torch.uint8)  # noqa: E731
    return u8(ycc[:, 0] + 16.0), u8(c[:, 0]), u8(c[:, 1])


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
    from papteam_opticalflow_amd.tensors import new_nv12, rgb_to_ycc, ycc_tables, ycc_to_rgb
    dev = torch.device("cuda", 0)
    rep = io.StringIO()
    tab, rtab = ycc_tables("bt709", "limited"), ycc_tables("bt709", "limited", reverse=True)

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

    def launch_forward(planes, out, layout):
        d = [tensors._plane_struct(p) for p in planes] + [tensors._struct(out, *tensors.descriptor(out, layout)[1:])]
        refs = [ctypes.byref(x) for x in d]
        T, H, W = planes[0].shape
        tensors._launch(dev, "papof_ycc_to_rgb_tensor", T, H, W, refs[0], refs[1], refs[2], 2, 0, 0, 0, (ctypes.c_int * 6)(*tab), refs[3])
        return capi.load().papof_ycc_to_rgb_fast(W, *refs)

    import cases
    say("Decoder surfaces on one %s device.  BT.709 limited, siting (left, center).  Device time between two events around "
        "one call, median of %d after warm-up; 'back to back': per call of 20 calls between two events.  Every version timed in "
        "the same run." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    img = cases.load_frame_u8("1920", 1)
    for T, dec in ((8, 1), (32, 8)):
        src = img[::dec, ::dec]
        frames = torch.from_numpy(np.stack([np.ascontiguousarray(np.roll(src, -3 * k, axis=1)) for k in range(T)])).to(dev)
        H, W = frames.shape[1:3]
        surface, planes = new_nv12(T, H, W, dev)
        rgb_to_ycc(frames, out=planes)
        pbytes = sum(p.numel() for p in planes)
        say()
        say("%d NV12 frames of %d x %d at a pitch of %d (%.2f MB of planes)" % (T, W, H, surface.shape[2], pbytes / 1e6))
        for out_dtype, layout in ((torch.uint8, "NHWC"), (torch.float32, "NCHW")):
            res = {}
            fw = lambda: res.__setitem__("k", ycc_to_rgb(*planes, layout=layout, out_dtype=out_dtype))  # noqa: E731
            k, kb = device_ms(fw), burst_ms(fw)
            floor = pbytes + res["k"].numel() * res["k"].element_size()
            say("  ycc_to_rgb -> %s %s" % (str(out_dtype).replace("torch.", ""), layout))
            say("    one call                                 %9.3f ms   %.4f ms per frame" % (k, k / T))
            say("    per call, 20 calls back to back          %9.3f ms   %.4f ms per frame" % (kb, kb / T))
            say("    byte floor: planes + frames once = %.2f MB = %.4f ms at %.1f TB/s: back to back the call takes %.1f x that "
                "(%.3f TB/s of distinct bytes)" % (floor / 1e6, floor / HBM * 1e3, HBM / 1e12, kb / (floor / HBM * 1e3),
                                                   floor / (kb * 1e-3) / 1e12))
            # the generic instance on the same surface: an output that starts off a dword (uint8) or off 16 bytes (float32)
            shape = res["k"].shape
            aligned = torch.empty(shape, dtype=out_dtype, device=dev)
            off = torch.empty(res["k"].numel() + 1, dtype=out_dtype, device=dev)[1:].view(shape)  # one element further
            which = launch_forward(planes, aligned, layout)
            fa = burst_ms(lambda: launch_forward(planes, aligned, layout))
            gen_which = launch_forward(planes, off, layout)
            ga = burst_ms(lambda: launch_forward(planes, off, layout))
            say("    instances on this surface, back to back: dword instance (chosen: %d) %.3f ms, generic instance (output moved "
                "off its alignment; dword instance chosen: %d) %.3f ms = %.2f x; the same bytes: %s" % (
                    which, fa, gen_which, ga, ga / fa, torch.equal(aligned, off) and torch.equal(aligned, res["k"])))
            t = device_ms(lambda: res.__setitem__("t", torch_forward(*planes, tab, SITING, out_dtype, layout)))
            say("    the rule in PyTorch operations, int32    %9.3f ms   %.1f x the kernel; the same bytes: %s" % (
                t, t / k, torch.equal(res["k"].view(torch.uint8), res["t"].contiguous().view(torch.uint8))))
            fl = device_ms(lambda: res.__setitem__("f", float_forward(*planes, out_dtype, layout)))
            cc = ycc_to_rgb(*planes, siting=("center", "center"), layout=layout, out_dtype=out_dtype)
            scale = 1.0 if out_dtype == torch.uint8 else 255.0
            diff = (cc.double() - res["f"].double()).abs() * scale
            say("    F.interpolate(bilinear) + matrix, float32 %8.3f ms   %.1f x the kernel; against the kernel at (center, center): "
                "max %.3f levels, %.2f %% of elements differ by more than half a level" % (
                    fl, fl / k, float(diff.max()), 100.0 * float((diff > 0.5).double().mean())))
            # and back
            src_frames = res["k"]
            back = {}
            rv = lambda: back.__setitem__("k", rgb_to_ycc(src_frames, layout=layout, out=planes))  # noqa: E731
            r, rb = device_ms(rv), burst_ms(rv)
            say("  rgb_to_ycc <- %s %s, into the surface" % (str(out_dtype).replace("torch.", ""), layout))
            say("    one call                                 %9.3f ms   %.4f ms per frame" % (r, r / T))
            say("    per call, 20 calls back to back          %9.3f ms   %.4f ms per frame   %.1f x the byte floor (%.3f TB/s of "
                "distinct bytes)" % (rb, rb / T, rb / (floor / HBM * 1e3), floor / (rb * 1e-3) / 1e12))
            t = device_ms(lambda: back.__setitem__("t", torch_reverse(src_frames, rtab, layout)))
            say("    the rule in PyTorch operations, int64    %9.3f ms   %.1f x the kernel; the same bytes: %s" % (
                t, t / r, all(torch.equal(a, b) for a, b in zip(back["k"], back["t"]))))
            fl = device_ms(lambda: back.__setitem__("f", float_reverse(src_frames, layout)))
            cc = rgb_to_ycc(src_frames, siting=("center", "center"), layout=layout)
            diff = torch.cat([(a.double() - b.double()).abs().reshape(-1) for a, b in zip(cc, back["f"])])
            say("    matrix + avg_pool2d, float32             %9.3f ms   %.1f x the kernel; against the kernel at (center, center): "
                "max %.0f levels, %.2f %% of samples differ" % (fl, fl / r, float(diff.max()), 100.0 * float((diff > 0).double().mean())))
            rgb_to_ycc(frames, out=planes)  # the surface as it was for the next case
    say()
    for line in resources():
        say(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
