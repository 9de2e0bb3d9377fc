#!/usr/bin/env python3
"""Cost of inverse telecine's two kernels on one device: tensors.field_metrics (one k_field_metrics launch) against the same
rule composed of PyTorch operations and against its byte floor, and tensors.weave_fields (one k_weave_fields launch) against
two index_selects with strided copies.

field_metrics: 16 fields of 540 x 1920 x 3 uint8 NHWC -- the committed 1080p frame in 3:2 pulldown, panning by 3 px per
film frame -- and 64 fields of 68 x 240 x 3 (the frame decimated by 8).  The PyTorch composition is the rule in int32: the
quantisation, slices for the lines above and below, minimum / comparisons for the comb measure, the maxima over the
channels, and a padded view + sum per cell; its counts must equal the kernel's.  Byte floor: every field byte read once plus
the counts, over the 6.3 TB/s that streaming kernels reach on this device.  Times are device times between two events around
one call, the median of --reps (11) after warm-up, both versions in the same run.

    python3 tools/telecine_probe.py --out profiles/telecine_probe.txt"""
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
from papteam_opticalflow_amd.tensors import field_metrics, match_fields, weave_fields  # noqa: E402

HBM = 6.3e12  # bytes per second that streaming kernels reach


def film_fields(T, step=3, decimate=1):
    """T fields of the committed frame in 3:2 pulldown (first 0), instant k rolled by step k columns"""
    import cases
    img = cases.load_frame_u8("1920", 1)[::decimate, ::decimate]
    if img.shape[0] % 2:  # (135 rows at 8: the last one twice, fields of 68)
        img = np.concatenate([img, img[-1:]])
    seq = [k for i in range(T) for k in [i] * (2 if i % 2 == 0 else 3)][:T]
    return torch.from_numpy(np.stack([np.ascontiguousarray(np.roll(img, -step * k, axis=1)[i & 1::2]) for i, k in enumerate(seq)]))


def torch_metrics(v, first, cell_rows, comb_q, diff_q):
    """the rule of papof_field_metrics_tensor on uint8 fields v (T, Hf, W, C) in PyTorch operations: counts (T, 3, Gy, Gx) int32"""
    T, Hf, W, C = v.shape
    Q = v.to(torch.int32) * 257
    Gy, Gx = -(-Hf // cell_rows), -(-W // 64)
    out = torch.zeros((T, 3, Gy, Gx), dtype=torch.int32, device=v.device)

    def m(b, a, c):
        da, dc = a - b, c - b
        outside = ((da > 0) & (dc > 0)) | ((da < 0) & (dc < 0))
        return torch.where(outside, torch.minimum(da.abs(), dc.abs()), torch.zeros_like(da)).amax(-1)

    for par in (0, 1):
        ts = torch.tensor([t for t in range(1, T - 1) if (t + first) & 1 == par], device=v.device)
        if len(ts) == 0:
            continue
        rows = slice(1, Hf) if par == 0 else slice(0, Hf - 1)
        up, dn = (slice(0, Hf - 1), slice(1, Hf))
        b = Q[ts][:, rows]
        am, cm, ap, cp = Q[ts - 1][:, up], Q[ts - 1][:, dn], Q[ts + 1][:, up], Q[ts + 1][:, dn]
        Mm, Mp = m(b, am, cm), m(b, ap, cp)
        nd = torch.maximum((ap - am).abs(), (cp - cm).abs()).amax(-1)
        hits = torch.stack((Mp > Mm + comb_q, Mm > Mp + comb_q, nd > diff_q), 1)  # (n, 3, Hf - 1, W)
        full = torch.zeros((len(ts), 3, Gy * cell_rows, Gx * 64), dtype=torch.int32, device=v.device)
        full[:, :, rows, :W] = hits.to(torch.int32)
        out[ts] = full.view(len(ts), 3, Gy, cell_rows, Gx, 64).sum((3, 5), dtype=torch.int32)
    return out


def torch_weave(v, table):
    T, Hf, W, C = v.shape
    out = torch.empty((table.shape[0], 2 * Hf, W, C), dtype=v.dtype, device=v.device)
    out[:, 0::2] = v.index_select(0, table[:, 0])
    out[:, 1::2] = v.index_select(0, table[:, 1])
    return out


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


def burst_ms(fn, reps, n=20):
    """median device time per call in ms of n calls enqueued back to back between two events: the host's work on one call
    hides behind the device's on the one before, which one call between two events cannot show"""
    def many():
        for _ in range(n):
            fn()
    return device_ms(many, reps) / n


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

    say("Inverse telecine on one %s device.  Device time between two events around one call, median of %d after warm-up; "
        "the kernel and the PyTorch composition timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    comb_q, diff_q = tensors._check_q("c", tensors.COMB_THRESHOLD), tensors._check_q("d", tensors.DIFF_THRESHOLD)
    for T, decimate in ((16, 1), (64, 8)):
        v = film_fields(T, decimate=decimate).to(dev)
        _, Hf, W, C = v.shape
        res = {}
        k = device_ms(lambda: res.__setitem__("k", field_metrics(v, layout="NHWC").counts), args.reps)
        t = device_ms(lambda: res.__setitem__("t", torch_metrics(v, 0, 16, comb_q, diff_q)), args.reps)
        kb = burst_ms(lambda: field_metrics(v, layout="NHWC"), args.reps)
        floor = v.numel() + res["k"].numel() * 4
        m = match_fields(field_metrics(v, layout="NHWC"))
        say()
        say("field_metrics (k_field_metrics): %d uint8 NHWC fields of %d x %d x %d, cells of 16 x 64 -> counts %s" % (
            T, W, Hf, C, tuple(res["k"].shape)))
        say("  one call                                   %9.3f ms   %.4f ms per field" % (k, k / T))
        say("  per call, 20 calls back to back            %9.3f ms   %.4f ms per field" % (kb, kb / T))
        say("  byte floor: every field byte once + the counts = %.2f MB = %.4f ms at %.1f TB/s: back to back the call takes "
            "%.1f x that (%.3f TB/s of distinct bytes)" % (floor / 1e6, floor / HBM * 1e3, HBM / 1e12, kb / (floor / HBM * 1e3),
                                                          floor / (kb * 1e-3) / 1e12))
        say("  the rule in PyTorch operations, int32      %9.3f ms   %.1f x the kernel; the same counts: %s" % (
            t, t / k, torch.equal(res["k"], res["t"])))
        say("    (one call against one call)")
        say("  match_fields on them: cadence %s, share %.2f, votes %s" % (m.cadence, m.share, "".join("FPNV"[i] for i in m.votes.tolist())))
        if decimate == 1:
            table = torch.from_numpy(tensors.telecine_plan(m.groups.numpy(), 0, "bob")[0])
            tab = table.to(dev)
            kw = device_ms(lambda: res.__setitem__("k", weave_fields(v, table, layout="NHWC")), args.reps)
            kd = device_ms(lambda: res.__setitem__("k", weave_fields(v, tab, layout="NHWC")), args.reps)
            tw = device_ms(lambda: res.__setitem__("t", torch_weave(v, tab)), args.reps)
            kwb = burst_ms(lambda: weave_fields(v, table, layout="NHWC"), args.reps)
            twb = burst_ms(lambda: torch_weave(v, tab), args.reps)
            nbytes = 2 * res["k"].numel()
            say()
            say("weave_fields (k_weave_fields): %d frames of %d x %d x %d uint8 from those fields" % (len(table), W, 2 * Hf, C))
            say("  the call, table on the host (checked and uploaded) %9.3f ms; table on the device (copied to the host, checked, "
                "uploaded) %9.3f ms" % (kw, kd))
            say("  two index_selects + strided copies                 %9.3f ms   %.2f x the call; the same bytes: %s" % (
                tw, tw / kw, torch.equal(res["k"], res["t"])))
            say("  per call, 20 back to back: the call %9.3f ms, the index_selects and copies %9.3f ms = %.2f x the call" % (
                kwb, twb, twb / kwb))
            say("  byte floor: every output byte read and written once = %.2f MB = %.4f ms: back to back the call takes %.1f x "
                "that" % (nbytes / 1e6, nbytes / HBM * 1e3, kwb / (nbytes / HBM * 1e3)))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
