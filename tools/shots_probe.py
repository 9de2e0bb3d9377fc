#!/usr/bin/env python3
"""Cost of the shot-boundary kernel on one device: tensors.shot_histograms (one k_cell_hist launch) against the same rule
composed of PyTorch operations, against its byte floor and next to tensors.field_metrics, whose mapping it shares; and the
whole of tensors.flow_video_shots on a video with one cut against tensors.flow_video_fb on the same frames.

shot_histograms: 8 uint8 frames of 1920 x 1080 x 3 -- the committed 1080p frame rolled by 3 columns per frame, the last
three frames upside down: a cut at pair 4 --, NHWC and NCHW, and 32 frames of 240 x 135 x 3 (the frame decimated by 8).  The
PyTorch composition is the rule in int32: the quantisation, the integer luma, the bin, and the per-cell counts by one
scatter_add_ on offset indices; its counts must equal the kernel's.  Byte floor: every frame byte read once plus the counts,
over the 6.3 TB/s that streaming kernels reach on this device.  Times are device times between two events around one call, the
median of --reps (11) after warm-up, both versions in the same run.

flow_video_shots: the 8 frames of 1080p, 5 pyramid levels, wall time of the whole call (it is complete on return), the median
of 3 after one warm-up call, against flow_video_fb on the same frames -- which solves the cut pair too.

    python3 tools/shots_probe.py --out profiles/shots_probe.txt"""
import argparse
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import (detect_cuts, field_metrics, flow_video_fb, flow_video_shots,  # noqa: E402
                                             shot_histograms)

HBM = 6.3e12  # bytes per second that streaming kernels reach


def video(T, decimate=1, cut=None):
    """T frames of the committed frame, frame k rolled by 3 k columns; from frame `cut` on upside down"""
    import cases
    img = cases.load_frame_u8("1920", 1)[::decimate, ::decimate]
    frames = [np.roll(img, -3 * k, axis=1) for k in range(T)]
    if cut is not None:
        frames = [f if k < cut else f[::-1] for k, f in enumerate(frames)]
    return torch.from_numpy(np.stack([np.ascontiguousarray(f) for f in frames]))


def torch_hist(v, cell_rows, bins):
    """the rule of papof_cell_hist_tensor on uint8 frames v (T, H, W, 3) in PyTorch operations: hist (T, Gy, Gx, bins) int32"""
    T, H, W, C = v.shape
    Q = v.to(torch.int32) * 257
    L = (77 * Q[..., 0] + 150 * Q[..., 1] + 29 * Q[..., 2]) >> 8
    b = (L * bins) >> 16
    Gy, Gx = -(-H // cell_rows), -(-W // 64)
    cy = (torch.arange(H, device=v.device) // cell_rows)[None, :, None]
    cx = (torch.arange(W, device=v.device) // 64)[None, None, :]
    t = torch.arange(T, device=v.device)[:, None, None]
    idx = (((t * Gy + cy) * Gx + cx) * bins + b).reshape(-1).to(torch.int64)
    out = torch.zeros(T * Gy * Gx * bins, dtype=torch.int32, device=v.device)
    out.scatter_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
    return out.view(T, Gy, Gx, bins)


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


def wall_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Shot boundaries on one %s device.  Device time between two events around one call, median of %d after warm-up; "
        "the kernel and the PyTorch composition timed in the same run." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    big = video(8, cut=5).to(dev)
    cases_ = [("NHWC", big, "NHWC"), ("NCHW", big.permute(0, 3, 1, 2).contiguous(), "NCHW"),
              ("NHWC", video(32, decimate=8).to(dev), "NHWC")]
    for name, v, layout in cases_:
        nhwc = v if layout == "NHWC" else v.permute(0, 2, 3, 1)
        T, H, W, C = nhwc.shape
        res = {}
        k = device_ms(lambda: res.__setitem__("k", shot_histograms(v, layout=layout).hist), args.reps)
        t = device_ms(lambda: res.__setitem__("t", torch_hist(nhwc, 16, 16)), args.reps)
        kb = burst_ms(lambda: shot_histograms(v, layout=layout), args.reps)
        floor = v.numel() + res["k"].numel() * 4
        say()
        say("shot_histograms (k_cell_hist): %d uint8 %s frames of %d x %d x %d, cells of 16 x 64, 16 bins -> hist %s" % (
            T, name, W, H, C, tuple(res["k"].shape)))
        say("  one call                                   %9.3f ms   %.4f ms per frame" % (k, k / T))
        say("  per call, 20 calls back to back            %9.3f ms   %.4f ms per frame" % (kb, kb / T))
        say("  byte floor: every frame byte once + the counts = %.2f MB = %.4f ms at %.1f TB/s: back to back the call takes "
            "%.1f x that (%.3f TB/s of distinct bytes)" % (floor / 1e6, floor / HBM * 1e3, HBM / 1e12, kb / (floor / HBM * 1e3),
                                                          floor / (kb * 1e-3) / 1e12))
        say("  the rule in PyTorch operations, int32      %9.3f ms   %.1f x the kernel; the same counts: %s" % (
            t, t / k, torch.equal(res["k"], res["t"])))
        say("    (one call against one call)")
        for bins in (4, 64):
            say("  %2d bins, one call                          %9.3f ms" % (
                bins, device_ms(lambda: shot_histograms(v, bins=bins, layout=layout), args.reps)))
        s = detect_cuts(shot_histograms(v, layout=layout))
        say("  detect_cuts on them: cuts %s, flashes %s, distances %s" % (s.cuts, s.flashes, " ".join("%.3f" % d for d in s.distances)))
    fields = torch.from_numpy(np.stack([np.ascontiguousarray(big[k // 2].cpu().numpy()[k & 1::2]) for k in range(16)])).to(dev)
    fm = device_ms(lambda: field_metrics(fields, layout="NHWC"), args.reps)
    fmb = burst_ms(lambda: field_metrics(fields, layout="NHWC"), args.reps)
    ffloor = fields.numel() + 16 * 3 * 34 * 30 * 4
    say()
    say("field_metrics (k_field_metrics) in the same run: 16 uint8 NHWC fields of 1920 x 540 x 3: one call %.3f ms, back to back "
        "%.3f ms = %.1f x its byte floor of %.4f ms" % (fm, fmb, fmb / (ffloor / HBM * 1e3), ffloor / HBM * 1e3))
    say()
    say("flow_video_shots against flow_video_fb: the 8 NHWC frames of 1920 x 1080 x 3 with the cut at pair 4, %d levels, wall "
        "time of the whole call, median of 3 after one warm-up call" % args.levels)
    out = {}
    ws = wall_ms(lambda: out.__setitem__("s", flow_video_shots(big, args.levels, layout="NHWC")))
    wf = wall_ms(lambda: out.__setitem__("f", flow_video_fb(big, args.levels, layout="NHWC")))
    fb, shots = out["s"]
    say("  flow_video_shots  %9.1f ms   cuts %s, ranges %s" % (ws, shots.cuts, shots.ranges))
    say("  flow_video_fb     %9.1f ms   7 pairs solved, the cut pair among them" % wf)
    say("  saved             %9.1f ms = %.2f of flow_video_fb's time per pair (%.1f ms)" % (wf - ws, (wf - ws) / (wf / 7), wf / 7))
    same = all(torch.equal(fb.flow_fw[i], out["f"].flow_fw[i]) for i in range(7) if i not in shots.cuts)
    say("  the other pairs' forward flows are flow_video_fb's bytes: %s" % same)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
