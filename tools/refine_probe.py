#!/usr/bin/env python3
"""Cost and effect of the edge-aware flow refinement (tensors.refine_flow -> papof_refine_flow_tensor: one k_refine per pass).

Cost, uint8 NHWC guides (C = 3), float64 flows of the frames themselves (flow_pairs_fb) with their occlusion masks:
  1080p       the committed 1920x1080 pair, its forward flow (5 levels), one item;
  240 B=32    32 pairs of 240x135 made from the committed frames, their forward flows (4 levels);
each at radius 7 and 3, one pass: the time between two events around the call (one kernel; median, min, max of --reps after
warm-up), the passes over the window that a lane made (mean and maximum over the pixels; the kernel's optional output), and
the same filter written with torch operations (unfold, sort, cumsum, gather; float64 weights: a time baseline, not a byte
reference).  Then the share of a flow_video_fb + refine_video_flows pipeline that the refinement takes, and what it does to
estimated flows: end-point error on the scene with known ground truth (tests/_refine_ref.py: two_layer_frames), the
interpolation error of frame 2 of the committed triples and the hole PSNR of inpaint_video on the synthetic video of
tests/test_inpaint_cpu.py, with refined against unrefined flows.

LDS bank conflicts come from a run of their own:
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -f csv -d DIR -o refine -- python3 tools/refine_probe.py --kernel-only
    python3 tools/refine_probe.py --pmc DIR --out profiles/refine_probe.txt"""
import argparse
import csv
import glob
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd import tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (flow_pairs_fb, flow_video_fb, inpaint_video, interpolate,  # noqa: E402
                                             refine_flow, refine_video_flows)


def video_240(n):
    import cases
    f1, f2 = cases.load_frame_u8("240", 1), cases.load_frame_u8("240", 2)
    return np.stack([np.roll(f1 if i % 2 == 0 else f2, (i // 2) * 3, axis=1) for i in range(n)])


def make_cases(dev):
    import cases
    a, b = (torch.from_numpy(cases.load_frame_u8("1920", i)[None]).to(dev) for i in (1, 2))
    fb = flow_pairs_fb(a, b, 5, layout="NHWC")
    v = torch.from_numpy(video_240(33)).to(dev)
    fv = flow_video_fb(v, 4, layout="NHWC")
    return [("1920x1080, 1 item", a, fb.flow_fw, fb.occlusion[:, 0].contiguous()),
            ("240x135, 32 items", v[:-1], fv.flow_fw, fv.occlusion[:, 0].contiguous())]


def torch_refine(flow, guide, occ, radius, sigma_s, sigma_c):
    """the filter with torch operations: unfold the padded planes, sort each window by value, cumsum the weights in that
    order, take the first value at or beyond half the total (float64 weights, exp on the device)"""
    B, _, H, W = flow.shape
    k = 2 * radius + 1
    unf = lambda t: torch.nn.functional.unfold(torch.nn.functional.pad(t, (radius,) * 4), k)  # noqa: E731  (B, c k k, H W)
    g = guide.permute(0, 3, 1, 2).double() / 255.0
    C = g.shape[1]
    live = unf((~occ & torch.isfinite(flow).all(1))[:, None].double())
    gn = unf(g).view(B, C, k * k, H * W)
    d2 = ((gn - g.reshape(B, C, 1, H * W)) ** 2).mean(1)
    d = torch.arange(-radius, radius + 1, device=flow.device, dtype=torch.float64)
    ws = torch.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2 * sigma_s ** 2)).reshape(1, k * k, 1)
    w = ws * torch.exp(-d2 / (2 * sigma_c ** 2)) * live
    out = []
    for c in range(2):
        vals = unf(torch.nan_to_num(flow[:, c:c + 1]))
        sv, order = torch.sort(vals, dim=1)
        cum = torch.cumsum(torch.gather(w, 1, order), 1)
        first = (2 * cum >= cum[:, -1:]).double().argmax(1, keepdim=True)
        out.append(torch.gather(sv, 1, first).view(B, H, W))
    return torch.stack(out, 1)


def event_times(fn, reps):
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


def pmc_share(path):
    """sum of SQ_LDS_BANK_CONFLICT over sum of SQ_LDS_IDX_ACTIVE of the k_refine dispatches in rocprofv3's counter CSV"""
    files = glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit("no *counter_collection.csv under %s" % path)
    tot = {}
    for row in csv.DictReader(open(files[0])):
        row = {k.strip().lower(): v for k, v in row.items()}
        if "k_refine" in row.get("kernel_name", ""):
            tot[row["counter_name"]] = tot.get(row["counter_name"], 0.0) + float(row["counter_value"])
    return tot


def epe(flow, true, mask=None):
    e = ((flow.double().cpu().numpy() - true) ** 2).sum(1)[0] ** 0.5
    return float(e[mask].mean() if mask is not None else e.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run the refinement calls only (for rocprofv3 --pmc)")
    ap.add_argument("--pmc", default=None, help="rocprofv3 output directory of a --pmc run of --kernel-only")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases_ = make_cases(dev)
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, g, f, o in cases_:
            for radius in (7, 3):
                refine_flow(f, g, occlusion=o, radius=radius, sigma_s=float(radius), layout="NHWC")
        torch.cuda.synchronize()
        return
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    say("Edge-aware flow refinement on one %s device.  uint8 NHWC guides (C = 3), float64 flows of the frames themselves with "
        "their occlusion masks, one pass, sigma_s = radius, sigma_c = 7 / 255.  Times: between two events around the call, median "
        "(min, max) of %d after warm-up." % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for what, g, f, o in cases_:
        B, H, W, _ = g.shape
        for radius in (7, 3):
            call = lambda: refine_flow(f, g, occlusion=o, radius=radius, sigma_s=float(radius), layout="NHWC")  # noqa: E731
            med, lo, hi = event_times(call, args.reps)
            desc = tensors._check_refine_flow(f, g, o, None, "NHWC", None)
            _, count = tensors._refine(f, desc[2], desc[0], desc[1], desc[3], desc[4], radius, float(radius), 7 / 255, 1, desc[5],
                                       passes=True)
            n = (2 * radius + 1) ** 2
            say()
            say("%s, radius %d (%d neighbours): k_refine %8.3f ms (%.3f, %.3f) = %.2f ns per pixel; passes per pixel: mean %.2f, "
                "max %d; per neighbour visit of a pass %.1f ps" % (what, radius, n, med, lo, hi, 1e6 * med / (B * H * W),
                                                                 float(count.double().mean()), int(count.max()),
                                                                 1e9 * med / (B * H * W * n * float(count.double().mean()))))
            try:
                t_med, t_lo, t_hi = event_times(lambda: torch_refine(f, g, o, radius, float(radius), 7 / 255), max(3, args.reps // 3))
                got, ref = call(), torch_refine(f, g, o, radius, float(radius), 7 / 255)
                say("    torch (unfold, sort, cumsum, gather)  %9.3f ms (%.3f, %.3f) = %.1f x k_refine; peak memory %.1f GB; "
                    "components equal to k_refine's: %.4f" % (t_med, t_lo, t_hi, t_med / med, torch.cuda.max_memory_allocated() / 1e9,
                                                            float((got == ref).double().mean())))
            except torch.cuda.OutOfMemoryError:
                say("    torch (unfold, sort, cumsum, gather): out of memory")
            torch.cuda.empty_cache()
    if args.pmc:
        tot = pmc_share(args.pmc)
        say()
        say("LDS, summed over the four k_refine dispatches of a --kernel-only run under rocprofv3 --pmc: %s; bank-conflict share "
            "of the LDS-active cycles %.3f" % (", ".join("%s %.4g" % kv for kv in sorted(tot.items())),
                                               tot.get("SQ_LDS_BANK_CONFLICT", 0.0) / max(tot.get("SQ_LDS_IDX_ACTIVE", 0.0), 1.0)))
    say()
    say("Share of a pipeline (wall, call + synchronise, median of %d):" % args.reps)
    import cases
    for what, frames, levels in (("240x135, 17 frames", torch.from_numpy(video_240(17)).to(dev), 4),
                                 ("1920x1080, 2 frames", torch.from_numpy(np.stack([cases.load_frame_u8("1920", i) for i in (1, 2)])).to(dev), 5)):
        def wall(fn):
            fn()
            torch.cuda.synchronize()
            dt = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                dt.append(time.perf_counter() - t0)
            return float(np.median(dt)), r
        t_flow, fb = wall(lambda: flow_video_fb(frames, levels, layout="NHWC"))
        t_ref, _ = wall(lambda: refine_video_flows(frames, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC"))
        say("  %s: flow_video_fb %.2f ms, refine_video_flows (defaults; both directions, the mask recomputed) %.2f ms = %.1f %% of "
            "the two" % (what, 1e3 * t_flow, 1e3 * t_ref, 100 * t_ref / (t_flow + t_ref)))
    say()
    say("Estimated flows of the scene with known ground truth (96x128, two layers; flow_pairs_fb, 4 levels), end-point error "
        "in the band around the motion boundaries and over the whole image:")
    from _refine_ref import two_layer_frames
    for seed in (0, 1, 2):
        f1, f2, true, band = two_layer_frames(seed)
        v = torch.from_numpy(np.concatenate([f1, f2])).to(dev)
        fb = flow_video_fb(v, 4, layout="NHWC")
        line = "  seed %d: unrefined band %.3f whole %.3f" % (seed, epe(fb.flow_fw, true, band), epe(fb.flow_fw, true))
        for iters in (1, 3):
            for use_occ in (True, False):
                r = refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion if use_occ else None, layout="NHWC",
                                       iters=iters)
                line += "; %d pass%s %s mask: band %.3f whole %.3f" % (iters, "es" if iters > 1 else "", "with" if use_occ else
                                                                       "without", epe(r.flow_fw, true, band), epe(r.flow_fw, true))
        say(line)
    say()
    say("Interpolation error (mean absolute, [0, 1]) of frame 2 of the committed triples from frames 1 and 3 at t = 0.5, 5 levels, "
        "the device's flows; splat with weights 1:")
    for r in ("240", "480"):
        f1, f2, f3 = (cases.load_frame_u8(r, i) for i in (1, 2, 3))
        v = torch.from_numpy(np.stack([f1, f3])).to(dev)
        truth = f2.astype(np.float64) / 255.0
        fb = flow_video_fb(v, 5, layout="NHWC")
        line = "  %sx%s:" % (cases.SIZES[r][1], cases.SIZES[r][0])
        for name, flows in (("unrefined", fb), ("refined, 1 pass", refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC")),
                            ("refined, 3 passes", refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC", iters=3))):
            for method in ("gather", "splat"):
                out = interpolate(v[:1], v[1:], flows.flow_fw, flows.flow_bw, 0.5, occlusion=flows.occlusion, layout="NHWC",
                                  out_dtype=torch.float64, method=method)
                line += "  %s %s %.6f" % (name, method, float(np.abs(out[0, 0].cpu().numpy() - truth).mean()))
        say(line)
    say()
    say("Video completion (the synthetic video of tests/test_inpaint_cpu.py: 8 frames of 200x120, a moving occluder, masks "
        "dilated by 3 px; flow_video_fb, 4 levels; inpaint_video(flows=...) at its defaults), PSNR over the masked pixels:")
    from test_inpaint_cpu import _psnr_masked, synthetic_video
    clean, frames, masks, _, _ = synthetic_video()
    v, m = torch.from_numpy(frames).to(dev), torch.from_numpy(masks).to(dev)
    fb = flow_video_fb(v, 4, layout="NHWC")
    both = fb.occlusion | torch.stack([m[:-1], m[1:]], 1)  # the pixels under the masks get no vote either
    line = " "
    for name, flows in (("unrefined", fb),
                        ("refined", refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=fb.occlusion, layout="NHWC")),
                        ("refined, masks as occlusion", refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=both, layout="NHWC")),
                        ("refined, masks as occlusion, 3 passes", refine_video_flows(v, fb.flow_fw, fb.flow_bw, occlusion=both,
                                                                                   layout="NHWC", iters=3))):
        out = inpaint_video(v, m, 4, flows=(flows.flow_fw, flows.flow_bw), layout="NHWC")
        line += " %s %.2f dB;" % (name, _psnr_masked(out.video.cpu().numpy(), clean, masks))
    say(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
