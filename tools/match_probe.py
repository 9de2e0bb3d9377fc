#!/usr/bin/env python3
"""Cost and effect of the dense block matcher (tensors.match_pairs -> papof_match_tensor: k_match_prepare, k_match;
tensors.match_init -> papof_match_densify_tensor: k_match_densify, then the hole fill).

Frames: one uint8 NHWC pair (C = 3) of band-limited texture per size -- 240x135, 480x270, 1920x1080 -- the second frame a pan
of the first by (28, 9) pixels (tests/_match_ref.py: pan_scene).  Per size, for the defaults (stride 2, patch 3, search 20)
and for search 32:
  match_pairs (both directions: two items)     the time between two events around the call, median (min, max) of --reps;
  match_init                                    likewise;
  flow_pairs_fb, 5 levels                       the cold call, wall time around the call and a synchronisation;
  flow_pairs_ld, 2 levels                       likewise, and both calls' end-point error on the pixels that stay in view;
  the same matcher with torch operations        replicate padding, shifted absolute differences, avg_pool2d as the box sum, a
                                                running minimum of the packed keys: a time baseline, and the share of its cells
                                                that equal k_match's (the rule is the same: all of them).
Kernel times and counters come from runs of their own, and other builds of the library (match.hip with another kG, linked
with the same objects) are timed in child processes through PAPOF_LIB; the report names what it was given:
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o match -- python3 tools/match_probe.py --kernel-only
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -f csv -d DIR2 -o match -- python3 tools/match_probe.py --kernel-only --reps 1
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES -f csv -d DIR3 \
        -o match -- python3 tools/match_probe.py --kernel-only --reps 1
    python3 tools/match_probe.py --kernel-trace DIR --pmc DIR2 DIR3 --ab 1=LIB1 8=LIB8 16=LIB16 --out profiles/match_probe.txt"""
import argparse
import csv
import glob
import io
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import flow_pairs_fb, flow_pairs_ld, match_init, match_pairs  # noqa: E402

SIZES = ((135, 240), (270, 480), (1080, 1920))
CONFIGS = (dict(stride=2, patch=3, search=20), dict(stride=2, patch=3, search=32))
KERNELS = ("k_match_prepare", "k_match_densify", "k_match")  # (the longer names first: k_match is a prefix of both)


def make_cases(dev):
    from _match_ref import pan_scene
    out = []
    for H, W in SIZES:
        im1, im2, truth, inside = pan_scene(3, (28, 9), H, W)
        out.append(("%dx%d" % (W, H), torch.from_numpy(im1[None]).to(dev), torch.from_numpy(im2[None]).to(dev), truth, inside))
    return out


def torch_match(a, b, stride, patch, search):
    """the rule with torch operations on (1, H, W, C) uint8 frames: (d (2, h, w), cost (h, w)) in cells, int64"""
    F = torch.nn.functional
    n = stride * stride
    dec = lambda t: ((F.avg_pool2d(t.permute(0, 3, 1, 2).float(), stride, divisor_override=1) + n // 2) // n)  # noqa: E731
    A, B = dec(a), dec(b)
    h, w = A.shape[2:]
    P, s = patch, search
    Ap = F.pad(A, (P,) * 4, mode="replicate")
    ys = torch.arange(-P, h + P, device=a.device)
    xs = torch.arange(-P, w + P, device=a.device)
    yy, xx = torch.meshgrid(torch.arange(h, device=a.device), torch.arange(w, device=a.device), indexing="ij")
    best = torch.full((h, w), torch.iinfo(torch.int64).max, device=a.device)
    for dy in range(-s, s + 1):
        rows = B[:, :, (ys + dy).clamp(0, h - 1)]
        row_ok = (yy + dy >= 0) & (yy + dy < h)
        for dx in range(-s, s + 1):
            D = (Ap - rows[:, :, :, (xs + dx).clamp(0, w - 1)]).abs().sum(1, keepdim=True)
            cost = F.avg_pool2d(D, 2 * P + 1, stride=1, divisor_override=1)[0, 0].long()
            key = (cost << 26) | ((dx * dx + dy * dy) << 14) | ((dy + 64) << 7) | (dx + 64)
            ok = row_ok & (xx + dx >= 0) & (xx + dx < w)
            best = torch.where(ok, torch.minimum(best, key), best)
    return torch.stack([(best & 127) - 64, ((best >> 7) & 127) - 64]), best >> 26


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


def wall_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    dt = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(dt)), min(dt), max(dt)


def _rows(path, pattern):
    files = glob.glob(os.path.join(path, "**", pattern), recursive=True)
    if not files:
        raise SystemExit("no %s under %s" % (pattern, path))
    for row in csv.DictReader(open(files[0])):
        yield {k.strip().lower(): v for k, v in row.items()}


def _kernel(name):
    for k in KERNELS:
        if k in name:
            return k
    return None


def kernel_trace(path, reps):
    """{kernel: [[us of each dispatch of case i]]} from rocprofv3's kernel trace of a --kernel-only run, whose cases run in
    order, `reps` calls each (k_match_prepare runs twice per call: one launch per frame tensor)"""
    per = {"k_match_prepare": 2 * reps, "k_match": reps, "k_match_densify": 2 * reps}
    seen = {k: [] for k in KERNELS}
    rows = sorted(_rows(path, "*kernel_trace.csv"), key=lambda r: int(r["start_timestamp"]))
    for r in rows:
        k = _kernel(r.get("kernel_name", ""))
        if k:
            seen[k].append((int(r["end_timestamp"]) - int(r["start_timestamp"])) / 1e3)
    return {k: [v[i:i + per[k]] for i in range(0, len(v), per[k])] for k, v in seen.items()}


def pmc_totals(path):
    """{kernel: {counter: sum over its dispatches}} of rocprofv3's counter CSV"""
    tot = {}
    for r in _rows(path, "*counter_collection.csv"):
        k = _kernel(r.get("kernel_name", ""))
        if k:
            t = tot.setdefault(k, {})
            t[r["counter_name"]] = t.get(r["counter_name"], 0.0) + float(r["counter_value"])
    return tot


def epe(flow, truth, where):
    f = flow[0].double().cpu().numpy()
    return float(np.hypot(f[0] - truth[..., 0], f[1] - truth[..., 1])[where].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-only", action="store_true", help="run match_pairs and match_init only, --reps times per case")
    ap.add_argument("--kernel-trace", default=None, help="rocprofv3 output directory of a --kernel-trace run of --kernel-only")
    ap.add_argument("--pmc", default=[], nargs="*", help="rocprofv3 output directories of --pmc runs of --kernel-only --reps 1")
    ap.add_argument("--ab", default=[], nargs="*", metavar="KG=LIB",
                    help="other builds of libpapof.so (match.hip with kG = KG) to time with --match-only in child processes")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline")
    ap.add_argument("--match-only", action="store_true", help="time match_pairs only (A/B builds through PAPOF_LIB)")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases_ = make_cases(dev)
    torch.cuda.synchronize()
    if args.kernel_only:
        for _, a, b, _, _ in cases_:
            for cfg in CONFIGS:
                for _ in range(args.reps):
                    m = match_pairs(a, b, layout="NHWC", **cfg)
                    match_init(*m, tuple(a.shape[1:3]))
        torch.cuda.synchronize()
        return
    if args.match_only:
        for name, a, b, _, _ in cases_:
            for cfg in CONFIGS:
                print("%s search %d: match_pairs %.3f (%.3f, %.3f) ms" % (
                    name, cfg["search"], *event_times(lambda: match_pairs(a, b, layout="NHWC", **cfg), args.reps)), flush=True)
        return
    rep = io.StringIO()

    def say(s=""):
        print(s, flush=True)
        rep.write(s + "\n")

    kt = kernel_trace(args.kernel_trace, args.reps) if args.kernel_trace else None
    say("Dense block matching on one %s device.  One uint8 NHWC pair (C = 3) per size, a pan by (28, 9) pixels; both directions "
        "(two items).  Event and wall times: median (min, max) of %d after warm-up, in ms." % (
            torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    i = 0
    for name, a, b, truth, inside in cases_:
        size = tuple(a.shape[1:3])
        cold = wall_times(lambda: flow_pairs_fb(a, b, 5, layout="NHWC"), max(3, args.reps // 2))
        e_cold = epe(flow_pairs_fb(a, b, 5, layout="NHWC").flow_fw, truth, inside)
        say()
        say("%s: flow_pairs_fb, 5 levels, cold: %.2f (%.2f, %.2f) ms wall; EPE in view %.3f px" % (name, *cold, e_cold))
        for cfg in CONFIGS:
            t_m = event_times(lambda: match_pairs(a, b, layout="NHWC", **cfg), args.reps)
            m = match_pairs(a, b, layout="NHWC", **cfg)
            t_i = event_times(lambda: match_init(*m, size), args.reps)
            init = match_init(*m, size)
            t_ld = wall_times(lambda: flow_pairs_ld(a, b, 2, layout="NHWC", **cfg), max(3, args.reps // 2))
            e_ld = epe(flow_pairs_ld(a, b, 2, layout="NHWC", **cfg).flow_fw, truth, inside)
            h, w = m.cost_fw.shape[1:]
            cand = (2 * cfg["search"] + 1) ** 2
            sads = 2.0 * h * w * cand * (2 * cfg["patch"] + 1) ** 2
            say("  stride %d patch %d search %d (%d x %d cells, %d candidates, %.3g packed SADs):" % (
                cfg["stride"], cfg["patch"], cfg["search"], w, h, cand, sads))
            say("    match_pairs %.3f (%.3f, %.3f) ms = %.2f SADs per ns; match_init %.3f (%.3f, %.3f) ms; reliable %.4f" % (
                *t_m, sads / (1e6 * t_m[0]), *t_i, float(init.reliable.double().mean())))
            say("    flow_pairs_ld, 2 levels: %.2f (%.2f, %.2f) ms wall = %.2f x the cold call; EPE in view %.4f px" % (
                *t_ld, t_ld[0] / cold[0], e_ld))
            if kt:
                for k in KERNELS:
                    us = kt[k][i] if i < len(kt[k]) else []
                    if us:
                        say("    %-16s %9.1f us per dispatch (min %.1f, max %.1f; %d dispatches under rocprofv3 --kernel-trace)" % (
                            k, float(np.median(us)), min(us), max(us), len(us)))
            if not args.no_torch:
                t_t = event_times(lambda: torch_match(a, b, **cfg), 1)
                d, c = torch_match(a, b, **cfg)
                same = float(((cfg["stride"] * d == m.disp_fw[0].long()).all(0) & (c == m.cost_fw[0].long())).double().mean())
                say("    torch operations, ONE direction: %.1f ms = %.0f x k_match per direction; cells equal to k_match's: %.4f" % (
                    t_t[0], t_t[0] / (t_m[0] / 2), same))
            i += 1
    for path in args.pmc:
        say()
        say("Counters of rocprofv3 --pmc over a --kernel-only --reps 1 run (the six cases once each, both directions), summed per "
            "kernel over its dispatches:")
        for k, t in sorted(pmc_totals(path).items()):
            say("  %s: %s" % (k, ", ".join("%s %.4g" % kv for kv in sorted(t.items()))))
            if t.get("SQ_LDS_IDX_ACTIVE"):
                say("    LDS bank-conflict share of the LDS-array cycles: %.2f %%" % (100 * t.get("SQ_LDS_BANK_CONFLICT", 0.0) / t["SQ_LDS_IDX_ACTIVE"]))
            if t.get("SQ_INSTS_VALU") and t.get("SQ_INSTS_LDS"):
                say("    VALU wave-instructions per LDS wave-instruction: %.2f" % (t["SQ_INSTS_VALU"] / t["SQ_INSTS_LDS"]))
    if args.ab:
        say()
        say("A/B: match_pairs (both directions) of other builds of the library, match.hip with only kG changed, each in a child "
            "process (--match-only --reps %d, PAPOF_LIB); the shipped build's are the match_pairs lines above." % args.reps)
        for item in args.ab:
            kg, lib = item.split("=", 1)
            env = dict(os.environ, PAPOF_LIB=os.path.abspath(lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--match-only", "--reps", str(args.reps)], env=env,
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                raise SystemExit("the kG = %s build failed: %s" % (kg, out.stderr[-400:]))
            say("  kG = %s:" % kg)
            for line in out.stdout.splitlines():
                if "match_pairs" in line:
                    say("    " + line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
