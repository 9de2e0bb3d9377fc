#!/usr/bin/env python3
"""Cost of the two mesh kernels (tensors.mesh_motion -> papof_mesh_motion_tensor: k_mesh_median + k_mesh_spatial;
tensors.warp_mesh -> papof_warp_mesh_tensor: k_warp_mesh) on one device: device time between events, median of --reps in one
run, after warm-up.

  warp        8 uint8 NHWC frames of 1920x1080 (C = 3), float64 matrices, uint8 out: warp_affine, and warp_mesh with a
              16 x 16 table (staged in LDS) and a 40 x 40 one (read from global memory); both move the same bytes.
  medians     mesh_motion (16 x 16 cells, motion and mask) on one 1920x1080 pair and on 100 pairs of 240x135, against the
              same rule in torch operations (an index gather of every window's lattice samples, then torch.sort, then a
              gather of the rank) and against ONE iteration of global_motion on the same flows.
  whole call  stabilize_video_mesh against stabilize_video on the same video at 240x135 and 1920x1080 (wall: call +
              synchronise), split into flow_video_fb against flow_video and the rest.

    python3 tools/mesh_probe.py --out profiles/mesh_probe.txt"""
import argparse
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from papteam_opticalflow_amd.tensors import (flow_video, flow_video_fb, global_motion, mesh_motion, stabilize_video,  # noqa: E402
                                             stabilize_video_mesh, warp_affine, warp_mesh)


def device_us(fn, reps):
    """median (min, max) of the device time of fn between two events, microseconds"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return float(np.median(out)), min(out), max(out)


def wall_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(out)), min(out), max(out)


def flows(B, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    f = torch.empty(B, 2, H, W, dtype=torch.float64)
    A = torch.zeros(B, 2, 3, dtype=torch.float64)
    for i in range(B):
        A[i, :, :2] = torch.eye(2, dtype=torch.float64) + 0.01 * torch.randn(2, 2, generator=g, dtype=torch.float64)
        A[i, :, 2] = 2 * torch.randn(2, generator=g, dtype=torch.float64)
        f[i, 0] = A[i, 0, 0] * x + A[i, 0, 1] * y + A[i, 0, 2] - x
        f[i, 1] = A[i, 1, 0] * x + A[i, 1, 1] * y + A[i, 1, 2] - y
    f += 0.2 * torch.randn(B, 2, H, W, generator=g, dtype=torch.float64)
    occ = torch.rand(B, H, W, generator=g) < 0.05
    return f.to(dev), A.to(dev), occ.to(dev)


def torch_medians(f, A, occ, grid):
    """the window medians of mesh_motion in torch operations: the closure that runs them on the device"""
    from _mesh_ref import _axis, lattice_step
    B, _, H, W = f.shape
    GH, GW = grid
    step = lattice_step(H, W, GH, GW)
    idx = np.zeros(((GH + 1) * (GW + 1), 1024), np.int64)
    live = np.zeros(idx.shape, bool)
    for i in range(GH + 1):
        ys = _axis(i, GH, H, step)
        for j in range(GW + 1):
            xs = _axis(j, GW, W, step)
            k = (ys[:, None] * W + xs[None, :]).ravel()
            idx[i * (GW + 1) + j, :len(k)] = k
            live[i * (GW + 1) + j, :len(k)] = True
    idx, live = torch.from_numpy(idx).to(f.device), torch.from_numpy(live).to(f.device)
    y, x = torch.meshgrid(torch.arange(H, device=f.device, dtype=torch.float64),
                          torch.arange(W, device=f.device, dtype=torch.float64), indexing="ij")

    def run():
        gx = ((A[:, 0, 0, None, None] * x + A[:, 0, 1, None, None] * y) + A[:, 0, 2, None, None]) - x
        gy = ((A[:, 1, 0, None, None] * x + A[:, 1, 1, None, None] * y) + A[:, 1, 2, None, None]) - y
        X, Y = x + f[:, 0], y + f[:, 1]
        valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1) & ~occ
        res = torch.stack([f[:, 0] - gx, f[:, 1] - gy], 1).reshape(B, 2, H * W)
        v = valid.reshape(B, H * W)[:, idx] & live                      # (B, V, 1024)
        s = torch.where(v[:, None], res[:, :, idx], torch.full((), float("inf"), dtype=torch.float64, device=f.device))
        s = torch.sort(s, dim=-1).values
        n = v.sum(-1)
        rank = ((n - 1).clamp(min=0) // 2)[:, None, :, None].expand(B, 2, -1, 1)
        return torch.gather(s, 3, rank)[..., 0], n

    return run


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

    def line(what, t, base=None):
        say("  %-46s %10.1f us  (%.1f, %.1f)%s" % (what, t[0], t[1], t[2], "" if base is None else "   %.2f x" % (t[0] / base)))

    say("The mesh kernels on one %s device: device time between events, median (min, max) of %d in one run after warm-up."
        % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    g = torch.Generator().manual_seed(3)
    fr = torch.randint(0, 256, (8, 1080, 1920, 3), generator=g, dtype=torch.uint8).to(dev)
    th = 0.01 * torch.randn(8, generator=g, dtype=torch.float64)
    M = torch.zeros(8, 2, 3, dtype=torch.float64)
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = th.cos(), -th.sin(), th.sin(), th.cos()
    M[:, :, 2] = 3 * torch.randn(8, 2, generator=g, dtype=torch.float64)
    M = M.to(dev)
    say()
    say("warp: 8 uint8 NHWC frames of 1920x1080 (C = 3), float64 matrices, uint8 out")
    ta = device_us(lambda: warp_affine(fr, M, layout="NHWC"), args.reps)
    line("warp_affine", ta)
    for cells in (16, 40):
        D = (1.5 * torch.randn(8, cells + 1, cells + 1, 2, generator=g, dtype=torch.float64)).to(dev)
        line("warp_mesh, %d x %d cells (%s)" % (cells, cells, "LDS" if (cells + 1) ** 2 <= 33 * 33 else "global"),
             device_us(lambda: warp_mesh(fr, M, D, layout="NHWC"), args.reps), ta[0])
    for what, B, H, W, seed in (("1920x1080, 1 pair", 1, 1080, 1920, 1), ("240x135, 100 pairs", 100, 135, 240, 2)):
        f, A, occ = flows(B, H, W, seed, dev)
        say()
        say("medians: %s, 16 x 16 cells, float64 flow, motion and mask" % what)
        tm = device_us(lambda: mesh_motion(f, motion=A, occlusion=occ), args.reps)
        line("mesh_motion (both kernels)", tm)
        line("mesh_motion, spatial=False", device_us(lambda: mesh_motion(f, motion=A, occlusion=occ, spatial=False), args.reps), tm[0])
        line("torch: index gather + sort + gather", device_us(torch_medians(f, A, occ, (16, 16)), max(3, args.reps // 2)), tm[0])
        o4 = torch.stack([occ, occ], 1)
        line("global_motion, ONE iteration", device_us(lambda: global_motion(f, occlusion=o4, iters=1), args.reps), tm[0])
    import cases
    for res, T in (("240", 8), ("1920", 3)):
        a = cases.load_frame_u8(res, 1)
        H, W, _ = a.shape
        v = torch.from_numpy(np.stack([np.roll(a, (t, 2 * t), (0, 1)) for t in range(T)])).to(dev)
        say()
        say("whole call: %d uint8 NHWC frames of %dx%d, %d levels (wall: call + synchronise, median (min, max) of %d)"
            % (T, W, H, args.levels, max(3, args.reps // 3)))
        n = max(3, args.reps // 3)
        ts = wall_us(lambda: stabilize_video(v, args.levels, layout="NHWC"), n)
        line("stabilize_video", ts)
        tmesh = wall_us(lambda: stabilize_video_mesh(v, args.levels, layout="NHWC"), n)
        line("stabilize_video_mesh", tmesh, ts[0])
        tf = wall_us(lambda: flow_video(v, args.levels, layout="NHWC", out_dtype=torch.float64), n)
        tfb = wall_us(lambda: flow_video_fb(v, args.levels, layout="NHWC", out_dtype=torch.float64), n)
        line("flow_video", tf)
        line("flow_video_fb", tfb, tf[0])
        sv = stabilize_video_mesh(v, args.levels, layout="NHWC")
        fb = flow_video_fb(v, args.levels, layout="NHWC", out_dtype=torch.float64)
        tk = device_us(lambda: mesh_motion(sv.flow, motion=sv.motion, occlusion=fb.occlusion), args.reps)
        tw = device_us(lambda: warp_mesh(v, sv.transforms, sv.mesh, layout="NHWC"), args.reps)
        twa = device_us(lambda: warp_affine(v, sv.transforms, layout="NHWC"), args.reps)
        line("mesh_motion on its flows (device)", tk)
        line("warp_mesh (device)", tw)
        line("warp_affine (device)", twa)
        say("  the difference of the whole calls, %.1f us: %.1f us the backward flows of flow_video_fb, %.1f us mesh_motion, "
            "%.1f us warp_mesh over warp_affine; mesh_motion is %.3f %% of stabilize_video_mesh"
            % (tmesh[0] - ts[0], tfb[0] - tf[0], tk[0], tw[0] - twa[0], 100 * tk[0] / tmesh[0]))
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
