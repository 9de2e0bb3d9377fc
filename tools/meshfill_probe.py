#!/usr/bin/env python3
"""Cost of the mosaic under the mesh rule (tensors.mosaic_mesh -> papof_mosaic_mesh_tensor: k_mesh_bounds + k_mosaic over
MeshMosaicArgs) on one device: device time between events around the call, median of --reps in one run, after warm-up.

  fill 1080p  stabilize_video_mesh_full's mosaic: 8 stabilized 1920x1080x3 uint8 frames, fill radius 15 (31 sources each), a
              16 x 16 grid, mode "first" with the count -- tools/mosaic_probe.py's case (a), the same sources and matrices.
              mosaic_mesh with neighbour_mesh's tables and with tables of zeros against mosaic (the affine call) on the same
              sources and matrices; each with the culling switched off (PAPOF_MOSAIC_CULL=0: no bounds kernel, no widened
              corner box, no per-pixel early-out); and against the composition it replaces: one warp_mesh per slot plus
              torch.where (the same pixels without the kernel).
  fill 240    the same at 240x135, 32 frames.
In both cases every neighbour exists, so slot k of all outputs is one slice of the video and the composition reads it in place.

    python3 tools/meshfill_probe.py --out profiles/meshfill_probe.txt"""
import argparse
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mosaic_probe import no_cull, shaky_motion, timed  # noqa: E402
from papteam_opticalflow_amd import tensors  # noqa: E402

GRID = (16, 16)


def fill_case(T, H, W, outs, radius, dev, seed):
    """the calls of stabilize_video_mesh_full's last step for the output frames `outs`: (mosaic, mosaic_mesh, mosaic_mesh on zero
    tables, the composition)"""
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    A = shaky_motion(T, H, W, seed)
    M = tensors.stabilizing_transforms(A, 15)
    src, mats = tensors.neighbour_transforms(M, A, radius)
    # per-vertex residuals of about 0.1 % of the frame's width per pair: tables of a few pixels
    res = 0.001 * W * torch.from_numpy(np.random.default_rng(seed).normal(0, 1, (T - 1, GRID[0] + 1, GRID[1] + 1, 2)))
    E = tensors.neighbour_mesh(res, 15, radius)
    src, mats, E = src[outs].contiguous(), mats[outs].contiguous().to(dev), E[outs].contiguous().to(dev)
    assert int(src.min()) >= 0  # every neighbour exists
    src_host = src.numpy()
    Z = torch.zeros_like(E)
    slot = [(mats[:, k].contiguous(), E[:, k].contiguous()) for k in range(src.shape[1])]

    def composed():
        out = have = None
        for k in range(src.shape[1]):
            s0 = int(src_host[0, k])
            w, v = tensors.warp_mesh(frames[s0:s0 + len(outs)], slot[k][0], slot[k][1], layout="NHWC")
            if k == 0:
                out, have = w, v
                continue
            v = v & ~have
            out = torch.where(v.unsqueeze(-1), w, out)
            have = have | v
        return out

    a = tensors.mosaic_mesh(frames, src_host, mats, E, (H, W), mode="first", layout="NHWC")
    assert torch.equal(a.out, composed())  # the same pixels
    amp = float(E.abs().max())
    return (lambda: tensors.mosaic(frames, src_host, mats, (H, W), mode="first", layout="NHWC"),
            lambda: tensors.mosaic_mesh(frames, src_host, mats, E, (H, W), mode="first", layout="NHWC"),
            lambda: tensors.mosaic_mesh(frames, src_host, mats, Z, (H, W), mode="first", layout="NHWC"), composed, amp)


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

    def line(what, t, base=None):
        say("  %-50s %10.1f us  (%.1f, %.1f)%s" % (what, t[0], t[1], t[2], "" if base is None else "   %.2f x" % (t[0] / base)))

    say("The mosaic under the mesh rule on one %s device.  Device time between events around the call, median (min, max) of %d "
        "in one run after warm-up; ratios against the first line of each case."
        % (torch.cuda.get_device_properties(0).gcnArchName.split(":")[0], args.reps))
    for title, T, H, W, outs, seed in (("8 frames of 1920x1080x3 uint8", 48, 1080, 1920, list(range(20, 28)), 1),
                                        ("32 frames of 240x135x3 uint8", 64, 135, 240, list(range(16, 48)), 3)):
        affine, mesh, zero, composed, amp = fill_case(T, H, W, outs, 15, dev, seed)
        say()
        say("border fill: %s, fill radius 15 (31 sources), a 16 x 16 grid, mode first + count; tables of up to %.1f px" % (title, amp))
        ta = timed(affine, args.reps)
        line("mosaic (the affine call)", ta)
        line("mosaic, PAPOF_MOSAIC_CULL=0", timed(no_cull(affine), args.reps), ta[0])
        tm = timed(mesh, args.reps)
        line("mosaic_mesh, neighbour_mesh's tables", tm, ta[0])
        line("mosaic_mesh, PAPOF_MOSAIC_CULL=0", timed(no_cull(mesh), args.reps), ta[0])
        tz = timed(zero, args.reps)
        line("mosaic_mesh, tables of zeros", tz, ta[0])
        line("mosaic_mesh, tables of zeros, PAPOF_MOSAIC_CULL=0", timed(no_cull(zero), args.reps), ta[0])
        tc = timed(composed, max(3, args.reps // 2))
        line("31 warp_mesh + torch.where (the same pixels)", tc, ta[0])
        say("  mosaic_mesh is %.2f x the affine call and %.2f x the composition it replaces: it %s the composition"
            % (tm[0] / ta[0], tm[0] / tc[0], "beats" if tm[0] < tc[0] else "does NOT beat"))
        del affine, mesh, zero, composed
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write(rep.getvalue())


if __name__ == "__main__":
    main()
