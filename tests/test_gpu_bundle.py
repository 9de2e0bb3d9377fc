"""Bundle adjustment on device tensors (papteam_opticalflow_amd/tensors.py: bundle_sums, bundle_adjust, link_flows,
panorama_bundle -> papof_bundle_sums_tensor).  Every one of a link's twenty sums must lie within the bound of ANY summation
order of the numpy restatement's terms (tests/_bundle_ref.py: the per-pixel terms are the same operations on both sides), on
the smallest shapes at which the kernels can go wrong; two runs and a link alone or in a batch must give the same bytes; the
device's bundle_adjust must land where the restatement's own driver lands; bundle_adjust and panorama_bundle must be their
parts chained by hand, and a full circle must get the full-circle canvas where panorama_wide raises."""
import math

import numpy as np
import pytest

import _bundle_ref as B

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _links(L, H, W, f, seed, yaw_deg=6.0, noise=0.5):
    """L link rotations a few degrees apart, their exact flows with `noise` px of Gaussian noise and a tenth of the pixels thrown
    up to 6 px, and the rotations the sums are evaluated at (0.3 degrees off): (flows (L, 2, H, W), Rij (L, 3, 3))"""
    Rt = np.stack([B.roll(0.02 * l) @ B.pitch(-0.01 * l) @ B.yaw(math.radians(yaw_deg) * (l + 1)) for l in range(L)])
    flows = np.stack([B.exact_flows([np.eye(3), Rt[l]], [(0, 1)], H, W, f)[0] for l in range(L)])
    flows = B.noisy(flows, noise, 0.1, 6.0, seed)
    return flows, B.perturbed(Rt, 0.3, seed, ref=-1)


def _check(S, flows, Rij, f, occ=None, step=1, scale=1.0, what=""):
    want, mag, n = B.sums_reference(flows, Rij, f, occ, step, scale)
    S = S.cpu().numpy()
    assert S.shape == want.shape
    bound = np.maximum(n - 1, 0)[:, None] * 2.0 ** -53 * mag
    worst = float((np.abs(S - want) / np.where(bound > 0, bound, 1.0)).max())
    print("%s: valid %s, worst |difference| / bound %.3f" % (what, n.tolist(), worst))
    assert (np.abs(S - want) <= bound).all(), (what, np.argwhere(np.abs(S - want) > bound).tolist())
    assert np.array_equal(S[:, 16], n.astype(np.float64)) and (S[:, 18:] == 0).all()
    return n


@pytest.mark.parametrize("H,W,L,step,dtype", [(33, 65, 3, 1, "f64"), (257, 513, 2, 1, "f64"), (33, 65, 3, 2, "f64"),
                                              (33, 65, 3, 3, "f64"), (33, 65, 3, 1, "f32"), (31, 63, 2, 1, "strided")])
def test_sums_are_the_restatements(H, W, L, step, dtype):
    """(33, 65): partial tiles both ways, 4 blocks; (257, 513): 81 blocks, the reduce wave's loop wraps past 64; steps 2 and 3;
    float32 flows; a non-contiguous slice of a larger (L, H, W, 2) tensor"""
    from papteam_opticalflow_amd.tensors import bundle_sums
    f = 0.9 * W
    flows, Rij = _links(L, H, W, f, seed=H + step)
    if dtype == "f32":
        flows = flows.astype(np.float32)
        t = torch.from_numpy(flows).cuda()
    elif dtype == "strided":
        big = torch.zeros((L + 1, H + 3, W + 5, 2), dtype=torch.float64, device="cuda")
        big[1:, 2:H + 2, 4:W + 4] = torch.from_numpy(flows).cuda().permute(0, 2, 3, 1)
        t = big[1:, 2:H + 2, 4:W + 4].permute(0, 3, 1, 2)
        assert not t.is_contiguous()
    else:
        t = torch.from_numpy(flows).cuda()
    S = bundle_sums(t, torch.from_numpy(Rij), f, step=step, scale=1.5)
    n = _check(S, flows, Rij, f, None, step, 1.5, "%d x %d, %d links, step %d, %s" % (H, W, L, step, dtype))
    assert (n > 0.5 * (-(-H // step)) * (-(-W // step))).all()


def test_occlusion_nan_and_inf():
    """an occlusion plane (bool and uint8, channel 0 read, channel 1 ignored), NaN and infinite flows: left out on both sides"""
    from papteam_opticalflow_amd.tensors import bundle_sums
    H, W, L, f = 33, 65, 3, 60.0
    flows, Rij = _links(L, H, W, f, seed=11)
    rng = np.random.default_rng(12)
    occ = (rng.uniform(size=(L, 2, H, W)) < 0.3)
    occ[:, 1] = ~occ[:, 0]
    flows[0, 0, 3, 5] = math.nan
    flows[1, 1, 32, 64] = math.inf
    flows[2, 0, 0, 0] = -math.inf
    flows[2, :, 10:20, 10:30] = math.nan
    t = torch.from_numpy(flows).cuda()
    n0 = _check(bundle_sums(t, torch.from_numpy(Rij), f), flows, Rij, f, what="NaN and inf")
    for mask in (torch.from_numpy(occ).cuda(), torch.from_numpy(occ.astype(np.uint8) * 7).cuda()):
        n1 = _check(bundle_sums(t, torch.from_numpy(Rij), f, occlusion=mask), flows, Rij, f, occ, what="occlusion %s" % mask.dtype)
    assert (n1 < 0.8 * n0).all() and (n1 > 0).all()


def test_the_horizon_of_a_link():
    """yaw 80 degrees at f = 40 on 20 x 30: qz = cos 80 -+ sin 80 * px runs from -0.18 to 0.53, so part of the frame lies at or
    behind qz = 0.0625 and is left out, whatever its flow; next to it a link in front of its horizon and one wholly behind"""
    from papteam_opticalflow_amd.tensors import bundle_sums
    H, W, f = 20, 30, 40.0
    rng = np.random.default_rng(3)
    flows = rng.uniform(-2, 2, (3, 2, H, W))
    Rij = np.stack([B.yaw(math.radians(80)), B.yaw(math.radians(5)), B.yaw(math.radians(170))])
    n = _check(bundle_sums(torch.from_numpy(flows).cuda(), torch.from_numpy(Rij), f), flows, Rij, f, what="horizon")
    inside = lambda fl: int(((fl[0] + np.arange(W) >= 0) & (fl[0] + np.arange(W) <= W - 1) &  # noqa: E731
                             (fl[1] + np.arange(H)[:, None] >= 0) & (fl[1] + np.arange(H)[:, None] <= H - 1)).sum())
    assert 0 < n[0] < inside(flows[0]) and n[1] == inside(flows[1]) and n[2] == 0


def test_two_runs_and_a_link_alone_give_the_same_bytes():
    from papteam_opticalflow_amd.tensors import bundle_sums
    H, W, L, f = 257, 513, 3, 400.0
    flows, Rij = _links(L, H, W, f, seed=21)
    t, r = torch.from_numpy(flows).cuda(), torch.from_numpy(Rij)
    a, b = bundle_sums(t, r, f, step=2), bundle_sums(t, r, f, step=2)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for l in range(L):
        alone = bundle_sums(t[l:l + 1], r[l:l + 1], f, step=2)
        assert torch.equal(alone.view(torch.int64), a[l:l + 1].view(torch.int64)), l


# ---- the adjustment
@pytest.fixture(scope="module")
def noisy_ring():
    Rs, links, flows = B.ring()
    return Rs, links, B.noisy(flows), B.perturbed(Rs, 0.2)


def test_device_bundle_adjust_lands_where_the_restatements_driver_lands(noisy_ring):
    """the noisy ring (18 frames of 48 x 80, f = 120 started 10 % short): the device's bundle_adjust against tests/_bundle_ref.py's
    own driver over the restatement's sums -- the same accepted steps, the frame corners within 1e-8 px (the figure
    tests/test_gpu_homography.py uses for the same kind of comparison) and the focal length within 1e-10"""
    from papteam_opticalflow_amd.tensors import bundle_adjust
    Rs, links, flows, R0 = noisy_ring
    H, W, f = 48, 80, 120.0
    b = bundle_adjust(torch.from_numpy(flows).cuda(), links, torch.from_numpy(R0), 0.9 * f, iters=10)
    R, f1, cost, accepted = B.adjust_reference(lambda Rij, fk: B.sums_reference(flows, Rij, fk)[0], links, R0, 0.9 * f, iters=10)
    d = B.corner_error(b.rotations.cpu().numpy(), R, f, H, W)
    print("device against the restatement's driver: corners %.3g px, focal %.3g, accepted %s / %s, to the truth %.3g px" %
          (d, abs(b.focal - f1), b.accepted.astype(int), accepted.astype(int), B.corner_error(b.rotations.cpu().numpy(), Rs, f, H, W)))
    assert np.array_equal(b.accepted, accepted) and b.ok and b.rotations.is_cuda
    assert d < 1e-8 and abs(b.focal - f1) < 1e-10 * f
    print("cost histories differ by at most %.3g relative" % float(np.abs(b.cost / cost - 1).max()))


def test_bundle_adjust_is_the_host_solver_over_bundle_sums(noisy_ring):
    """byte for byte: bundle_solve driven by bundle_sums by hand, with a mask, step 2 and another scale"""
    from papteam_opticalflow_amd.tensors import bundle_adjust, bundle_solve, bundle_sums
    Rs, links, flows, R0 = noisy_ring
    t = torch.from_numpy(flows.astype(np.float32)).cuda()
    occ = torch.from_numpy(np.random.default_rng(5).uniform(size=flows.shape) < 0.1).cuda()
    b = bundle_adjust(t, links, torch.from_numpy(R0), 125.0, occlusion=occ, iters=4, scale=2.0, step=2, ref=3, fix_focal=True)

    def evaluate(Rij, fk):
        return bundle_sums(t, torch.from_numpy(np.ascontiguousarray(Rij)), fk, occlusion=occ, step=2, scale=2.0).cpu().numpy()
    R, f1, cost, accepted, S = bundle_solve(evaluate, links, R0, 125.0, iters=4, ref=3, fix_focal=True)
    assert b.focal == f1 == 125.0 and np.array_equal(b.rotations.cpu().numpy(), R) and np.array_equal(b.rotations[3].cpu().numpy(), R0[3])
    assert np.array_equal(b.cost, cost) and np.array_equal(b.accepted, accepted)
    assert np.array_equal(b.support, S[:, 15] / (24 * 40))


# ---- the panorama
@pytest.fixture(scope="module")
def small_ring():
    frames, Rs, f, tex = B.ring_scene()
    return torch.from_numpy(frames).cuda(), Rs, f


def test_link_flows_start_from_the_rotations(small_ring):
    """a pair three frames (30 px) apart on frames 80 px wide at TWO pyramid levels: from the rotations' flow the solver is
    within a pixel of the exact flow over the pixels the forward-backward check keeps; from zero it is not"""
    from papteam_opticalflow_amd.tensors import flow_pairs_fb, link_flows
    v, Rs, f = small_ring
    links = np.array([[0, 3], [10, 13], [46, 47]])
    fb = link_flows(v, links, torch.from_numpy(Rs), f, 2, layout="NHWC")
    assert tuple(fb.flow_fw.shape) == (3, 2, 48, 80) and fb.occlusion.dtype == torch.bool
    exact = B.exact_flows(Rs, links, 48, 80, f)
    keep = ~fb.occlusion[:, 0].cpu().numpy() & np.isfinite(exact).all(1)
    err = np.hypot(*(fb.flow_fw.cpu().numpy() - exact).transpose(1, 0, 2, 3))
    zero = flow_pairs_fb(v[links[:, 0]], v[links[:, 1]], 2, layout="NHWC")
    err0 = np.hypot(*(zero.flow_fw.cpu().numpy() - exact).transpose(1, 0, 2, 3))
    print("link flows at 2 levels: median error %.3f px from the rotations, %.3f px from zero; kept %.2f" %
          (np.median(err[keep]), np.median(err0[keep]), keep.mean()))
    assert np.median(err[keep]) < 1.0 and np.median(err0[:2][keep[:2]]) > 5.0 and keep.mean() > 0.3


@pytest.fixture(scope="module")
def ring():
    """the ring that tests/test_bundle_cpu.py follows with the oracle's flows: 48 frames of 96 x 160 at 7.5 degrees, 20 px per
    frame, which the solver follows at 8 levels (on the 48 x 80 ring it does not at any: its chain comes out at 265 to 311 of
    the 352.5 degrees, under or barely at a full circle with the field of view; here it is 328, 383 with the field of view)"""
    frames, Rs, f, tex = B.ring_scene(48, 96, 160, 1)
    return torch.from_numpy(frames).cuda(), Rs, f


def test_panorama_bundle_is_its_composition_and_returns_the_full_circle(ring):
    """the ring (48 frames of 96 x 160 over 360 degrees) at 8 levels with the focal length given: panorama_bundle returns the
    bytes of the public calls chained by hand and a canvas of round(2 pi f) columns; panorama_wide raises on the same
    frames"""
    from papteam_opticalflow_amd.tensors import (bundle_adjust, bundle_links, bundle_transforms, chain_rotations, flow_video,
                                                 global_homography, link_flows, mosaic_rays, panorama_bundle, panorama_wide)
    v, Rs, f = ring
    T, H, W = 48, 96, 160
    with pytest.raises(ValueError, match="spans"):
        panorama_wide(v, 8, focal=f, layout="NHWC")
    p = panorama_bundle(v, 8, focal=f, ref=0, layout="NHWC", bundle_iters=6)
    flow, _, _ = flow_video(v, 8, layout="NHWC")
    assert torch.equal(flow, p.flow)
    mo = global_homography(flow)
    assert torch.equal(mo.motion, p.motion) and torch.equal(mo.ok, p.ok)
    chain = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    R1 = bundle_adjust(flow, chain, chain_rotations(mo, (H, W), f, ref=0), f, iters=6, ref=0, fix_focal=True).rotations
    links = bundle_links(R1, (H, W), f)
    assert np.array_equal(links, p.links)
    near = links[:, 1] == links[:, 0] + 1
    far = link_flows(v, links[~near], R1, f, 2, layout="NHWC")
    flows = torch.empty((len(links), 2, H, W), dtype=torch.float64, device="cuda")
    occ = torch.zeros((len(links), 2, H, W), dtype=torch.bool, device="cuda")
    at = torch.from_numpy(near).cuda()
    flows[at], flows[~at], occ[~at] = flow[torch.from_numpy(links[near, 0]).cuda()], far.flow_fw, far.occlusion
    b = bundle_adjust(flows, links, R1, f, occlusion=occ, iters=6, ref=0)
    assert torch.equal(b.rotations, p.rotations) and b.focal == p.focal and np.array_equal(b.cost, p.cost)
    M, cols, rows, size, origin = bundle_transforms(b.rotations, (H, W), b.focal, ref=0)
    assert torch.equal(M[0], p.matrices) and torch.equal(cols, p.cols) and torch.equal(rows, p.rows) and origin == p.origin
    assert size[1] == round(2 * math.pi * b.focal) and tuple(p.image.shape) == size + (3,)
    mo_ = mosaic_rays(v, torch.arange(T)[None], M, cols, rows, mode="median", layout="NHWC")
    assert torch.equal(mo_.out[0], p.image) and torch.equal(mo_.count[0], p.count)
    inner = slice(size[0] // 4, size[0] - size[0] // 4)
    cnt = p.count.cpu().numpy()[inner]
    closing = [tuple(int(x) for x in l) for l in links if l[1] - l[0] > T // 2]
    print("panorama_bundle on the ring: %d links (closing: %s), focal %.3f of %.3f, %d x %d canvas, count %d .. %d, corners %.2f "
          "px from the truth" % (len(links), closing, p.focal, f, size[1], size[0], cnt.min(), cnt.max(),
                                 B.corner_error(p.rotations.cpu().numpy(), Rs, f, H, W)))
    assert cnt.min() >= 1  # every column of the circle is covered
