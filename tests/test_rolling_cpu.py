"""CPU-side checks of rolling-shutter rectification (papteam_opticalflow_amd/tensors.py: rectify_frames, rectify_flows,
rectify_video, stabilize_video_rs; include/papof.h: papof_rs_rectify_tensor, papof_rs_flow_tensor): known answers of the
numpy fp64 restatement in tests/_rolling_ref.py that tests/test_gpu_rolling.py compares the device's output with -- a camera
of constant velocity, where the rule is exact; a shaking camera with exact flows, measured in world points; pictures cut
from the committed 960 x 540 frame with exact flows and with the oracle's; the identities at readout = 0 and H = 1 --, every
Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.
No device is touched here."""
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _interp_ref import as_f64  # noqa: E402
from _rolling_ref import flows_reference, rectify_reference  # noqa: E402
from _stab_ref import warp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import rectify_flows, rectify_frames, rectify_video, stabilize_video_rs  # noqa: E402

H_SCENE, W_SCENE = 96, 160


# ---- a translating camera: the image position of the world point w at time s is w - c(s), and row y of frame t is exposed
# at t + tau(y), tau(y) = readout * (y - a) / H
def _tau(y, readout, anchor, H):
    return (readout / H) * (y - anchor * (H - 1))


def exact_flows(c, T, H, W, readout, anchor=0.5):
    """the flows of the rolling-shutter video of a camera at c(s) (s -> (.., 2)), solved per row -- under a translation the
    flow depends on the row alone --: P' + c(t' + tau(P'_y)) = P + c(t + tau(P_y)), 60 fixed-point iterations (the
    contraction is |readout| |c_y'| / H, a few per cent)"""
    y = np.arange(H, dtype=np.float64)
    tau = lambda yy: _tau(yy, readout, anchor, H)  # noqa: E731

    def flow(t, dt):
        d = np.zeros((H, 2))
        for _ in range(60):
            d = c(t + tau(y)) - c(t + dt + tau(y + d[:, 1]))
        return np.broadcast_to(d.T[:, :, None], (2, H, W))

    fw = np.stack([flow(t, 1) for t in range(T - 1)])
    bw = np.stack([flow(t + 1, -1) for t in range(T - 1)])
    return fw, bw


def world_errors(c, P, valid, readout, anchor=0.5, frames=None):
    """(RMS distance between the world point that rectified pixel q shows -- the sensor's P_iters(q), exposed at its own
    row's time -- and the one the global-shutter frame shows there, the same for the unrectified video: P = q), over the
    valid pixels of `frames` (default: the interior ones)"""
    T, H, W, _ = P.shape
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    e, e0 = [], []
    for t in frames if frames is not None else range(1, T - 1):
        ok = valid[t]
        q = np.stack([x[ok], r[ok]], -1)
        p = P[t][ok]
        e.append(p + c(t + _tau(p[:, 1], readout, anchor, H)) - (q + c(float(t))))
        e0.append(c(t + _tau(q[:, 1], readout, anchor, H)) - c(float(t)))
    e, e0 = np.concatenate(e), np.concatenate(e0)
    return float(np.sqrt((e ** 2).sum(1).mean())), float(np.sqrt((e0 ** 2).sum(1).mean()))


# ---- 1. constant velocity: the parabola is a line and the rule is exact
V = np.array([5.0, -3.0])  # the camera's velocity in pixels per frame


@pytest.mark.parametrize("readout", [0.8, -0.7])
def test_constant_velocity_is_exact(readout):
    T, H, W = 3, H_SCENE, W_SCENE  # an end frame of each kind and an interior one
    r, a = readout / H, 0.5 * (H - 1)
    F = -V / (1.0 + r * V[1])  # F = -v (1 + r F_y): the landing row has its own delay
    fw = np.broadcast_to(F[None, :, None, None], (T - 1, 2, H, W)).copy()
    bw = -fw
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Py = (yy + r * V[1] * a) / (1.0 + r * V[1])  # P = q - v tau(P_y)
    exact = np.stack([xx - V[0] * (r * (Py - a)), Py], -1)
    frames = np.zeros((T, H, W, 1))
    err = {}
    for iters in (1, 2, 3, 8):
        _, valid, P, _ = rectify_reference(frames, fw, bw, readout, iters=iters, parts=True)
        assert valid.mean() > 0.9
        err[iters] = float(np.hypot(*np.moveaxis(P - exact, -1, 0))[valid].max())
    print("readout %s: |P_iters - exact| max over valid pixels: %s; contraction |r| |v| = %.4f"
          % (readout, {k: "%.2e" % v for k, v in err.items()}, abs(r) * np.hypot(*V)))
    assert err[8] <= 1e-9
    assert err[2] <= err[1] / 10 and err[3] <= err[2] / 10
    gfw, gbw = flows_reference(fw, bw, readout, iters=8)
    for g, want in ((gfw, -V), (gbw, V)):  # the global-shutter flow of a scene that moves by -v per frame
        ok = ~np.isnan(g[:, 0])
        assert ok.mean() > 0.85 and (np.isnan(g[:, 1]) == ~ok).all()
        assert np.abs(g[:, 0][ok] - want[0]).max() <= 1e-9 and np.abs(g[:, 1][ok] - want[1]).max() <= 1e-9


# ---- 2. shake: drift plus two sinusoids, exact flows, the error in world points
def shaking_camera(periods, amp=6.0, seed=0):
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, (len(periods), 2))
    am = rng.uniform(0.5, 1, (len(periods), 2)) * amp

    def c(s):
        s = np.asarray(s, np.float64)[..., None]
        return sum(am[i] * np.sin(2 * np.pi * s / periods[i] + ph[i]) for i in range(len(periods))) + np.array([3.0, 1.0]) * s
    return c


SHAKES = {(12.0, 7.0): 0.2, (9.0, 4.3): 0.5}  # the sinusoids' periods in frames -> the cap on the ratio to the unrectified error


@pytest.mark.parametrize("readout", [0.5, 0.9])
@pytest.mark.parametrize("periods", sorted(SHAKES))
def test_shake_with_exact_flows(periods, readout):
    """Twelve frames of 96 rows under a drift of (3, 1) px per frame plus two sinusoids of 3 .. 6 px per axis, exact flows,
    3 iterations; the RMS distance in world points over the valid pixels of the interior frames, measured here:
        periods 12 and 7:    readout 0.5: 0.083 px of 0.932 unrectified (0.089)    readout 0.9: 0.135 of 1.653 (0.082)
        periods 9 and 4.3:   readout 0.5: 0.312 px of 1.204 (0.259)                readout 0.9: 0.513 of 2.111 (0.243)
    The caps are about twice these ratios.  A period of 4.3 frames is close to what three samples one frame apart can
    follow; at periods 6 and 3.1, near half the frame rate, the same scene leaves 0.41 .. 0.44 of the error (not asserted)."""
    T, H, W = 12, H_SCENE, 24
    c = shaking_camera(periods)
    fw, bw = exact_flows(c, T, H, W, readout)
    _, valid, P, _ = rectify_reference(np.zeros((T, H, W, 1)), fw, bw, readout, iters=3, parts=True)
    assert valid[1:-1].mean() > 0.8
    e, e0 = world_errors(c, P, valid, readout)
    print("periods %s readout %s: world-point RMS %.4f px rectified, %.4f px unrectified, ratio %.3f (cap %.1f); valid %.3f"
          % (periods, readout, e, e0, e / e0, SHAKES[periods], valid[1:-1].mean()))
    assert e <= SHAKES[periods] * e0


# ---- 3. pictures: frames cut from the committed 960 x 540 frame, each row at its own camera offset
T_PIC, READOUT_PIC, PERIODS_PIC, ORIGIN = 8, 0.9, (12.0, 7.0), (400.0, 200.0)  # ORIGIN: the window's (column, row) at c = 0
CAP = 99.0  # dB: the PSNR written for identical bytes


def _render(img, X, Y):
    """img (h, w, 3) float64 sampled bilinearly at the points (X, Y), rounded to uint8"""
    x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
    fx, fy = (X - x0)[..., None], (Y - y0)[..., None]
    v = (img[y0, x0] * (1 - fx) + img[y0, x0 + 1] * fx) * (1 - fy) + (img[y0 + 1, x0] * (1 - fx) + img[y0 + 1, x0 + 1] * fx) * fy
    return np.rint(v).astype(np.uint8)


def picture_scene():
    """(the camera c, the rolling-shutter video (T, H, W, 3) uint8 -- pixel (x, y) of frame t shows the picture at ORIGIN +
    (x, y) + c(t + tau(y)) --, the global-shutter video -- at ORIGIN + (x, y) + c(t) --, the exact flows)"""
    import cases
    img = cases.load_frame_u8("960", 1).astype(np.float64)
    T, H, W = T_PIC, H_SCENE, W_SCENE
    c = shaking_camera(PERIODS_PIC)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rolling, glob = [], []
    for t in range(T):
        cr, cg = c(t + _tau(yy, READOUT_PIC, 0.5, H)), c(float(t))
        rolling.append(_render(img, ORIGIN[0] + xx + cr[..., 0], ORIGIN[1] + yy + cr[..., 1]))
        glob.append(_render(img, ORIGIN[0] + xx + cg[0], ORIGIN[1] + yy + cg[1]))
    return (c, np.stack(rolling), np.stack(glob)) + exact_flows(c, T, H, W, READOUT_PIC)


def psnr(video, truth, valid):
    """PSNR in dB over the valid pixels of the interior frames, CAP for identical bytes"""
    d = (as_f64(video) - as_f64(truth))[1:-1][valid[1:-1]]
    err = float((d * d).mean())
    return CAP if err == 0 else min(CAP, -10.0 * math.log10(err))


def oracle_flows(frames, levels=4):
    """flow_video_fb with the oracle: pair i from frame i to i + 1 and back"""
    from _libs import OracleLib, build_oracle
    build_oracle()
    L = OracleLib()
    f = as_f64(frames)
    fw = np.stack([np.stack(L.coarse2fine_flow(f[i], f[i + 1], levels)[:2]) for i in range(len(f) - 1)])
    bw = np.stack([np.stack(L.coarse2fine_flow(f[i + 1], f[i], levels)[:2]) for i in range(len(f) - 1)])
    return fw, bw


# measured by test_pictures: PSNR in dB of the unrectified video, rectified with exact flows, with the oracle's flows
PICTURES_MEASURED = (17.97, 31.15, 27.58)


def pictures_bar():
    """the least PSNR with estimated flows: halfway between the unrectified video's and the one measured with the oracle's
    flows -- the slack is for the device's flows differing from the oracle's"""
    return 0.5 * (PICTURES_MEASURED[0] + PICTURES_MEASURED[2])


def test_pictures():
    """Eight frames of 96 x 160 cut from the committed 960 x 540 frame under the shake of periods 12 and 7 frames, readout
    0.9, each row rendered at its own camera offset; PSNR in dB against the global-shutter render over the pixels of the
    interior frames that are valid with both sets of flows (0.964 of them), measured here on the restatement:
        unrectified 17.97     exact flows 31.15     the oracle's flows (4 levels) 27.58
    The oracle's flows are off by 0.22 px on average (the rows' shear is below its smoothness prior); the world-point RMS
    error with them is 0.34 px of 1.60 px unrectified.  The exact-flow figure is the resampling's own loss (two bilinear
    renders of an 8-bit picture).  Bar for estimated flows: halfway between the unrectified figure and the oracle's."""
    c, rolling, glob, fw, bw = picture_scene()
    exact, valid = rectify_reference(rolling, fw, bw, READOUT_PIC)
    ofw, obw = oracle_flows(rolling)
    est, evalid, P, _ = rectify_reference(rolling, ofw, obw, READOUT_PIC, parts=True)
    both = valid & evalid
    got = (psnr(rolling, glob, both), psnr(exact, glob, both), psnr(est, glob, both))
    e, e0 = world_errors(c, P, evalid, READOUT_PIC)
    print("pictures: unrectified %.2f dB, exact flows %.2f dB, oracle's flows %.2f dB (bar %.2f dB) over %.3f of the interior "
          "pixels; oracle flow error %.3f px; world-point RMS with the oracle's flows %.3f px of %.3f px unrectified"
          % (*got, pictures_bar(), both[1:-1].mean(), np.abs(ofw - fw).mean(), e, e0))
    assert both[1:-1].mean() > 0.9
    assert got[1] > got[0]
    assert np.allclose(got, PICTURES_MEASURED, rtol=0, atol=0.05), (got, PICTURES_MEASURED)
    assert got[2] >= pictures_bar()


# ---- 4. identities on the restatement
def _random_flows(T, H, W, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    return rng.normal(0, scale, (T - 1, 2, H, W)), rng.normal(0, scale, (T - 1, 2, H, W))


def _some_matrices(T, H, W, seed):
    rng = np.random.default_rng(seed)
    M = np.tile(np.eye(2, 3), (T, 1, 1)) + rng.normal(0, 0.03, (T, 2, 3))
    M[:, :, 2] += rng.normal(0, 2.0, (T, 2))
    return M


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_readout_zero_returns_the_frames_and_with_matrices_the_affine_warp(dtype):
    T, H, W, C = 3, 24, 37, 3
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (T, H, W, C)).astype(np.uint8) if dtype == np.uint8 else rng.random((T, H, W, C)).astype(dtype)
    if dtype == np.uint8:
        frames.reshape(-1)[:256] = np.arange(256)  # every byte value occurs
    fw, bw = _random_flows(T, H, W, 2)
    fw[0, :, 3, 4], bw[1, :, 5, 6] = math.nan, math.inf  # no flow is read
    for anchor in (0.0, 0.5, 1.0):
        video, valid, P, seen = rectify_reference(frames, fw, bw, 0.0, anchor, 3, parts=True)
        assert video.dtype == dtype and video.tobytes() == frames.tobytes() and valid.all()
        assert seen["s_zero"] == 3 * T * H * W and sum(seen.values()) == seen["s_zero"]
        assert (P[..., 0] == np.arange(W)).all() and (P[..., 1] == np.arange(H)[:, None]).all()
    M = _some_matrices(T, H, W, 3)
    M[1, 0, 0] = math.nan
    for mdt in (np.float64, np.float32):
        for odt in (None, np.uint8, np.float32, np.float64):
            video, valid = rectify_reference(frames, fw, bw, 0.0, 0.5, 3, M.astype(mdt), odt)
            want, wvalid = warp_reference(frames, M.astype(mdt), dtype if odt is None else odt)
            assert video.dtype == want.dtype and video.tobytes() == want.tobytes() and (valid == wvalid).all()
            assert valid.any() and not valid[1].any() and not valid.all()


def test_rectified_flows_at_readout_zero_are_the_flows_where_they_land_in_the_image():
    T, H, W = 4, 20, 31
    fw, bw = _random_flows(T, H, W, 4, 6.0)  # finite: a NaN neighbour would enter a sample through its zero weight
    fw[0, 0, :4, :4] = 900.0
    r, x = np.mgrid[0:H, 0:W].astype(np.float64)
    for dt in (np.float64, np.float32):
        gfw, gbw = flows_reference(fw.astype(dt), bw.astype(dt), 0.0, out_dtype=dt)
        for g, f in ((gfw, fw.astype(dt)), (gbw, bw.astype(dt))):
            X, Y = x + f[:, 0].astype(np.float64), r + f[:, 1].astype(np.float64)
            inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
            assert g.dtype == dt and inside.any() and (~inside).any()
            assert (g[:, 0][inside] == f[:, 0][inside]).all() and (g[:, 1][inside] == f[:, 1][inside]).all()
            assert np.isnan(g[:, 0][~inside]).all() and np.isnan(g[:, 1][~inside]).all()


def test_one_row_is_the_identity():
    """H = 1: a = 0 and the one row is the anchor row, whatever readout and anchor are"""
    T, W = 3, 17
    frames = np.random.default_rng(5).random((T, 1, W, 2))
    fw, bw = _random_flows(T, 1, W, 6)
    for readout, anchor in ((1.0, 0.0), (-0.7, 0.5), (0.3, 1.0)):
        video, valid = rectify_reference(frames, fw, bw, readout, anchor, 8)
        assert video.tobytes() == frames.tobytes() and valid.all()


def test_the_end_frames_read_one_flow_and_the_anchor_row_none():
    T, H, W = 4, 21, 16
    frames = np.random.default_rng(7).random((T, H, W, 1))
    fw, bw = _random_flows(T, H, W, 8, 1.0)
    video, valid = rectify_reference(frames, fw, bw, 0.8)
    fw2, bw2 = fw.copy(), bw.copy()
    bw2[0], fw2[T - 2] = math.nan, math.nan  # frame 0 has no use for a backward flow, frame T - 1 none for a forward one
    v2, k2 = rectify_reference(frames, fw2, bw2, 0.8)
    assert v2[[0, T - 1]].tobytes() == video[[0, T - 1]].tobytes() and (k2[[0, T - 1]] == valid[[0, T - 1]]).all()
    assert not k2[1, :9].any() and not k2[1, 11:].any() and not k2[T - 2, :9].any()  # the interior frames need both
    a = (H - 1) // 2  # the anchor row of anchor = 0.5: s == 0, nothing is read
    assert k2[:, a].all() and v2[:, a].tobytes() == frames[:, a].tobytes()


# ---- 5. Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_V = lambda: _z(5, 3, 8, 8)  # noqa: E731
_F = lambda: _z(4, 2, 8, 8)  # noqa: E731


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: rectify_frames(_V(), _F(), _F(), 0.8), ValueError),                                # CPU tensors
    (lambda: rectify_frames(None, _F(), _F(), 0.8), TypeError),
    (lambda: rectify_flows(_F(), _F(), 0.8), ValueError),
    (lambda: rectify_flows(None, _F(), 0.8), TypeError),
    (lambda: rectify_video(_V(), 2, 0.8), ValueError),
    (lambda: rectify_video(None, 2, 0.8), TypeError),
    (lambda: stabilize_video_rs(_V(), 2, 0.8), ValueError),
    (lambda: stabilize_video_rs(None, 2, 0.8), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_SHUTTER = [
    (dict(readout=1.5), ValueError), (dict(readout=-1.01), ValueError), (dict(readout=math.nan), ValueError),
    (dict(readout=math.inf), ValueError), (dict(readout="0.8"), TypeError), (dict(readout=None), TypeError),
    (dict(readout=True), TypeError),
    (dict(anchor=-0.1), ValueError), (dict(anchor=1.1), ValueError), (dict(anchor=math.nan), ValueError),
    (dict(anchor=None), TypeError), (dict(anchor=False), TypeError),
]
_SOLVE = [(dict(iters=0), ValueError), (dict(iters=9), ValueError), (dict(iters=2.0), ValueError), (dict(iters=True), ValueError),
          (dict(iters=None), ValueError)]
_COMMON = [
    (dict(layout="CHWN"), ValueError),
    (dict(frames=_z(5, 5, 8, 8)), ValueError), (dict(frames=_z(5, 8, 8, 5), layout="NHWC"), ValueError),   # channels
    (dict(frames=_z(5, 0, 8, 8)), ValueError), (dict(frames=_z(5, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(frames=_z(1, 3, 8, 8)), ValueError),                                                          # one frame
    (dict(frames=_z(8, 8)), ValueError), (dict(frames=np.zeros((5, 3, 8, 8))), TypeError),
    (dict(frames=_z(5, 3, 8, 8, device="meta")), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),
    (dict(bogus=1), TypeError),
]
_FLOWS = [
    (dict(flow_fw=_z(4, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_bw=_z(4, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(4, 3, 8, 8), flow_bw=_z(4, 3, 8, 8)), ValueError), (dict(flow_bw=_z(4, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError), (dict(flow_bw=np.zeros((4, 2, 8, 8))), TypeError),
    (dict(flow_fw=_z(4, 2, 8, 8, device="meta"), flow_bw=_z(4, 2, 8, 8, device="meta")), ValueError),
    (dict(flow_bw=_z(4, 2, 8, 8, device="meta")), ValueError),
]
_FRAME_FLOWS = [
    (dict(frames=_z(4, 3, 8, 8)), ValueError),                                                          # 3 pairs, 4 given
    (dict(flow_fw=_z(4, 2, 8, 9), flow_bw=_z(4, 2, 8, 9)), ValueError),
    (dict(flow_fw=_z(5, 2, 8, 8), flow_bw=_z(5, 2, 8, 8)), ValueError),
]
_MATRICES = [
    (dict(matrices=_z(5, 3, 3)), ValueError), (dict(matrices=_z(4, 2, 3)), ValueError), (dict(matrices=_z(2, 3)), ValueError),
    (dict(matrices=_z(5, 2, 3, dtype=torch.float16)), TypeError), (dict(matrices=np.zeros((5, 2, 3))), TypeError),
    (dict(matrices=_z(5, 2, 3, device="meta")), ValueError),
]
_FIT = [
    (dict(model="projective"), ValueError), (dict(radius=-1), ValueError), (dict(radius=1.5), ValueError),
    (dict(crop=0.0), ValueError), (dict(crop=1.5), ValueError), (dict(crop="1"), TypeError),
    (dict(iters=0), ValueError), (dict(scale=0.0), ValueError), (dict(scale=None), TypeError),
    (dict(rs_iters=0), ValueError), (dict(rs_iters=9), ValueError), (dict(rs_iters=1.0), ValueError),
]
_CONSISTENCY = [(dict(consistency=(0.1,)), TypeError), (dict(consistency=(-0.1, 0.5)), ValueError), (dict(consistency=0.5), TypeError)]


@pytest.mark.parametrize("kw,exc", _COMMON + _SHUTTER + _SOLVE + _FLOWS + _FRAME_FLOWS + _MATRICES)
def test_rectify_frames_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), flow_fw=_F(), flow_bw=_F(), readout=0.8)
    args.update(kw)
    with pytest.raises(exc):
        rectify_frames(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), args.pop("readout"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _SHUTTER + _SOLVE + _FLOWS + [
    (dict(out_dtype=torch.uint8), TypeError), (dict(out_dtype=torch.float16), TypeError), (dict(layout="NHWC"), TypeError),
    (dict(flow_fw=_z(2, 8, 8), flow_bw=_z(2, 8, 8)), ValueError), (dict(flow_fw=_z(4, 2, 0, 8), flow_bw=_z(4, 2, 0, 8)), ValueError)])
def test_rectify_flows_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(flow_fw=_F(), flow_bw=_F(), readout=0.8)
    args.update(kw)
    with pytest.raises(exc):
        rectify_flows(args.pop("flow_fw"), args.pop("flow_bw"), args.pop("readout"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _SHUTTER + _SOLVE + _CONSISTENCY + [(dict(levels=0), ValueError)])
def test_rectify_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, levels, readout = kw.pop("frames", _V()), kw.pop("levels", 2), kw.pop("readout", 0.8)
    with pytest.raises(exc):
        rectify_video(frames, levels, readout, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _SHUTTER + _FIT + _CONSISTENCY + [(dict(levels=0), ValueError)])
def test_stabilize_video_rs_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, levels, readout = kw.pop("frames", _V()), kw.pop("levels", 2), kw.pop("readout", 0.8)
    with pytest.raises(exc):
        stabilize_video_rs(frames, levels, readout, **kw)
    assert stub == []


def test_the_defaults():
    for f in (rectify_frames, rectify_flows, rectify_video):
        assert f.__kwdefaults__["anchor"] == 0.5 and f.__kwdefaults__["iters"] == 3
    assert stabilize_video_rs.__kwdefaults__["anchor"] == 0.5 and stabilize_video_rs.__kwdefaults__["rs_iters"] == 3
    assert tensors.MAX_RS_ITERS == 8


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(192, 24, 3, 1), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
_P = (64, 8, 1, 0)       # a (frame, row, column) plane of 8 x 8
_FS = (128, 8, 1, 64)    # a flow (pair, row, column, component) of 8 x 8


def _rect(lib, h, n=4, size=(8, 8, 3), fr=_OK, fw=_OK, bw=_OK, mat=None, out=_OK, valid=_OK, readout=0.8, anchor=0.5, iters=3):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "fw": lambda: _t(strides=_FS), "bw": lambda: _t(capi.DTYPE_F32, _FS),
            "mat": lambda: _t(strides=(6, 3, 1, 0)), "out": lambda: _t(capi.DTYPE_U8, data=0x9000),
            "valid": lambda: _t(capi.DTYPE_U8, _P)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, fw=fw, bw=bw, mat=mat, out=out, valid=valid).items()}
    return lib.papof_rs_rectify_tensor(h, n, size[0], size[1], size[2], _ref(d["fr"]), _ref(d["fw"]), _ref(d["bw"]), readout,
                                       anchor, iters, _ref(d["mat"]), _ref(d["out"]), _ref(d["valid"]), None)


def _rflow(lib, h, n=4, size=(8, 8), fw=_OK, bw=_OK, ofw=_OK, obw=_OK, readout=0.8, anchor=0.5, iters=3):
    make = {"fw": lambda: _t(strides=_FS), "bw": lambda: _t(capi.DTYPE_F32, _FS), "ofw": lambda: _t(strides=_FS, data=0x9000),
            "obw": lambda: _t(capi.DTYPE_F32, _FS, data=0xa000)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fw=fw, bw=bw, ofw=ofw, obw=obw).items()}
    return lib.papof_rs_flow_tensor(h, n, size[0], size[1], _ref(d["fw"]), _ref(d["bw"]), readout, anchor, iters, _ref(d["ofw"]),
                                    _ref(d["obw"]), None)


_RULE_REFUSALS = [
    dict(fw=None), dict(bw=None), dict(fw=_t(strides=_FS, data=0)), dict(bw=_t(strides=_FS, data=0)),    # NULL
    dict(fw=_t(capi.DTYPE_U8, _FS)), dict(bw=_t(7, _FS)), dict(fw=_t(-1, _FS)),                          # dtypes
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))), dict(fw=_t(strides=(-128, 8, 1, 64))),
    dict(n=1), dict(n=0), dict(n=-4),                                                                   # sizes
    dict(readout=1.0000001), dict(readout=-1.5), dict(readout=math.nan), dict(readout=math.inf), dict(readout=-math.inf),
    dict(anchor=-1e-9), dict(anchor=1.0000001), dict(anchor=math.nan), dict(anchor=math.inf),
    dict(iters=0), dict(iters=9), dict(iters=-1),
]


@pytest.mark.parametrize("kw", _RULE_REFUSALS + [
    dict(fr=None), dict(out=None), dict(fr=_t(data=0)), dict(out=_t(capi.DTYPE_U8, data=0)),            # NULL
    dict(valid=_t(capi.DTYPE_U8, _P, data=0)), dict(mat=_t(strides=(6, 3, 1, 0), data=0)),
    dict(fr=_t(dtype=3)), dict(fr=_t(dtype=-1)), dict(out=_t(3, data=0x9000)), dict(out=_t(-1, data=0x9000)),  # dtypes
    dict(valid=_t(capi.DTYPE_F32, _P)), dict(mat=_t(capi.DTYPE_U8, (6, 3, 1, 0))), dict(mat=_t(3, (6, 3, 1, 0))),
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr=_t(strides=(192, 24, 3, -1))),                      # negative strides
    dict(out=_t(capi.DTYPE_U8, (192, -24, 3, 1), data=0x9000)), dict(valid=_t(capi.DTYPE_U8, (64, 8, -1, 0))),
    dict(mat=_t(strides=(6, -3, 1, 0))), dict(mat=_t(strides=(-6, 3, 1, 0))),
    dict(out=_t(capi.DTYPE_U8, (0, 24, 3, 1), data=0x9000)), dict(out=_t(capi.DTYPE_U8, (192, 0, 3, 1), data=0x9000)),  # zero
    dict(out=_t(capi.DTYPE_U8, (192, 24, 0, 1), data=0x9000)), dict(out=_t(capi.DTYPE_U8, (192, 24, 3, 0), data=0x9000)),
    dict(valid=_t(capi.DTYPE_U8, (0, 8, 1, 0))), dict(valid=_t(capi.DTYPE_U8, (64, 0, 1, 0))),
    dict(valid=_t(capi.DTYPE_U8, (64, 8, 0, 0))),
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(-1, 8, 3)), dict(size=(8, 8, 0)), dict(size=(8, 8, 5)),
])
def test_c_abi_rectify_refuses(kw):
    assert _rect(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


@pytest.mark.parametrize("kw", _RULE_REFUSALS + [
    dict(ofw=None), dict(obw=None), dict(ofw=_t(strides=_FS, data=0)), dict(obw=_t(strides=_FS, data=0)),
    dict(ofw=_t(capi.DTYPE_U8, _FS, data=0x9000)), dict(obw=_t(3, _FS, data=0x9000)),
    dict(ofw=_t(strides=(128, -8, 1, 64), data=0x9000)), dict(obw=_t(strides=(128, 8, 1, -64), data=0x9000)),
    dict(ofw=_t(strides=(0, 8, 1, 64), data=0x9000)), dict(ofw=_t(strides=(128, 0, 1, 64), data=0x9000)),
    dict(obw=_t(strides=(128, 8, 0, 64), data=0x9000)), dict(obw=_t(strides=(128, 8, 1, 0), data=0x9000)),
    dict(size=(0, 8)), dict(size=(8, 0)), dict(size=(-1, 8)),
])
def test_c_abi_rectified_flows_refuses(kw):
    assert _rflow(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle():
    lib = _lib()
    assert _rect(lib, None) == -1 and _rect(lib, None, valid=None) == -1 and _rect(lib, None, mat=_t(strides=(6, 3, 1, 0))) == -1
    assert _rflow(lib, None) == -1
