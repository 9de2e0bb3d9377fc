"""CPU-side checks of video deblurring (papteam_opticalflow_amd/tensors.py: deblur, deblur_video; include/papof.h:
papof_deblur_tensor, papof_deblur_workspace): known answers of the numpy fp64 restatement in tests/_deblur_ref.py that
tests/test_gpu_deblur.py compares the device's frames with, its quality on a shaking camera and on a steady pan against
bars fixed beforehand, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal
of the C ABI through ctypes.  No device is touched here."""
import ctypes
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _deblur_ref import BRANCHES, deblur_reference, slots  # noqa: E402
from _interp_ref import _taps, as_f64, convert  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import blur_schedule  # noqa: E402


def _rand(T, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    return (0.01 + 0.98 * rng.random((T, H, W, C))).astype(dtype)  # (>= EPS: see test_one_sample_at_the_frame...)


def _smooth_flows(T, H, W, seed, amp=1.5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fw = np.stack([np.stack([amp * np.sin(0.3 * x + rng.uniform(0, 6)), amp * np.cos(0.2 * y + rng.uniform(0, 6))])
                   for _ in range(T - 1)])
    return fw, -fw + rng.normal(0, 0.05, fw.shape)


# ---- known answers of the restatement
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_one_sample_at_the_frame_and_radius_zero_return_the_input(dtype):
    """est = L and ratio = b / b = 1.0 for values >= EPS (0.0 / EPS = 0.0 for a zero): the bytes of the input, whatever
    the flows and however many iterations"""
    T, H, W, C = 3, 9, 11, 3
    frames = _rand(T, H, W, C, dtype, 1)
    frames[0, 0, 0] = 0
    fw, bw = _smooth_flows(T, H, W, 2, amp=4.0)
    for iters in (1, 5):
        out, support = deblur_reference(frames, fw, bw, [0.0], [1.0], radius=0, iters=iters, out_dtype=dtype)
        assert out.dtype == dtype and out.tobytes() == frames.tobytes()
        assert (support == 1).all()


def test_zero_flows_and_radius_zero_return_uint8_bytes_for_any_table():
    T, H, W, C = 3, 8, 10, 3
    frames = _rand(T, H, W, C, np.uint8, 3)
    frames.reshape(-1)[:256] = np.arange(256)  # every byte value occurs
    z = np.zeros((T - 1, 2, H, W))
    for K, shape, shutter, phase in ((1, "box", 0.5, -0.5), (5, "triangle", 1.0, 0.0), (16, "box", 0.5, -0.5),
                                     (64, "triangle", 1.0, -1.0)):
        off, w = blur_schedule(shutter, K, phase, shape)
        out, support = deblur_reference(frames, z, z, off, w, radius=0, iters=6, out_dtype=np.uint8)
        assert out.dtype == np.uint8 and (out == frames).all() and (support == 1).all(), (K, shape)


def test_nan_flows_leave_the_video_unchanged_with_no_support():
    T, H, W, C = 4, 7, 9, 2
    nan = np.full((T - 1, 2, H, W), math.nan)
    off, w = blur_schedule(0.5, 8)
    for dtype in (np.uint8, np.float32, np.float64):
        frames = _rand(T, H, W, C, dtype, 4)
        for R in (0, 2):
            out, support = deblur_reference(frames, nan, nan, off, w, radius=R, iters=3, out_dtype=dtype)
            assert out.tobytes() == frames.tobytes() and not support.any()
    frames = _rand(T, H, W, C, np.float64, 5) - 0.5  # negative values and a NaN are data of value 0
    frames[1, 2, 3] = math.nan
    out, _ = deblur_reference(frames, nan, nan, off, w, radius=1, iters=2)
    assert out.tobytes() == np.fmax(frames, 0.0).tobytes()


def test_any_grouping_of_the_targets_gives_the_same_result():
    T, H, W, C = 5, 8, 12, 2
    frames = _rand(T, H, W, C, np.float32, 6)
    fw, bw = _smooth_flows(T, H, W, 7)
    off, w = blur_schedule(0.8, 6, -0.5, "triangle")
    whole = deblur_reference(frames, fw, bw, off, w, radius=2, iters=3)
    for groups in ([[0], [1], [2], [3], [4]], [[4, 2], [0], [3, 1]], [[0, 1, 2], [3, 4]]):
        out, support = np.zeros_like(whole[0]), np.zeros_like(whole[1])
        for g in groups:
            o, s = deblur_reference(frames, fw, bw, off, w, radius=2, iters=3, targets=g)
            out[g], support[g] = o[g], s[g]
        assert out.tobytes() == whole[0].tobytes() and support.tobytes() == whole[1].tobytes()


def test_slot_order_and_end_frames():
    assert slots(0, 2, 2) == [(0, 0), (1, 1)] and slots(1, 2, 2) == [(0, 1), (2, 0)]
    assert slots(0, 3, 2) == [(0, 0), (1, 1), (3, 2)]
    assert slots(1, 3, 2) == [(0, 1), (1, 2), (2, 0)]
    assert slots(2, 3, 2) == [(0, 2), (2, 1), (4, 0)]
    assert slots(4, 9, 4) == list(enumerate([4, 5, 3, 6, 2, 7, 1, 8, 0])) and slots(3, 7, 0) == [(0, 3)]
    # with zero flows and one sample the update of a pixel is the mean over the slots of b_s / b_t, summed in slot order
    for T in (2, 3):
        frames = _rand(T, 4, 5, 1, np.float64, 8 + T)
        z = np.zeros((T - 1, 2, 4, 5))
        out, support = deblur_reference(frames, z, z, [0.0], [1.0], radius=2, iters=1)
        for t in range(T):
            corr = np.zeros_like(frames[t])
            for _, s in slots(t, T, 2):
                corr = corr + frames[s] / frames[t]
            assert out[t].tobytes() == (frames[t] * (corr / float(T))).tobytes() and (support[t] == T).all()


def test_the_line_follows_the_velocity_of_each_frame():
    """three frames, radius 0: the interior frame's velocity is half the difference of its two flows, the end frames' their
    one flow -- checked on pass A's estimate through a single off-centre sample"""
    T, H, W = 3, 6, 16
    frames = _rand(T, H, W, 1, np.float64, 11)
    fw, bw = np.zeros((T - 1, 2, H, W)), np.zeros((T - 1, 2, H, W))
    fw[0, 0], fw[1, 0], bw[0, 0], bw[1, 0] = 2.0, 4.0, -1.0, -3.0
    out, _ = deblur_reference(frames, fw, bw, [0.5], [2.0], radius=0, iters=1, consistency=None)
    x = np.arange(W, dtype=np.float64)
    for t, v in ((0, 2.0), (1, 0.5 * (4.0 - -1.0)), (2, 0.0 - -3.0)):
        L = frames[t, ..., 0]
        xa, xb = np.clip(x + 0.5 * v, 0, W - 1), np.clip(x - 0.5 * v, 0, W - 1)
        est = np.stack([np.interp(xa, x, L[r]) for r in range(H)])
        ratio = L / np.maximum(est, 2.0 ** -10)
        want = L * np.stack([np.interp(xb, x, ratio[r]) for r in range(H)])
        assert np.allclose(out[t, ..., 0], want, rtol=1e-13, atol=0)


def test_the_census_counts_every_branch():
    T, H, W, C = 4, 9, 40, 1
    frames = _rand(T, H, W, C, np.float64, 12)
    frames[:, :, :6] = 0.0  # a dark band: estimates under the floor
    fw, bw = _smooth_flows(T, H, W, 13, amp=3.0)
    fw[:, :, 4, 20], bw[:, :, 5, 9] = math.nan, math.inf
    fw[:, :, 0, 0] = 500.0
    off, w = blur_schedule(1.0, 4)
    *_, seen = deblur_reference(frames, fw, bw, off, w, radius=1, iters=1, parts=True)
    assert sorted(seen) == sorted(BRANCHES) and all(seen.values()), seen


# ---- quality: a shaking camera and a steady pan on the committed 480 x 270 frame
H, W, T_SHAKE, MID, CROP = 96, 160, 7, 3, 16
X0, Y0 = 150, 70  # the window's origin in the committed frame (tests/test_blur_cpu.py's)
SUB = 64          # sub-frames of an exposure


def camera(t):
    return np.array([6 * math.sin(2 * math.pi * t / 5.3) + 3 * math.sin(2 * math.pi * t / 2.9 + 1),
                     5 * math.sin(2 * math.pi * t / 4.1 + 2) + t])


def _window(img, dx, dy):
    """the H x W window of img moved by (dx, dy) pixels: out(r, x) = img(Y0 + r - dy, X0 + x - dx), bilinear"""
    yy, xx = Y0 + np.arange(H)[:, None] - dy, X0 + np.arange(W)[None, :] - dx
    yi, xi = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = (yy - yi)[..., None], (xx - xi)[..., None]
    return ((1 - fy) * ((1 - fx) * img[yi, xi] + fx * img[yi, xi + 1])
            + fy * ((1 - fx) * img[yi + 1, xi] + fx * img[yi + 1, xi + 1]))


@functools.lru_cache(maxsize=None)
def scene(kind, shutter, noise=0.0):
    """(the recorded uint8 frames (T, H, W, 3) -- each the mean of SUB sub-frames over its shutter, plus Gaussian noise of
    `noise` / 255, quantised --, the sharp float64 frames, the exact translational flows) of the camera path `kind`: "shake"
    (camera) or "pan" ((6, 2) pixels per frame).  Cached and shared: treat as read-only."""
    import cases
    img = as_f64(cases.load_frame_u8("480", 1))
    path = camera if kind == "shake" else (lambda t: np.array([6.0 * t, 2.0 * t]))
    at = lambda time: _window(img, *path(time))  # noqa: E731
    sharp = np.stack([at(float(t)) for t in range(T_SHAKE)])
    blurred = np.stack([np.mean([at(t + shutter * ((j + 0.5) / SUB - 0.5)) for j in range(SUB)], 0) for t in range(T_SHAKE)])
    if noise:
        blurred = blurred + np.random.default_rng(21).normal(0, noise / 255.0, blurred.shape)
    fw = np.empty((T_SHAKE - 1, 2, H, W))
    for t in range(T_SHAKE - 1):
        fw[t] = (path(t + 1.0) - path(float(t)))[:, None, None]
    return convert(blurred, np.uint8), sharp, fw, -fw


def psnr(a, b, m=CROP):
    d = (as_f64(a) - as_f64(b))[m:-m, m:-m]
    return -10.0 * math.log10(float((d * d).mean()))


def deblurred_mid(frames, fw, bw, shutter, radius, iters, each=None):
    off, w = blur_schedule(shutter, 16)
    return deblur_reference(frames, fw, bw, off, w, radius=radius, iters=iters, targets=[MID], each=each)[0][MID]


@functools.lru_cache(maxsize=None)
def estimated_flows(shutter):
    """the oracle's flows at 4 levels on the blurred uint8 frames of the shake scene (cached and shared: read-only)"""
    from test_rolling_cpu import oracle_flows
    return oracle_flows(scene("shake", shutter)[0], 4)


# the least gains in dB, fixed before the restatement was run: about half of what a prototype of the rule gained
BAR_EXACT, BAR_WIDE_SHUTTER, BAR_ESTIMATED, BAR_PAN = 6.0, 4.0, 2.5, 1.5


def test_shake_with_exact_flows_gains_6_db():
    """The shake scene: 7 frames of 96 x 160 cut from the committed 480 x 270 frame under camera(), shutter 0.5, speeds of
    3.7, 7.1 and 2.3 pixels per frame around the middle frame, uint8; PSNR of the middle frame against the sharp one, 16
    pixels cropped.  Measured here: blurred 25.58 dB; radius 1, 6 iterations: 36.40 dB (+10.82, bar +6); radius 2: 40.02
    dB (must not be more than 1 dB below radius 1); radius 0, recorded: 26.80 dB -- one frame alone cannot fill the zeros
    of its own blur."""
    frames, sharp, fw, bw = scene("shake", 0.5)
    before = psnr(frames[MID], sharp[MID])
    got = {R: psnr(deblurred_mid(frames, fw, bw, 0.5, R, 6), sharp[MID]) for R in (0, 1, 2)}
    print("shake, exact flows, shutter 0.5: blurred %.2f dB; radius 0 / 1 / 2: %.2f / %.2f / %.2f dB" % (before, got[0], got[1], got[2]))
    assert got[1] - before >= BAR_EXACT
    assert got[2] >= got[1] - 1.0


def test_shake_with_a_full_shutter_gains_4_db():
    """shutter 1.0, exact flows, radius 1, 8 iterations.  Measured here: blurred 20.66 dB, deblurred 29.13 dB (+8.47, bar +4)"""
    frames, sharp, fw, bw = scene("shake", 1.0)
    before, got = psnr(frames[MID], sharp[MID]), psnr(deblurred_mid(frames, fw, bw, 1.0, 1, 8), sharp[MID])
    print("shake, exact flows, shutter 1.0, 8 iterations: blurred %.2f dB, deblurred %.2f dB" % (before, got))
    assert got - before >= BAR_WIDE_SHUTTER


def test_shake_with_estimated_flows_gains_2_5_db():
    """The oracle's flows at 4 levels on the blurred uint8 frames, shutter 0.5, radius 1, 6 iterations.  Measured here: the
    flows are 0.40 px off per component on average; blurred 25.58 dB, deblurred 30.71 dB (+5.13, bar +2.5).  Recorded: radius
    2 30.83 dB; shutter 1.0 (flows 0.82 px off), 8 iterations: 20.66 -> 23.00 dB."""
    frames, sharp, fw, _ = scene("shake", 0.5)
    ofw, obw = estimated_flows(0.5)
    before = psnr(frames[MID], sharp[MID])
    got = {R: psnr(deblurred_mid(frames, ofw, obw, 0.5, R, 6), sharp[MID]) for R in (1, 2)}
    print("shake, oracle's flows (%.2f px off), shutter 0.5: blurred %.2f dB; radius 1 / 2: %.2f / %.2f dB"
          % (np.abs(ofw - fw).mean(), before, got[1], got[2]))
    assert got[1] - before >= BAR_ESTIMATED
    wide, wsharp, wfw, _ = scene("shake", 1.0)
    ofw, obw = estimated_flows(1.0)
    print("shake, oracle's flows (%.2f px off), shutter 1.0, 8 iterations: blurred %.2f dB, deblurred %.2f dB"
          % (np.abs(ofw - wfw).mean(), psnr(wide[MID], wsharp[MID]), psnr(deblurred_mid(wide, ofw, obw, 1.0, 1, 8), wsharp[MID])))


def test_steady_pan_gains_1_5_db():
    """A pan of (6, 2) pixels per frame, where every frame carries the same blur and no neighbour helps: uint8 with noise
    of 2 / 255, shutter 0.5, radius 0, 8 iterations.  Measured here: blurred 24.57 dB, deblurred 27.21 dB (+2.64, bar
    +1.5); radius 1: 27.40 dB -- the neighbours average the noise, they add no frequency."""
    frames, sharp, fw, bw = scene("pan", 0.5, 2.0)
    before = psnr(frames[MID], sharp[MID])
    got = {R: psnr(deblurred_mid(frames, fw, bw, 0.5, R, 8), sharp[MID]) for R in (0, 1)}
    print("pan, shutter 0.5, 8 iterations: blurred %.2f dB; radius 0 / 1: %.2f / %.2f dB" % (before, got[0], got[1]))
    assert got[0] - before >= BAR_PAN


def test_recorded_curve_and_lucky_frame():
    """Recorded, not asserted (README).  Shake scene, shutter 0.5, exact flows, radius 1, PSNR in dB
    after 2 .. 12 iterations: 33.49 35.61 36.58 36.70 36.40 35.97 35.53 35.14 34.80 34.51 34.26 -- it peaks at 5 and falls
    behind it: there is no prior.  The lucky-frame baseline -- the neighbour of smallest speed (frame 4, 2.3 px per frame)
    carried to the middle frame with the exact flow, bilinearly --: 29.97 dB, so 4.4 dB of the 10.8 dB are selection and
    6.4 dB fusion."""
    frames, sharp, fw, bw = scene("shake", 0.5)
    curve = {}
    deblurred_mid(frames, fw, bw, 0.5, 1, 12, each=lambda t, it, L: curve.__setitem__(it + 1, psnr(L, sharp[MID])))
    print("shake, exact flows, radius 1, iterations 2 .. 12: " + " ".join("%d: %.2f" % (k, curve[k]) for k in range(2, 13)))
    d = fw[MID, :, 0, 0]  # frame 3 -> 4: the lucky frame 4 read at p + d
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    taps = _taps(np.clip(x + d[0], 0, W - 1).ravel(), np.clip(y + d[1], 0, H - 1).ravel(), H, W)
    lucky = sum(as_f64(frames[MID + 1])[r, c] * wt[:, None] for r, c, wt in taps).reshape(H, W, 3)
    print("lucky frame (frame 4 carried to frame 3): %.2f dB" % psnr(lucky, sharp[MID]))
    assert all(math.isfinite(v) for v in curve.values())


def test_recorded_two_passes():
    """Recorded, not asserted: passes=2 of deblur_video with the oracle's flows -- the flows estimated again on the first
    pass's uint8 video, the ORIGINAL frames deblurred with them --: 30.70 dB after the first pass, 30.85 dB after the second
    (over the four pairs around the middle frame the flows are 0.29 px off per component in the first pass and 0.28 px in the
    second: the deconvolved frames are sharper but ring, and the solver gains next to nothing from them).  Only the five
    frames whose flows the middle frame's update reads are computed."""
    from test_rolling_cpu import oracle_flows
    frames, sharp, fw, bw = scene("shake", 0.5)
    ofw, obw = estimated_flows(0.5)
    off, w = blur_schedule(0.5, 16)
    near = list(range(MID - 2, MID + 3))  # the middle frame's update reads the flows of these frames only
    first = deblur_reference(frames, ofw, obw, off, w, radius=1, iters=6, out_dtype=np.uint8, targets=near)[0][near]
    ofw2, obw2 = oracle_flows(first, 4)
    second = psnr(deblur_reference(frames[near], ofw2, obw2, off, w, radius=1, iters=6, targets=[2])[0][2], sharp[MID])
    print("passes=2 with the oracle's flows: first pass %.2f dB (flows %.2f px off), second %.2f dB (flows %.2f px off)"
          % (psnr(first[2], sharp[MID]), np.abs(ofw[near[:-1]] - fw[near[:-1]]).mean(), second, np.abs(ofw2 - fw[near[:-1]]).mean()))
    assert math.isfinite(second)


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_F = lambda: _z(2, 2, 8, 8)  # noqa: E731
_V = lambda: _z(3, 3, 8, 8)  # noqa: E731


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.deblur(_V(), _F(), _F()), ValueError),                                            # CPU tensors
    (lambda: tensors.deblur(None, _F(), _F()), TypeError),
    (lambda: tensors.deblur(_V(), _F(), _F(), layout="CHWN"), ValueError),
    (lambda: tensors.deblur(_z(3, 3, 8, 8, dtype=torch.int16), _F(), _F()), TypeError),
    (lambda: tensors.deblur(_z(3, 8), _F(), _F()), ValueError),
    (lambda: tensors.deblur_video(_V(), 2), ValueError),
    (lambda: tensors.deblur_video(_V(), 0), ValueError),                                               # pyramid levels
    (lambda: tensors.deblur_video(None, 2), TypeError),
    (lambda: tensors.deblur_video(_z(1, 3, 8, 8), 2), ValueError),                                     # fewer than 2 frames
    (lambda: tensors.deblur_video(_V(), 2, layout="HWC"), ValueError),
    (lambda: tensors.deblur_video(_V(), 2, consistency=(0.01,)), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("kw,exc", [
    (dict(shutter=0.0), ValueError), (dict(shutter=1.5), ValueError), (dict(shutter=math.nan), ValueError),  # the schedule
    (dict(samples=0), ValueError), (dict(samples=65), ValueError), (dict(samples=2.0), ValueError),
    (dict(phase=0.5), ValueError), (dict(phase=-1.5), ValueError), (dict(shape="gauss"), ValueError),
    (dict(shutter=2.0 ** -22, samples=2), ValueError),
    (dict(radius=-1), ValueError), (dict(radius=5), ValueError), (dict(radius=1.0), ValueError),       # radius, iters
    (dict(radius=True), ValueError), (dict(radius=None), ValueError),
    (dict(iters=0), ValueError), (dict(iters=257), ValueError), (dict(iters=2.0), ValueError), (dict(iters=None), ValueError),
    (dict(consistency=(0.01, -1.0)), ValueError), (dict(consistency=(math.nan, 0.5)), ValueError),     # consistency
    (dict(consistency="yes"), TypeError), (dict(consistency=(0.01,)), TypeError),
    (dict(frames=_z(1, 3, 8, 8)), ValueError),                                                         # one frame
    (dict(frames=_z(3, 5, 8, 8)), ValueError),                                                         # five channels
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError),                                     # flows
    (dict(flow_bw=_z(2, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(2, 3, 8, 8), flow_bw=_z(2, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(3, 2, 8, 8), flow_bw=_z(3, 2, 8, 8)), ValueError),                               # not (T - 1, 2, H, W)
    (dict(flow_fw=_z(2, 2, 8, 9), flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_bw=_z(2, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError),
    (dict(flow_fw=_z(2, 2, 8, 8, device="meta"), flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),  # devices
    (dict(flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),             # output dtype
    (dict(layout="NCWH"), ValueError),
])
def test_deblur_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        tensors.deblur(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(passes=0), ValueError), (dict(passes=9), ValueError), (dict(passes=1.0), ValueError), (dict(passes=True), ValueError),
    (dict(shutter=-1.0), ValueError), (dict(samples=100), ValueError), (dict(phase=1.0), ValueError),
    (dict(shape="tent"), ValueError), (dict(radius=5), ValueError), (dict(iters=0), ValueError),
    (dict(out_dtype=torch.int16), TypeError), (dict(consistency=(0.01, -1.0)), ValueError),
    (dict(consistency="yes"), TypeError), (dict(bogus=1), TypeError),
])
def test_deblur_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.deblur_video(_V(), 2, **kw)
    assert stub == []


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
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
_LO = 2.0 ** -20
_P = 8 * 3 * 8 * 8 * 4  # one target's bytes for 8 x 8 x 3 and radius 1


def _call(lib, h, n=3, size=(8, 8, 3), fr=_OK, fw=_OK, bw=_OK, off=(-0.25, 0.0, 0.25), w=(1.0, 1.0, 1.0), out=_OK, sup=None,
          ns=None, radius=1, iters=2, alphas=(0.01, 0.5), ws=0x2000, ws_bytes=3 * _P):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "fw": lambda: _t(strides=(128, 8, 1, 64)),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)), "out": lambda: _t(capi.DTYPE_U8)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, fw=fw, bw=bw, out=out).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    arr = lambda v: (ctypes.c_double * max(1, len(v)))(*v) if v is not None else None  # noqa: E731
    ns = ns if ns is not None else (len(off) if off is not None else 1)
    return lib.papof_deblur_tensor(h, n, size[0], size[1], size[2], ref(d["fr"]), ref(d["fw"]), ref(d["bw"]), ns, arr(off),
                                   arr(w), radius, iters, 1, alphas[0], alphas[1], ref(d["out"]), ref(sup),
                                   ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(fw=None), dict(bw=None), dict(out=None),                                        # NULL descriptors
    dict(fr=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(out=_t(data=0)),              # NULL data
    dict(sup=_t(capi.DTYPE_U8, data=0)), dict(off=None), dict(w=None),
    dict(fr=_t(dtype=3)), dict(fr=_t(dtype=-1)),                                                        # frame dtypes
    dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),                                                   # flow dtypes
    dict(sup=_t(capi.DTYPE_F32)), dict(sup=_t(capi.DTYPE_F64)), dict(sup=_t(dtype=5)),                 # support: U8 only
    dict(out=_t(dtype=3)),                                                                              # out dtype
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr=_t(strides=(192, 24, -3, 1))),                      # negative strides
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),
    dict(out=_t(strides=(192, 24, 3, -1))), dict(sup=_t(capi.DTYPE_U8, (-64, 8, 1, 0))),
    dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 0, 3, 1))),                          # zero out strides
    dict(out=_t(strides=(192, 24, 0, 1))), dict(out=_t(strides=(192, 24, 3, 0))),
    dict(sup=_t(capi.DTYPE_U8, (0, 8, 1, 0))), dict(sup=_t(capi.DTYPE_U8, (64, 0, 1, 0))),            # ... and support's
    dict(sup=_t(capi.DTYPE_U8, (64, 8, 0, 0))),
    dict(ns=0), dict(ns=-1), dict(ns=65, off=(0.25,) * 65, w=(1.0,) * 65),                             # n_samples
    dict(off=(1.0, 0.0, 0.25)), dict(off=(-1.0, 0.0, 0.25)), dict(off=(1.5, 0.0, 0.25)),              # offsets
    dict(off=(_LO / 2, 0.0, 0.25)), dict(off=(-_LO / 2, 0.0, 0.25)), dict(off=(5e-324, 0.0, 0.25)),
    dict(off=(1.0 - _LO / 2, 0.0, 0.25)), dict(off=(-(1.0 - _LO / 2), 0.0, 0.25)),
    dict(off=(math.nan, 0.0, 0.25)), dict(off=(math.inf, 0.0, 0.25)), dict(off=(0.25, 0.0, -math.inf)),
    dict(w=(-1.0, 1.0, 1.0)), dict(w=(1.0, math.nan, 1.0)), dict(w=(1.0, 1.0, math.inf)),              # weights
    dict(w=(0.0, 0.0, 0.0)), dict(w=(0.0, -0.0, 0.0)), dict(w=(1.0, 1.0, -5e-324)), dict(w=(1e308, 1e308, 1e308)),
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(size=(-1, 8, 3)), dict(size=(8, 8, 5)),  # sizes
    dict(size=(2 ** 15, 2 ** 15, 1), ws_bytes=2 ** 62), dict(size=(2 ** 30, 1, 1), ws_bytes=2 ** 62),  # H W >= 2^30
    dict(n=1), dict(n=0), dict(n=-2),                                                                   # T >= 2
    dict(radius=-1), dict(radius=5), dict(iters=0), dict(iters=-3), dict(iters=257),                   # radius, iters
    dict(alphas=(-0.01, 0.5)), dict(alphas=(0.01, math.nan)), dict(alphas=(math.inf, 0.5)),            # alphas
    dict(ws=0), dict(ws_bytes=_P - 1), dict(ws_bytes=0), dict(ws_bytes=-1),                             # workspace
    dict(radius=2, ws_bytes=_P),                                                                        # (P grows with R)
])
def test_c_abi_deblur_refuses(kw):
    assert _call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_deblur_without_a_handle():
    lib = _lib()
    assert _call(lib, None) == -1
    assert _call(lib, None, off=(_LO, -(1.0 - _LO), 0.0), w=(0.0, 2.0, 0.0), radius=0, iters=256, ws_bytes=_P) == -1


def test_c_abi_workspace_sizes():
    lib = _lib()
    ws = lib.papof_deblur_workspace
    assert ws(3, 8, 8, 3, 1) == 3 * _P and ws(3, 8, 8, 3, 0) == 3 * _P // 2 and ws(2, 1, 1, 1, 4) == 2 * 80
    P = 8 * 3 * 1080 * 1920 * 4  # a target of 1080p RGB with radius 1: 199 MB, ten of them fit 2 GiB
    assert ws(8, 1080, 1920, 3, 1) == 8 * P and ws(100, 1080, 1920, 3, 1) == 10 * P
    assert ws(5, 8192, 8192, 4, 4) == 8 * 4 * 8192 * 8192 * 10  # one target is more than 2 GiB: one target
    for bad in ((1, 8, 8, 3, 1), (0, 8, 8, 3, 1), (3, 0, 8, 3, 1), (3, 8, 0, 3, 1), (3, 8, 8, 0, 1), (3, 8, 8, 5, 1),
                (3, 8, 8, 3, -1), (3, 8, 8, 3, 5), (3, 2 ** 15, 2 ** 15, 1, 1), (3, 2 ** 30, 1, 1, 0)):
        assert ws(*bad) == -1, bad
    assert ws(3, 2 ** 15, 2 ** 15 - 1, 1, 0) > 0


def test_symbols_are_declared_and_listed():
    assert "papof_deblur_tensor" in capi.SYMBOLS and "papof_deblur_workspace" in capi.SYMBOLS
    lib = _lib()
    assert lib.papof_deblur_tensor.restype is ctypes.c_int and lib.papof_deblur_workspace.restype is ctypes.c_longlong
