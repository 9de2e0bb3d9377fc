"""CPU-side checks of synthetic motion blur (papteam_opticalflow_amd/tensors.py: blur_schedule, motion_blur, blur_video;
include/papof.h: papof_motion_blur_tensor): known answers of the shutter schedule and of the numpy fp64 restatement in
tests/_blur_ref.py that tests/test_gpu_blur.py compares the device's frames with, the quality of the rule on a panning
texture against the exact shutter integral, every Python argument error raised before a launch (CPU tensors, a stubbed
handle), and each refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _blur_ref import blur_reference  # noqa: E402
from _interp_ref import as_f64, convert, interp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import blur_schedule  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the schedule
def test_schedule_known_answers():
    off, w = blur_schedule(shutter=0.5, samples=4)
    assert off == [-0.1875, -0.0625, 0.0625, 0.1875] and w == [1.0] * 4
    for K in (1, 3, 5, 15, 63):
        off, w = blur_schedule(samples=K)
        assert off[K // 2] == 0.0 and len(off) == len(w) == K
        assert all(a < b for a, b in zip(off, off[1:]))
    off, _ = blur_schedule(1.0, 8, 0.0)  # opens at the frame
    assert off == [(k + 0.5) / 8 for k in range(8)]
    off, _ = blur_schedule(1.0, 8, -1.0)  # closes at the frame
    assert off == [(k + 0.5) / 8 - 1.0 for k in range(8)]
    off, _ = blur_schedule(0.3, 7, -0.25)  # the stated order of operations
    assert off == [0.3 * ((k + 0.5) / 7 + -0.25) for k in range(7)]
    assert blur_schedule() == blur_schedule(0.5, 16, -0.5, "box")


def test_triangle_weights():
    _, w = blur_schedule(samples=4, shape="triangle")
    assert w == [0.25, 0.75, 0.75, 0.25]
    _, w = blur_schedule(samples=5, shape="triangle")
    assert w == [1.0 - abs(2.0 * (k + 0.5) / 5 - 1.0) for k in range(5)] and w[2] == 1.0
    off_b, _ = blur_schedule(0.7, 9, -0.3, "box")
    off_t, w = blur_schedule(0.7, 9, -0.3, "triangle")
    assert off_b == off_t and all(x > 0 for x in w)
    assert blur_schedule(samples=1, shape="triangle")[1] == [1.0]


@pytest.mark.parametrize("kw", [
    dict(shutter=0.0), dict(shutter=-0.5), dict(shutter=1.0001), dict(shutter=math.nan), dict(shutter=math.inf),
    dict(shutter="0.5"), dict(shutter=None), dict(shutter=True),
    dict(samples=0), dict(samples=65), dict(samples=-1), dict(samples=4.0), dict(samples=True), dict(samples=None),
    dict(phase=0.01), dict(phase=-1.01), dict(phase=math.nan), dict(phase="centre"), dict(phase=None),
    dict(shape="gauss"), dict(shape=None), dict(shape=1),
    dict(shutter=2.0 ** -22, samples=2),               # offsets of magnitude 2^-24: below 2^-20 and not 0
    dict(shutter=1.0, samples=1, phase=-2.0 ** -30 - 0.5),  # an offset of -2^-30
])
def test_schedule_refuses(kw):
    with pytest.raises(ValueError):
        blur_schedule(**kw)


# ---- known answers of the restatement
def _rand(T, H, W, C, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (T, H, W, C)).astype(np.uint8)
    return rng.random((T, H, W, C)).astype(dtype)


def _smooth_flows(T, H, W, seed, amp=1.5):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fw = np.stack([np.stack([amp * np.sin(0.3 * x + rng.uniform(0, 6)), amp * np.cos(0.2 * y + rng.uniform(0, 6))])
                   for _ in range(T - 1)])
    return fw, -fw + rng.normal(0, 0.05, fw.shape)


def test_identical_uint8_frames_with_zero_flows_return_the_input_bytes():
    f = _rand(1, 11, 13, 3, np.uint8, 1)
    frames = np.repeat(f, 4, 0)
    z = np.zeros((3, 2, 11, 13))
    for K, shape in ((1, "box"), (5, "triangle"), (16, "box"), (64, "triangle")):
        for shutter, phase in ((0.5, -0.5), (1.0, 0.0), (1.0, -1.0)):
            off, w = blur_schedule(shutter, K, phase, shape)
            out = blur_reference(frames, z, z, off, w, out_dtype=np.uint8)
            assert out.dtype == np.uint8 and (out == frames).all(), (K, shape, shutter, phase)


def test_two_frames_use_one_side_each():
    T, H, W, C = 2, 9, 12, 2
    frames = _rand(T, H, W, C, np.float64, 2)
    fw, bw = _smooth_flows(T, H, W, 3)
    off, w = blur_schedule(0.8, 6, -0.5, "triangle")
    out = blur_reference(frames, fw, bw, off, w)
    acc0, acc1, w0, w1 = np.zeros((H, W, C)), np.zeros((H, W, C)), 0.0, 0.0
    for tau, wk in zip(off, w):
        if tau > 0:  # frame 0: the pair (0, 1) at tau
            acc0 = acc0 + wk * interp_reference(frames[:1], frames[1:], fw, bw, [tau])[0, 0]
            w0 = w0 + wk
        else:        # frame 1: the same pair at 1 + tau
            acc1 = acc1 + wk * interp_reference(frames[:1], frames[1:], fw, bw, [1.0 + tau])[0, 0]
            w1 = w1 + wk
    assert (_bits(out[0]) == _bits(acc0 / w0)).all() and (_bits(out[1]) == _bits(acc1 / w1)).all()


def test_a_middle_frame_sums_both_sides_and_the_frame_in_table_order():
    T, H, W, C = 3, 8, 10, 1
    frames = _rand(T, H, W, C, np.float32, 4)
    fw, bw = _smooth_flows(T, H, W, 5)
    occ = (np.random.default_rng(6).random((T - 1, 2, H, W)) < 0.3).astype(np.uint8)
    off, w = [0.25, -0.5, 0.0, 0.75], [0.5, 2.0, 1.0, 0.25]  # not sorted: the sums follow the table
    out = blur_reference(frames, fw, bw, off, w, occ)
    I = as_f64(frames)
    s = [interp_reference(frames[1:2], frames[2:3], fw[1:], bw[1:], [0.25], occ[1:])[0, 0],
         interp_reference(frames[0:1], frames[1:2], fw[:1], bw[:1], [0.5], occ[:1])[0, 0], I[1],
         interp_reference(frames[1:2], frames[2:3], fw[1:], bw[1:], [0.75], occ[1:])[0, 0]]
    acc, ws = np.zeros((H, W, C)), 0.0
    for S, wk in zip(s, w):
        acc = acc + wk * S
        ws = ws + wk
    assert (_bits(out[1]) == _bits(acc / ws)).all()


def test_phase_zero_returns_the_last_frame_and_phase_minus_one_the_first():
    T, H, W, C = 3, 7, 9, 3
    fw, bw = _smooth_flows(T, H, W, 7)
    for dtype in (np.uint8, np.float32, np.float64):
        frames = _rand(T, H, W, C, dtype, 8)
        off, w = blur_schedule(1.0, 8, 0.0)
        out = blur_reference(frames, fw, bw, off, w, out_dtype=dtype)
        assert out.dtype == dtype and (out[-1] == frames[-1]).all() and not (out[0] == frames[0]).all()
        off, w = blur_schedule(1.0, 8, -1.0)
        out = blur_reference(frames, fw, bw, off, w, out_dtype=dtype)
        assert (out[0] == frames[0]).all() and not (out[-1] == frames[-1]).all()


def test_a_weight_of_zero_skips_a_nan_sample():
    T, H, W, C = 2, 6, 8, 1
    frames = _rand(T, H, W, C, np.float64, 9)
    frames[1] = math.nan
    z = np.zeros((1, 2, H, W))
    out = blur_reference(frames, z, z, [0.0, 0.25], [1.0, 0.0])
    assert (_bits(out[0]) == _bits(frames[0] / 1.0)).all()
    assert np.isnan(blur_reference(frames, z, z, [0.0, 0.25], [1.0, 1e-300])[0]).all()  # and any weight > 0 does not


def test_output_conversion_is_the_interpolation_rule():
    T, H, W, C = 3, 6, 8, 2
    frames = _rand(T, H, W, C, np.float64, 10) * 1.4 - 0.2  # values outside [0, 1]
    fw, bw = _smooth_flows(T, H, W, 11)
    off, w = blur_schedule(0.5, 5)
    out = blur_reference(frames, fw, bw, off, w)
    for dt in (np.uint8, np.float32):
        assert (blur_reference(frames, fw, bw, off, w, out_dtype=dt) == convert(out, dt)).all()


# ---- quality: a panning scene with exact flows against the shutter integral
def _texture(seed=12, n=40):
    """a smooth random texture as a function of real coordinates: n cosines of periods >= 12 pixels"""
    rng = np.random.default_rng(seed)
    kx, ky = rng.uniform(-1, 1, n) * 2 * math.pi / 12, rng.uniform(-1, 1, n) * 2 * math.pi / 12
    ph, a = rng.uniform(0, 2 * math.pi, n), rng.uniform(0.2, 1.0, n)

    def tex(x, y):
        v = sum(a[j] * np.cos(kx[j] * x + ky[j] * y + ph[j]) for j in range(n))
        return 0.5 + 0.45 * v / a.sum()
    return tex


def _psnr(a, b, m=10):
    return -10.0 * math.log10(float(((a - b)[m:-m, m:-m] ** 2).mean()))


PAN = (6, 2)   # pixels per frame
H, W = 120, 160
Y0, X0 = 70, 150  # the window of frame 0 in the committed 480 x 270 frame


def _window(img, dx, dy):
    """the H x W window of img moved by (dx, dy) pixels, out(r, x) = img(Y0 + r - dy, X0 + x - dx), between pixel centres
    the bilinear interpolant: exact for an integer (dx, dy)"""
    yy, xx = Y0 + np.arange(H)[:, None] - dy, X0 + np.arange(W)[None, :] - dx
    yi, xi = np.floor(yy).astype(int), np.floor(xx).astype(int)
    fy, fx = (yy - yi)[..., None], (xx - xi)[..., None]
    return ((1 - fy) * ((1 - fx) * img[yi, xi] + fx * img[yi, xi + 1])
            + fy * ((1 - fx) * img[yi + 1, xi] + fx * img[yi + 1, xi + 1]))


def _panning(T=3):
    """frames of the committed frame panning by PAN pixels per frame, their exact flows, and scene(time) -> the frame at
    any time"""
    import cases
    img = as_f64(cases.load_frame_u8("480", 1))
    scene = lambda time: _window(img, PAN[0] * time, PAN[1] * time)  # noqa: E731
    frames = np.stack([scene(float(f)) for f in range(T)])
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = PAN
    return frames, fw, -fw, scene


@pytest.mark.parametrize("shutter", [0.5, 1.0])
def test_panning_frame_is_at_least_20_db_closer_to_the_shutter_integral(shutter):
    """A window of the committed 480 x 270 frame panning by (6, 2) pixels per frame (an integer pan: every frame is exact
    pixels of it) with exact flows.  The truth for the middle frame of three is the mean of 64 sub-frames over the shutter,
    each the window moved by its fraction of the pan, the scene between pixel centres being the bilinear interpolant -- so
    the figure isolates what the rule adds (where the samples land, and K samples for an integral), not the resampling
    error that any shift of sampled frames has.  10 border pixels are cropped.  With K >= 4 the result must be at least
    20 dB closer to the truth than the sharp frame is.  Measured here (sharp frame; then K = 4, 8, 16): shutter 0.5: 25.9 dB;
    55.4, 67.3, 79.9 dB; shutter 1.0: 22.0 dB; 46.6, 59.3, 71.5 dB -- margins of 24.6 .. 54.1 dB."""
    frames, fw, bw, scene = _panning()
    truth = np.mean([scene(1.0 + shutter * ((j + 0.5) / 64 - 0.5)) for j in range(64)], 0)
    sharp = _psnr(frames[1], truth)
    for K in (4, 8, 16):
        off, w = blur_schedule(shutter, K)
        p = _psnr(blur_reference(frames, fw, bw, off, w)[1], truth)
        print("shutter %.1f K %2d: sharp %.1f dB, blurred %.1f dB, margin %.1f dB" % (shutter, K, sharp, p, p - sharp))
        assert p - sharp >= 20.0, (shutter, K, sharp, p)


def test_band_limited_texture_is_recorded():
    """The same pan of an analytic texture (cosines of periods >= 12 pixels, exact at any shift), so that the bilinear
    resampling of the sampled frames counts as error too.  Recorded, not asserted: that error does
    not shrink with K and bounds the gain.  Measured here (sharp frame; K = 4, 16): shutter 0.5 (a path of 3.2 pixels):
    50.6 dB; 60.8, 60.1 dB; shutter 1.0 (6.3 pixels): 39.2 dB; 62.5, 61.2 dB."""
    tex = _texture()
    y, x = np.mgrid[0:72, 0:96].astype(np.float64)
    scene = lambda time: tex(x - PAN[0] * time, y - PAN[1] * time)  # noqa: E731
    frames = np.stack([scene(float(f)) for f in range(3)])[..., None]
    fw = np.zeros((2, 2, 72, 96))
    fw[:, 0], fw[:, 1] = PAN
    for shutter in (0.5, 1.0):
        truth = np.mean([scene(1.0 + shutter * ((j + 0.5) / 64 - 0.5)) for j in range(64)], 0)
        sharp = _psnr(frames[1, ..., 0], truth)
        for K in (4, 16):
            off, w = blur_schedule(shutter, K)
            p = _psnr(blur_reference(frames, fw, -fw, off, w)[1, ..., 0], truth)
            print("texture, shutter %.1f K %2d: sharp %.1f dB, blurred %.1f dB" % (shutter, K, sharp, p))
            assert math.isfinite(p)


def test_moving_rectangle_is_recorded():
    """A 24 x 16 rectangle moving by PAN over a static textured background, exact flows per pixel of each frame (the
    rectangle's pixels move, the others rest) and the exact occlusion mask; shutter 0.5, K = 16, the middle frame against
    the mean of 64 exactly composed sub-frames.  Recorded, not asserted: the gather rule reads the
    flow at the output pixel, so the band the rectangle's edge sweeps outside its own outline stays sharp.  Measured here:
    the sharp frame 44.26 dB, blurred 48.70 dB, blurred with the mask 48.96 dB."""
    T, H, W = 3, 72, 96  # noqa: F841
    back_tex, fore_tex = _texture(13), _texture(14)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    back = back_tex(x, y)

    def scene(time):
        xs, ys = x - PAN[0] * time, y - PAN[1] * time  # the rectangle's own coordinates
        inside = (xs >= 30) & (xs < 54) & (ys >= 24) & (ys < 40)
        return np.where(inside, 1.0 - fore_tex(xs, ys), back), inside
    frames = np.stack([scene(float(f))[0] for f in range(T)])[..., None]
    inside = [scene(float(f))[1] for f in range(T)]
    fw, bw = np.zeros((T - 1, 2, H, W)), np.zeros((T - 1, 2, H, W))
    occ = np.zeros((T - 1, 2, H, W), np.uint8)
    for i in range(T - 1):
        for c in range(2):
            fw[i, c][inside[i]] = PAN[c]
            bw[i, c][inside[i + 1]] = -PAN[c]
        occ[i, 0] = ~inside[i] & inside[i + 1]   # background of frame i covered in i + 1
        occ[i, 1] = ~inside[i + 1] & inside[i]   # background of frame i + 1 covered in i
    truth = np.mean([scene(1.0 + 0.5 * ((j + 0.5) / 64 - 0.5))[0] for j in range(64)], 0)
    off, w = blur_schedule(0.5, 16)
    sharp = _psnr(frames[1, ..., 0], truth)
    plain = _psnr(blur_reference(frames, fw, bw, off, w)[1, ..., 0], truth)
    masked = _psnr(blur_reference(frames, fw, bw, off, w, occ)[1, ..., 0], truth)
    print("moving rectangle: sharp %.2f dB, blurred %.2f dB, with the mask %.2f dB" % (sharp, plain, masked))
    assert all(math.isfinite(v) for v in (sharp, plain, masked))


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
    (lambda: tensors.motion_blur(_V(), _F(), _F()), ValueError),                                       # CPU tensors
    (lambda: tensors.motion_blur(None, _F(), _F()), TypeError),
    (lambda: tensors.motion_blur(_V(), _F(), _F(), layout="CHWN"), ValueError),
    (lambda: tensors.motion_blur(_z(3, 3, 8, 8, dtype=torch.int16), _F(), _F()), TypeError),
    (lambda: tensors.motion_blur(_z(3, 8), _F(), _F()), ValueError),
    (lambda: tensors.blur_video(_V(), 2), ValueError),
    (lambda: tensors.blur_video(_V(), 0), ValueError),                                                 # pyramid levels
    (lambda: tensors.blur_video(None, 2), TypeError),
    (lambda: tensors.blur_video(_z(1, 3, 8, 8), 2), ValueError),                                       # fewer than 2 frames
    (lambda: tensors.blur_video(_V(), 2, layout="HWC"), ValueError),
    (lambda: tensors.blur_video(_V(), 2, consistency=(0.01,)), TypeError),
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
    (dict(frames=_z(1, 3, 8, 8)), ValueError),                                                         # one frame
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError),                                     # flows
    (dict(flow_bw=_z(2, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(2, 3, 8, 8), flow_bw=_z(2, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(3, 2, 8, 8), flow_bw=_z(3, 2, 8, 8)), ValueError),                               # not (T - 1, 2, H, W)
    (dict(flow_fw=_z(2, 2, 8, 9), flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_bw=_z(2, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError),
    (dict(flow_fw=_z(2, 2, 8, 8, device="meta"), flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),  # devices
    (dict(flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(occlusion=_z(2, 2, 8, 8)), TypeError), (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.int32)), TypeError),  # mask
    (dict(occlusion=_z(2, 1, 8, 8, dtype=torch.bool)), ValueError), (dict(occlusion=[0]), TypeError),
    (dict(occlusion=_z(3, 2, 8, 8, dtype=torch.bool)), ValueError),
    (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.bool, device="meta")), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),             # output dtype
])
def test_motion_blur_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        tensors.motion_blur(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(shutter=-1.0), ValueError), (dict(samples=100), ValueError), (dict(phase=1.0), ValueError),
    (dict(shape="tent"), ValueError), (dict(out_dtype=torch.int16), TypeError),
    (dict(consistency=(0.01, -1.0)), ValueError), (dict(consistency="yes"), TypeError), (dict(bogus=1), TypeError),
])
def test_blur_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.blur_video(_V(), 2, **kw)
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


def _call(lib, h, n=3, size=(8, 8, 3), fr=_OK, fw=_OK, bw=_OK, occ=None, off=(-0.25, 0.0, 0.25), w=(1.0, 1.0, 1.0), out=_OK,
          ns=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "fw": lambda: _t(strides=(128, 8, 1, 64)),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)), "out": lambda: _t(capi.DTYPE_U8)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, fw=fw, bw=bw, out=out).items()}
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    arr = lambda v: (ctypes.c_double * max(1, len(v)))(*v) if v is not None else None  # noqa: E731
    ns = ns if ns is not None else (len(off) if off is not None else 1)
    return lib.papof_motion_blur_tensor(h, n, ref(d["fr"]), size[0], size[1], size[2], ref(d["fw"]), ref(d["bw"]), ref(occ), ns,
                                        arr(off), arr(w), ref(d["out"]), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(fw=None), dict(bw=None), dict(out=None),                                        # NULL descriptors
    dict(fr=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(out=_t(data=0)),              # NULL data
    dict(occ=_t(capi.DTYPE_U8, data=0)), dict(off=None), dict(w=None),
    dict(fr=_t(dtype=3)), dict(fr=_t(dtype=-1)),                                                        # frame dtypes
    dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),                                                   # flow dtypes
    dict(occ=_t(capi.DTYPE_F32)), dict(occ=_t(capi.DTYPE_F64)), dict(occ=_t(dtype=5)),                 # mask: U8 only
    dict(out=_t(dtype=3)),                                                                              # out dtype
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr=_t(strides=(192, 24, -3, 1))),                      # negative strides
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),
    dict(occ=_t(capi.DTYPE_U8, (-128, 8, 1, 64))), dict(out=_t(strides=(192, 24, 3, -1))),
    dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 0, 3, 1))),                          # zero out strides
    dict(out=_t(strides=(192, 24, 0, 1))), dict(out=_t(strides=(192, 24, 3, 0))),
    dict(ns=0), dict(ns=-1), dict(ns=65, off=(0.25,) * 65, w=(1.0,) * 65),                             # n_samples
    dict(off=(1.0, 0.0, 0.25)), dict(off=(-1.0, 0.0, 0.25)), dict(off=(1.5, 0.0, 0.25)),              # offsets
    dict(off=(_LO / 2, 0.0, 0.25)), dict(off=(-_LO / 2, 0.0, 0.25)), dict(off=(5e-324, 0.0, 0.25)),
    dict(off=(1.0 - _LO / 2, 0.0, 0.25)), dict(off=(-(1.0 - _LO / 2), 0.0, 0.25)),
    dict(off=(math.nan, 0.0, 0.25)), dict(off=(math.inf, 0.0, 0.25)), dict(off=(0.25, 0.0, -math.inf)),
    dict(w=(-1.0, 1.0, 1.0)), dict(w=(1.0, math.nan, 1.0)), dict(w=(1.0, 1.0, math.inf)),              # weights
    dict(w=(0.0, 0.0, 0.0)), dict(w=(0.0, -0.0, 0.0)), dict(w=(1.0, 1.0, -5e-324)),
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(size=(-1, 8, 3)),           # sizes
    dict(n=1), dict(n=0), dict(n=-2),                                                                   # T >= 2
])
def test_c_abi_motion_blur_refuses(kw):
    assert _call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_motion_blur_without_a_handle():
    lib = _lib()
    assert _call(lib, None) == -1
    assert _call(lib, None, off=(_LO, -(1.0 - _LO), 0.0), w=(0.0, 2.0, 0.0)) == -1  # (arguments that a handle would accept)


def test_symbol_is_declared_and_listed():
    assert "papof_motion_blur_tensor" in capi.SYMBOLS
    assert _lib().papof_motion_blur_tensor.restype is ctypes.c_int
