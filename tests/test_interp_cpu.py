"""CPU-side checks of frame interpolation (papteam_opticalflow_amd/tensors.py: interpolate, interpolate_pairs,
interpolate_video; include/papof.h: papof_interp_tensor): known answers of the numpy fp64 restatement in tests/_interp_ref.py
that tests/test_gpu_interp.py compares the device's frames with, the interpolation error on the committed frames with the
oracle's flows, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the
C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _interp_ref import as_f64, convert, interp_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


def _const_flows(B, H, W, u, v):
    fw = np.zeros((B, 2, H, W))
    fw[:, 0], fw[:, 1] = u, v
    return fw, -fw


def _shifted(img, dx, dy):
    """img (H, W, C) moved by (dx, dy) pixels: out(r, x) = img(r - dy, x - dx), wrapped"""
    return np.roll(img, (dy, dx), axis=(0, 1))


# ---- known answers of the restatement
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("d", [(1, 0), (0, -2), (3, 1), (-2, -1)])
def test_integer_translation_by_2d_gives_the_shift_by_d_at_half_time(dtype, d):
    rng = np.random.default_rng(1)
    H, W, C = 17, 23, 3
    I0 = rng.integers(0, 256, (H, W, C)).astype(dtype) if dtype == np.uint8 else rng.random((H, W, C)).astype(dtype)
    dx, dy = d
    I1 = _shifted(I0, 2 * dx, 2 * dy)  # I1(p + 2d) = I0(p)
    fw, bw = _const_flows(1, H, W, 2 * dx, 2 * dy)
    out = interp_reference(I0[None], I1[None], fw, bw, [0.5])[0, 0]
    want = as_f64(_shifted(I0, dx, dy))
    # interior: both samples p - d and p + d inside the image and away from the wrap of I1
    m = 2 * max(abs(dx), abs(dy))
    inner = (slice(m, H - m), slice(m, W - m))
    assert (out[inner].view(np.int64) == want[inner].view(np.int64)).all()
    # in the frame's own dtype as well: uint8 comes back as the same bytes
    o8 = interp_reference(I0[None], I1[None], fw, bw, [0.5], out_dtype=dtype)[0, 0]
    assert (o8[inner] == _shifted(I0, dx, dy)[inner]).all()


def test_zero_flow_is_the_plain_blend_and_times_are_weights():
    rng = np.random.default_rng(2)
    H, W, C = 6, 9, 2
    I0, I1 = rng.random((1, H, W, C)), rng.random((1, H, W, C))
    fw = np.zeros((1, 2, H, W))
    ts = [0.25, 0.5, 0.75]
    out = interp_reference(I0, I1, fw, fw, ts)
    for j, t in enumerate(ts):
        s = 1.0 - t
        want = (s * I0[0] + t * I1[0]) / (s + t)  # both samples at p, no mask: w0 = s, w1 = t
        assert (out[0, j].view(np.int64) == want.view(np.int64)).all()


def _row_sample(img, r, X):
    """img (H, W) sampled at (X, r), r an integer row: the four taps in (m, n) order, the n = 1 ones of weight 0"""
    xx = int(X)
    fx = X - xx
    return (((0.0 + img[r, xx] * (abs(1.0 - fx) * 1.0)) + img[r + 1, xx] * (abs(1.0 - fx) * 0.0))
            + img[r, xx + 1] * (abs(0.0 - fx) * 1.0)) + img[r + 1, xx + 1] * (abs(0.0 - fx) * 0.0)


def test_flows_that_leave_the_image_or_are_nan_take_each_fallback():
    rng = np.random.default_rng(3)
    H, W = 8, 10
    I0, I1 = rng.random((1, H, W, 1)), rng.random((1, H, W, 1))
    blend = lambda r, x, s, t: (s * I0[0, r, x, 0] + t * I1[0, r, x, 0]).view(np.int64)  # noqa: E731
    fw, bw = np.zeros((1, 2, H, W)), np.zeros((1, 2, H, W))
    # neither sample: v = 4 H at t = 0.5 moves q0 up by H and q1 down by H -- the blend of the two pixels at p
    fw[0, 1, 0, 0] = 4.0 * H
    # NaN in either flow: neither sample
    fw[0, 0, 3, 4] = math.nan
    bw[0, 1, 5, 6] = math.nan
    # only q1 (t = 0.25, u = W - 1 at x = 0): a0 = -0.1875 (W - 1) leaves, a1 = 0.5625 (W - 1) stays
    fw[0, 0, 2, 0] = W - 1.0
    # only q0 (the same flow at x = W - 1): q0 = (W - 1) - 0.1875 (W - 1) stays, q1 leaves
    fw[0, 0, 2, W - 1] = W - 1.0
    out = interp_reference(I0, I1, fw, bw, [0.5, 0.25])[0]
    for (r, x) in ((0, 0), (3, 4), (5, 6)):
        assert out[0, r, x, 0].view(np.int64) == blend(r, x, 0.5, 0.5)
        assert out[1, r, x, 0].view(np.int64) == blend(r, x, 0.75, 0.25)
    g1 = _row_sample(I1[0, :, :, 0], 2, 0.0 + (0.5625 * (W - 1.0) - 0.1875 * 0.0))
    assert out[1, 2, 0, 0].view(np.int64) == ((0.25 * g1) / (0.0 + 0.25)).view(np.int64)
    g0 = _row_sample(I0[0, :, :, 0], 2, (W - 1.0) + (0.0625 * 0.0 - 0.1875 * (W - 1.0)))
    assert out[1, 2, W - 1, 0].view(np.int64) == ((0.75 * g0) / (0.75 + 0.0)).view(np.int64)


def test_an_all_ones_mask_on_one_side_hands_the_pixel_to_the_other_frame():
    rng = np.random.default_rng(4)
    H, W, C = 9, 12, 3
    I0, I1 = rng.random((1, H, W, C)), rng.random((1, H, W, C))
    fw, bw = _const_flows(1, H, W, 0.0, 0.0)
    occ = np.zeros((1, 2, H, W), np.uint8)
    occ[:, 0] = 1  # every pixel of I0 occluded in I1: g1 is unreliable, w1 = 0, the pixel is I0's
    for t in (0.2, 0.5, 0.9):
        out = interp_reference(I0, I1, fw, bw, [t], occ)[0, 0]
        s = 1.0 - t
        assert (out.view(np.int64) == ((s * I0[0]) / s).view(np.int64)).all()
    occ[:] = 0
    occ[:, 1] = 1  # the reverse: the pixel is I1's
    out = interp_reference(I0, I1, fw, bw, [0.3], occ)[0, 0]
    assert (out.view(np.int64) == ((0.3 * I1[0]) / 0.3).view(np.int64)).all()
    occ[:] = 1  # both sides occluded: w0 = w1 = 0 -- the unweighted blend of both samples
    out = interp_reference(I0, I1, fw, bw, [0.3], occ)[0, 0]
    s = 1.0 - 0.3
    assert (out.view(np.int64) == ((s * I0[0] + 0.3 * I1[0]) / (s + 0.3)).view(np.int64)).all()
    # a nonzero byte other than 1 reads as 1
    occ[:] = 0
    occ[:, 0] = 7
    assert (interp_reference(I0, I1, fw, bw, [0.5], occ)[0, 0].view(np.int64) == ((0.5 * I0[0]) / 0.5).view(np.int64)).all()


def test_the_mask_is_sampled_bilinearly_where_the_sample_lands():
    H, W = 4, 6
    I0, I1 = np.zeros((1, H, W, 1)), np.ones((1, H, W, 1))
    fw, bw = np.zeros((1, 2, H, W)), np.zeros((1, 2, H, W))
    fw[0, 0, 1, 2] = 1.0  # t = 0.5: a0 = -0.25, a1 = 0.25: q0 = (1.75, 1), q1 = (2.25, 1)
    occ = np.zeros((1, 2, H, W), np.uint8)
    occ[0, 0, 1, 2] = 1  # O0 at q0 = 0.75
    out = interp_reference(I0, I1, fw, bw, [0.5], occ)[0, 0, 1, 2, 0]
    w0, w1 = 0.5 * (1.0 - 0.0), 0.5 * (1.0 - 0.75)
    assert out == (w0 * 0.0 + w1 * 1.0) / (w0 + w1)


def test_output_conversions():
    vals = np.array([0.0, 1.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, -0.1, 1.2, math.nan, math.inf, -math.inf, 100.4 / 255])
    got = convert(vals, np.uint8)
    assert got.tolist() == [0, 255, 0, 2, 2, 0, 255, 0, 255, 0, 100]  # half to even; NaN -> 0
    assert convert(vals, np.float32).dtype == np.float32
    assert (convert(vals, np.float64).view(np.int64) == vals.view(np.int64)).all()
    assert (as_f64(np.array([0, 1, 255], np.uint8)) == np.array([0.0, 1.0, 255.0]) / 255.0).all()


def test_interpolation_error_on_the_committed_frames_beats_the_plain_blend():
    """Middlebury's interpolation error (Baker et al.): frame 2 of each committed triple from frames 1 and 3 at t = 0.5,
    with the oracle's flows of (1, 3) both ways, 5 levels, and their occlusion mask.  Measured here (mean absolute error,
    as float64 in [0, 1]): 240x135 0.009064 against 0.009856 for 0.5 (I1 + I3); 480x270 0.009442 against 0.013774."""
    import cases
    from _libs import OracleLib, build_oracle
    from test_fb_cpu import fb_reference
    build_oracle()
    L = OracleLib()
    for res in ("240", "480"):
        f1, f2, f3 = (cases.load_frame_u8(res, i) for i in (1, 2, 3))
        a, b = as_f64(f1), as_f64(f3)
        vx, vy = L.coarse2fine_flow(a, b, 5)[:2]
        bx, by = L.coarse2fine_flow(b, a, 5)[:2]
        fw, bw = np.stack([vx, vy])[None], np.stack([bx, by])[None]
        occ = fb_reference(fw, bw)
        got = interp_reference(f1[None], f3[None], fw, bw, [0.5], occ)[0, 0]
        err = np.abs(got - as_f64(f2)).mean()
        blend = np.abs(0.5 * (a + b) - as_f64(f2)).mean()
        assert err < blend, (res, err, blend)


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
_I = lambda: _z(2, 3, 8, 8)  # noqa: E731


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.interpolate(_I(), _I(), _F(), _F(), 0.5), ValueError),                            # CPU tensors
    (lambda: tensors.interpolate(None, _I(), _F(), _F(), 0.5), TypeError),
    (lambda: tensors.interpolate(_I(), _I(), _F(), _F(), 0.5, layout="CHWN"), ValueError),
    (lambda: tensors.interpolate(_z(2, 3, 8, 8, dtype=torch.int16), _I(), _F(), _F(), 0.5), TypeError),
    (lambda: tensors.interpolate(_I(), _z(2, 3, 8, 9), _F(), _F(), 0.5), ValueError),                 # frame shapes
    (lambda: tensors.interpolate(_z(2, 3, 8), _I(), _F(), _F(), 0.5), ValueError),
    (lambda: tensors.interpolate_pairs(_I(), _I(), 2, 0.5), ValueError),
    (lambda: tensors.interpolate_pairs(_I(), _I(), 0, 0.5), ValueError),                               # pyramid levels
    (lambda: tensors.interpolate_video(_z(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.interpolate_video(None, 2), TypeError),
    (lambda: tensors.interpolate_video(_z(1, 3, 8, 8), 2), ValueError),                               # fewer than 2 frames
    (lambda: tensors.interpolate_video(_z(3, 3, 8, 8), 2, layout="HWC"), ValueError),
    (lambda: tensors.interpolate_video(_z(3, 3, 8, 8), 2, consistency=(0.01,)), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("kw,exc", [
    (dict(times=0.0), ValueError), (dict(times=1.0), ValueError), (dict(times=-0.5), ValueError),      # times
    (dict(times=math.nan), ValueError), (dict(times=math.inf), ValueError), (dict(times=[0.5, 1.5]), ValueError),
    (dict(times=[]), ValueError), (dict(times=torch.tensor([[0.5]])), TypeError), (dict(times="half"), TypeError),
    (dict(times=None), TypeError), (dict(times=True), TypeError), (dict(times=torch.tensor([0.5, 0.0])), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError),                                     # flows
    (dict(flow_bw=_z(2, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(2, 3, 8, 8), flow_bw=_z(2, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(3, 2, 8, 8), flow_bw=_z(3, 2, 8, 8)), ValueError),                               # not (B, 2, H, W)
    (dict(flow_fw=_z(2, 2, 8, 9), flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_bw=_z(2, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError),
    (dict(flow_fw=_z(2, 2, 8, 8, device="meta"), flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),  # devices
    (dict(flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(occlusion=_z(2, 2, 8, 8)), TypeError), (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.int32)), TypeError),  # mask
    (dict(occlusion=_z(2, 1, 8, 8, dtype=torch.bool)), ValueError), (dict(occlusion=[0]), TypeError),
    (dict(occlusion=_z(2, 2, 8, 8, dtype=torch.bool, device="meta")), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),             # output dtype
])
def test_interpolate_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(flow_fw=_F(), flow_bw=_F(), times=[0.5])
    args.update(kw)
    with pytest.raises(exc):
        tensors.interpolate(_I(), _I(), args.pop("flow_fw"), args.pop("flow_bw"), args.pop("times"), **args)
    assert stub == []


def test_frames_and_flows_on_different_devices(stub, monkeypatch):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(ValueError):
        tensors.interpolate(_I(), _z(2, 3, 8, 8, device="meta"), _F(), _F(), 0.5)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(factor=1), ValueError), (dict(factor=0), ValueError), (dict(factor=2.5), ValueError),
    (dict(factor=True), ValueError), (dict(factor="2"), ValueError),
    (dict(out_dtype=torch.int16), TypeError), (dict(consistency=(0.01, -1.0)), ValueError),
    (dict(consistency="yes"), TypeError), (dict(bogus=1), TypeError),
])
def test_interpolate_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.interpolate_video(_z(3, 3, 8, 8), 2, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(times=1.0), ValueError), (dict(times=[]), ValueError), (dict(out_dtype=torch.int16), TypeError),
    (dict(consistency=(math.nan, 0.5)), ValueError), (dict(bogus=1), TypeError),
])
def test_interpolate_pairs_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    times = kw.pop("times", 0.5)
    with pytest.raises(exc):
        tensors.interpolate_pairs(_I(), _I(), 2, times, **kw)
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


def _call(lib, h, n=2, seq=0, size=(8, 8, 3), fr=_OK, fr2=_OK, fw=_OK, bw=_OK, occ=None, times=(0.5,), out=_OK, ts=1024):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "fr2": lambda: _t(capi.DTYPE_F32), "fw": lambda: _t(strides=(128, 8, 1, 64)),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)), "out": lambda: _t(capi.DTYPE_U8, (2048, 24, 3, 1))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, fr2=fr2, fw=fw, bw=bw, out=out).items()}
    d["occ"] = occ
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    tarr = (ctypes.c_double * max(1, len(times)))(*times) if times is not None else None
    return lib.papof_interp_tensor(h, n, seq, ref(d["fr"]), ref(d["fr2"]), size[0], size[1], size[2], ref(d["fw"]),
                                   ref(d["bw"]), ref(d["occ"]), len(times) if times is not None else 1, tarr, ref(d["out"]),
                                   ts, None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(fw=None), dict(bw=None), dict(out=None),                                        # NULL descriptors
    dict(fr=_t(data=0)), dict(fr2=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(out=_t(data=0)),  # NULL data
    dict(occ=_t(capi.DTYPE_U8, data=0)), dict(times=None),
    dict(fr=_t(dtype=3)), dict(fr2=_t(dtype=-1)),                                                       # frame dtypes
    dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),                                                   # flow dtypes
    dict(occ=_t(capi.DTYPE_F32)), dict(occ=_t(capi.DTYPE_F64)), dict(occ=_t(dtype=5)),                 # mask: U8 only
    dict(out=_t(dtype=3)),                                                                              # out dtype
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr2=_t(strides=(192, 24, -3, 1))),                     # negative strides
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),
    dict(occ=_t(capi.DTYPE_U8, (-128, 8, 1, 64))), dict(out=_t(strides=(2048, 24, 3, -1))), dict(ts=-1024),
    dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(2048, 0, 3, 1))),                        # zero out strides
    dict(out=_t(strides=(2048, 24, 0, 1))), dict(out=_t(strides=(2048, 24, 3, 0))),
    dict(times=(0.25, 0.5), ts=0),
    dict(seq=1), dict(fr2=None),                                                                        # frames2 by mode
    dict(times=()), dict(times=(0.0,)), dict(times=(1.0,)), dict(times=(-0.5,)), dict(times=(1.5,)),  # times
    dict(times=(math.nan,)), dict(times=(math.inf,)), dict(times=(0.5, -math.inf)), dict(times=(0.5, 1.0)),
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(size=(-1, 8, 3)),           # sizes
    dict(n=0), dict(n=-2),
])
def test_c_abi_interp_refuses(kw):
    lib = _lib()
    if kw.get("times") == ():  # n_times = 0 with a valid pointer
        t = (ctypes.c_double * 1)(0.5)
        args = dict(kw)
        del args["times"]
        fr, fr2, fw, bw, out = (_t(capi.DTYPE_U8), _t(capi.DTYPE_F32), _t(strides=(128, 8, 1, 64)),
                                _t(capi.DTYPE_F32, (128, 8, 1, 64)), _t(capi.DTYPE_U8, (2048, 24, 3, 1)))
        r = ctypes.byref
        assert lib.papof_interp_tensor(ctypes.cast(_FAKE, ctypes.c_void_p), 2, 0, r(fr), r(fr2), 8, 8, 3, r(fw), r(bw), None,
                                       0, t, r(out), 1024, None) == -1
        return
    assert _call(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_interp_without_a_handle():
    lib = _lib()
    assert _call(lib, None) == -1
    assert _call(lib, None, seq=1, fr2=None) == -1


def test_version():
    assert _lib().papof_version() >= 111
