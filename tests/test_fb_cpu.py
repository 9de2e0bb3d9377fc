"""CPU-side checks of the forward-backward entry points (papteam_opticalflow_amd/tensors.py: flow_video_fb, flow_pairs_fb,
fb_consistency; include/papof.h: papof_flow_batch_tensor_fb, papof_fb_check_tensor): every Python argument error raised
before a launch (CPU tensors, a stubbed handle), each refusal of the C ABI through ctypes, and the numpy restatement of the
consistency check that tests/test_gpu_fb.py compares the device's masks with.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402


def fb_reference(fw, bw, alpha1=0.01, alpha2=0.5):
    """The check of include/papof.h (papof_flow_batch_tensor_fb) restated in numpy fp64: fw, bw (B, 2, H, W) flows ->
    uint8 (B, 2, H, W), 1 = occluded; channel 0 follows fw into bw, channel 1 bw into fw.  Bilinear sampling by the
    reference's rule (src/ImageProcessing.h:138-157): truncation toward zero, fraction clamped to [0, 1], neighbours clamped
    into the image, taps accumulated from 0 in (m, n) order.  numpy does not contract a * b + c: the bits are the kernel's."""
    fw, bw = np.asarray(fw, dtype=np.float64), np.asarray(bw, dtype=np.float64)
    B, _, H, W = fw.shape
    out = np.empty((B, 2, H, W), np.uint8)
    pb = np.arange(B)[:, None, None]
    for d, (f, b) in enumerate(((fw, bw), (bw, fw))):
        u, v = f[:, 0], f[:, 1]
        X = np.arange(W, dtype=np.float64)[None, None, :] + u
        Y = np.arange(H, dtype=np.float64)[None, :, None] + v
        inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
        Xc, Yc = np.where(inside, X, 0.0), np.where(inside, Y, 0.0)
        xx, yy = Xc.astype(np.int64), Yc.astype(np.int64)
        dx, dy = Xc - xx, Yc - yy
        dx = np.where(dx > 1, 1.0, dx)
        dx = np.where(dx < 0, 0.0, dx)
        dy = np.where(dy > 1, 1.0, dy)
        dy = np.where(dy < 0, 0.0, dy)
        bu, bv = np.zeros_like(u), np.zeros_like(v)
        for m in (0, 1):
            for n in (0, 1):
                cu, cv = np.clip(xx + m, 0, W - 1), np.clip(yy + n, 0, H - 1)
                s = np.abs(float(1 - m) - dx) * np.abs(float(1 - n) - dy)
                bu = bu + b[pb, 0, cv, cu] * s
                bv = bv + b[pb, 1, cv, cu] * s
        du, dv = u + bu, v + bv
        e = du * du + dv * dv
        mag = (u * u + v * v) + (bu * bu + bv * bv)
        with np.errstate(invalid="ignore"):
            ok = e <= alpha1 * mag + alpha2
        out[:, d] = (~inside | ~ok).astype(np.uint8)
    return out


def test_reference_of_consistent_and_inconsistent_flows():
    H, W = 5, 7
    fw = np.zeros((1, 2, H, W))
    fw[:, 0] = 1.0  # one column to the right ...
    bw = np.zeros((1, 2, H, W))
    bw[:, 0] = -1.0  # ... and back
    m = fb_reference(fw, bw)
    assert not m[0, 0, :, :-1].any() and m[0, 0, :, -1].all()  # the last column leaves the image
    assert not m[0, 1, :, 1:].any() and m[0, 1, :, 0].all()
    assert fb_reference(fw, np.zeros_like(bw))[0, 0, :, :-1].all()  # 1 + 0 against 0.01 * 1 + 0.5: occluded
    fw[0, 0, 2, 3] = math.nan
    assert fb_reference(fw, bw)[0, 0, 2, 3] == 1


def test_reference_at_the_bound_is_not_occluded():
    fw = np.zeros((1, 2, 3, 4))
    fw[:, 0] = 0.5
    bw = np.zeros_like(fw)
    # e = 0.25, m = 0.25: e == 0.5 * m + 0.125 exactly
    assert not fb_reference(fw, bw, 0.5, 0.125)[0, 0, :, :-1].any()
    assert fb_reference(fw, bw, 0.5, 0.124)[0, 0, :, :-1].all()


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2), ValueError),                                  # CPU tensors
    (lambda: tensors.flow_pairs_fb(_z(2, 3, 8, 8), _z(2, 3, 8, 8, device="meta"), 2), ValueError),  # mixed devices
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8, dtype=torch.int32), 2), TypeError),               # wrong dtype
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, out_dtype=torch.uint8), TypeError),
    (lambda: tensors.flow_pairs_fb(_z(2, 3, 8, 8), _z(2, 3, 8, 9), 2), ValueError),                 # mismatched shapes
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, layout="CHWN"), ValueError),                  # unknown layout
    (lambda: tensors.flow_video_fb(_z(1, 3, 8, 8), 2), ValueError),                                 # fewer than 2 frames
    (lambda: tensors.flow_pairs_fb(_z(2, 3, 8, 8), None, 2), TypeError),                            # not a tensor
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 0), ValueError),                                 # pyramid levels
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, consistency=(0.01,)), TypeError),             # consistency
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, consistency=0.5), TypeError),
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, consistency=(-0.01, 0.5)), ValueError),
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, consistency=(0.01, math.inf)), ValueError),
    (lambda: tensors.flow_video_fb(_z(3, 3, 8, 8), 2, consistency=(math.nan, 0.5)), ValueError),
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), _z(2, 2, 8, 8)), ValueError),                   # CPU flows
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), None), TypeError),
    (lambda: tensors.fb_consistency(_z(2, 3, 8, 8), _z(2, 3, 8, 8)), ValueError),                   # not (B, 2, H, W)
    (lambda: tensors.fb_consistency(_z(2, 8, 8), _z(2, 8, 8)), ValueError),
    (lambda: tensors.fb_consistency(_z(0, 2, 8, 8), _z(0, 2, 8, 8)), ValueError),
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), _z(2, 2, 8, 9)), ValueError),                   # mismatched shapes
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8, dtype=torch.uint8), _z(2, 2, 8, 8)), TypeError),  # uint8 flow
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8, dtype=torch.float16), _z(2, 2, 8, 8)), TypeError),
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), _z(2, 2, 8, 8, device="meta")), ValueError),    # mixed devices
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), _z(2, 2, 8, 8), alpha1=-1), ValueError),        # alphas
    (lambda: tensors.fb_consistency(_z(2, 2, 8, 8), _z(2, 2, 8, 8), alpha2=math.nan), ValueError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


def test_argument_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)  # the CPU tensor passes for a device one up to the handle
    with pytest.raises(TypeError):
        tensors.flow_video_fb(_z(3, 3, 8, 8), 2, bogus=1)
    with pytest.raises(ValueError):
        tensors.flow_pairs_fb(_z(2, 3, 8, 8), _z(2, 3, 8, 8), 2, consistency=(0.01, -0.5))
    assert stub == []


def test_flow_video_and_flow_pairs_keep_their_signature():
    """the new keyword belongs to the fb calls only: flow_video / flow_pairs hand every keyword to default_params"""
    import inspect
    for fn in (tensors.flow_video, tensors.flow_pairs):
        assert "consistency" not in inspect.signature(fn).parameters


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(64, 8, 1, 0), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"


def _flow():
    return _t(capi.DTYPE_F32, (128, 8, 1, 64))


def _warp():
    return _t(capi.DTYPE_F64, (64, 8, 1, 1))


def _occ():
    return _t(capi.DTYPE_U8, (128, 8, 1, 64))


def _call_fb(lib, h, n_pairs=2, sequence=1, frames=_OK, frames2=None, flow_fw=_OK, warp_fw=_OK, flow_bw=_OK, warp_bw=_OK,
             occ=_OK, alphas=(0.01, 0.5), hwc=(8, 8, 1), levels=2):
    pick = lambda d, make: make() if isinstance(d, str) else d  # noqa: E731
    ref = lambda d: ctypes.byref(d) if d is not None else None  # noqa: E731
    t = (ctypes.c_double * capi.N_TIMERS)()
    return lib.papof_flow_batch_tensor_fb(h, n_pairs, sequence, ref(pick(frames, lambda: _t(capi.DTYPE_U8))), ref(frames2),
                                          hwc[0], hwc[1], hwc[2], levels, None, ref(pick(flow_fw, _flow)),
                                          ref(pick(warp_fw, _warp)), ref(pick(flow_bw, _flow)), ref(pick(warp_bw, _warp)),
                                          ref(pick(occ, _occ)), alphas[0], alphas[1], None, t)


@pytest.mark.parametrize("kw", [
    # everything papof_flow_batch_tensor refuses
    dict(frames=None), dict(flow_fw=None), dict(warp_fw=None), dict(flow_bw=None), dict(warp_bw=None),
    dict(frames=_t(data=0)), dict(flow_bw=_t(data=0)), dict(warp_bw=_t(data=0)),                # null data
    dict(frames=_t(dtype=3)), dict(frames=_t(dtype=-1)),                                        # unknown dtype
    dict(frames=_t(strides=(64, -8, 1, 0))), dict(flow_bw=_t(strides=(128, 8, -1, 64))),        # negative strides
    dict(frames2=_t()), dict(sequence=0),                                                       # frames2 by mode
    dict(n_pairs=0), dict(hwc=(0, 8, 1)), dict(hwc=(8, 8, 0)), dict(levels=0),
    # uint8 flow (and warp) outputs
    dict(flow_fw=_t(capi.DTYPE_U8, (128, 8, 1, 64))), dict(flow_bw=_t(capi.DTYPE_U8, (128, 8, 1, 64))),
    dict(warp_bw=_t(capi.DTYPE_U8, (64, 8, 1, 1))),
    # a zero stride on any output
    dict(flow_fw=_t(strides=(128, 8, 1, 0))), dict(warp_fw=_t(strides=(0, 8, 1, 1))),
    dict(flow_bw=_t(strides=(128, 0, 1, 64))), dict(warp_bw=_t(strides=(64, 8, 0, 1))),
    dict(occ=_t(capi.DTYPE_U8, (128, 8, 1, 0))), dict(occ=_t(capi.DTYPE_U8, (0, 8, 1, 64))),
    # a mask that is not uint8, or not there
    dict(occ=_t(capi.DTYPE_F32, (128, 8, 1, 64))), dict(occ=_t(capi.DTYPE_F64, (128, 8, 1, 64))),
    dict(occ=_t(capi.DTYPE_U8, (128, 8, 1, 64), data=0)), dict(occ=_t(capi.DTYPE_U8, (128, -8, 1, 64))),
    # negative or non-finite alphas
    dict(alphas=(-0.01, 0.5)), dict(alphas=(0.01, -1e-300)), dict(alphas=(math.nan, 0.5)), dict(alphas=(0.01, math.inf)),
    dict(alphas=(-math.inf, 0.5)), dict(occ=None, alphas=(0.01, math.nan)),
])
def test_c_abi_fb_refuses(kw):
    lib = _lib()
    assert _call_fb(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_fb_without_a_handle():
    lib = _lib()
    assert _call_fb(lib, None) in (-1, -2)
    assert _call_fb(lib, None, occ=None) in (-1, -2)


def _call_check(lib, h, n_pairs=2, hw=(8, 8), fw=_OK, bw=_OK, occ=_OK, alphas=(0.01, 0.5)):
    pick = lambda d, make: make() if isinstance(d, str) else d  # noqa: E731
    ref = lambda d: ctypes.byref(d) if d is not None else None  # noqa: E731
    return lib.papof_fb_check_tensor(h, n_pairs, hw[0], hw[1], ref(pick(fw, _flow)), ref(pick(bw, _flow)), alphas[0],
                                     alphas[1], ref(pick(occ, _occ)), None)


@pytest.mark.parametrize("kw", [
    dict(fw=None), dict(bw=None), dict(occ=None),
    dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(occ=_t(capi.DTYPE_U8, (128, 8, 1, 64), data=0)),
    dict(fw=_t(capi.DTYPE_U8, (128, 8, 1, 64))), dict(bw=_t(dtype=3)),                          # flows: F32 / F64 only
    dict(fw=_t(strides=(128, 8, -1, 64))),                                                      # negative flow stride
    dict(occ=_t(capi.DTYPE_F64, (128, 8, 1, 64))), dict(occ=_t(capi.DTYPE_U8, (128, 8, 0, 64))),
    dict(alphas=(-1.0, 0.5)), dict(alphas=(0.01, math.nan)),
    dict(n_pairs=0), dict(hw=(0, 8)), dict(hw=(8, 0)),
])
def test_c_abi_check_refuses(kw):
    lib = _lib()
    assert _call_check(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_check_without_a_handle():
    assert _call_check(_lib(), None) == -1
