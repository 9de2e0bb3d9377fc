"""The initial flow without a GPU: the oracle composition of tests/_init_ref.py against orc_coarse2fine_flow bit for bit (it
is the restatement the GPU tests hold the library to), every Python argument error of init_flow / init_flow_bw raised before
a launch (CPU tensors, a stubbed handle), and the C ABI's refusals of an initial-flow descriptor through ctypes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import cases  # noqa: E402
from _init_ref import BICUBIC, BILINEAR, GMIXTURE, LAPLACIAN, coarse2fine_init, init_scale  # noqa: E402
from _libs import OracleLib  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402


@pytest.fixture(scope="module")
def orc():
    return OracleLib()


@pytest.fixture(scope="module")
def pair():
    return cases.load_pair("240")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("levels,interp,noise", [(1, BILINEAR, LAPLACIAN), (3, BILINEAR, LAPLACIAN), (5, BILINEAR, LAPLACIAN),
                                                 (8, BILINEAR, LAPLACIAN), (3, BICUBIC, LAPLACIAN),
                                                 (3, BILINEAR, GMIXTURE)])
def test_composition_without_init_is_the_oracle_call(orc, pair, levels, interp, noise):
    a, b = pair
    p = orc.default_params()
    p.interpolation, p.noise_model = interp, noise
    vx, vy, wi, _ = orc.coarse2fine_flow(a, b, levels, p)
    gx, gy, gw = coarse2fine_init(orc, a, b, levels, None, interp, noise)
    for got, want, what in ((gx, vx, "vx"), (gy, vy, "vy"), (gw, wi, "warpI2")):
        assert np.array_equal(_bits(got), _bits(want)), (levels, interp, noise, what)


def test_the_scale_is_a_product_of_ratios():
    assert init_scale(1) == 1.0
    assert init_scale(3) == 0.75 * 0.75
    assert init_scale(5, ratio=0.2) == init_scale(5)  # the pyramid's clamp


def test_an_initial_flow_changes_the_result(orc, pair):
    """the composition does use init: a uniform (3, -2) px start moves the 1-level flow"""
    a, b = pair
    h, w = a.shape[:2]
    init = np.zeros((h, w, 2))
    init[..., 0], init[..., 1] = 3.0, -2.0
    x0, _, _ = coarse2fine_init(orc, a, b, 1)
    x1, _, _ = coarse2fine_init(orc, a, b, 1, init)
    assert np.abs(x1 - x0).mean() > 1.0


# ---- Python argument errors, before anything is launched (CPU tensors pass for device ones up to the handle)
torch = pytest.importorskip("torch")


@pytest.fixture
def stub(monkeypatch):
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")
    return calls


def _frames(B=3, H=6, W=7, C=3):
    return torch.zeros((B, C, H, W), dtype=torch.uint8)


def _init(B=3, H=6, W=7, dtype=torch.float64):
    return torch.zeros((B, 2, H, W), dtype=dtype)


@pytest.mark.parametrize("init,exc", [
    ("not a tensor", TypeError),
    (np.zeros((3, 2, 6, 7)), TypeError),
    (_init(dtype=torch.float16), TypeError),
    (torch.zeros((3, 2, 6, 7), dtype=torch.int32), TypeError),
    (_init(B=2), ValueError),                        # wrong B
    (_init(B=4), ValueError),
    (_init(H=5), ValueError),                        # wrong H
    (_init(W=8), ValueError),                        # wrong W
    (torch.zeros((3, 3, 6, 7), dtype=torch.float64), ValueError),   # not 2 components
    (torch.zeros((3, 6, 7, 2), dtype=torch.float64), ValueError),   # NHWC is not accepted as is
    (torch.zeros((3, 6, 7), dtype=torch.float64), ValueError),
    (torch.zeros((2, 6), dtype=torch.float64), ValueError),
    (torch.zeros((1, 3, 2, 6, 7), dtype=torch.float64), ValueError),
    (torch.zeros((3, 2, 6, 7), dtype=torch.float64, device="meta"), ValueError),   # another device
])
@pytest.mark.parametrize("fn", ["pairs", "video", "pairs_fb", "video_fb", "video_fb_bw"])
def test_init_argument_errors_before_any_launch(stub, init, exc, fn):
    fr = _frames()
    with pytest.raises(exc):
        if fn == "pairs":
            tensors.flow_pairs(fr, fr, 2, init_flow=init)
        elif fn == "video":
            tensors.flow_video(_frames(B=4), 2, init_flow=init)
        elif fn == "pairs_fb":
            tensors.flow_pairs_fb(fr, fr, 2, init_flow=init)
        elif fn == "video_fb":
            tensors.flow_video_fb(_frames(B=4), 2, init_flow=init)
        else:
            tensors.flow_video_fb(_frames(B=4), 2, init_flow_bw=init)
    assert stub == []


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e7, -1.0000001e6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_refused_values_raise_before_any_launch(stub, bad, dtype):
    init = _init(dtype=dtype)
    init[0, 0, 2, 3] = bad
    fr = _frames()
    with pytest.raises(ValueError):
        tensors.flow_pairs(fr, fr, 2, init_flow=init)
    with pytest.raises(ValueError):
        tensors.flow_pairs_fb(fr, fr, 2, init_flow_bw=init)
    with pytest.raises(ValueError):
        tensors.flow_video(_frames(B=4), 2, init_flow=init[0])  # the broadcast form
    assert stub == []


def test_the_bound_itself_is_accepted(stub, monkeypatch):
    """|x| == 1e6 passes the checks and reaches the handle (the stub), as does a broadcast (2, H, W) flow"""
    monkeypatch.setattr(tensors, "_index", lambda dev: 0)
    init = _init()
    init[0, 1, 0, 0] = -1e6
    fr = _frames()
    with pytest.raises(TypeError):  # the stubbed handle returns None: the call fails after the checks
        tensors.flow_pairs(fr, fr, 2, init_flow=init)
    with pytest.raises(TypeError):
        tensors.flow_video(_frames(B=4), 2, init_flow=init[0].expand(2, 6, 7))
    assert stub == [0, 0]


def test_the_new_keywords():
    import inspect
    for fn in (tensors.flow_pairs, tensors.flow_video):
        ps = inspect.signature(fn).parameters
        assert ps["init_flow"].default is None and "init_flow_bw" not in ps
    for fn in (tensors.flow_pairs_fb, tensors.flow_video_fb):
        ps = inspect.signature(fn).parameters
        assert ps["init_flow"].default is None and ps["init_flow_bw"].default is None


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
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


def _ref(d):
    return ctypes.byref(d) if d is not None else None


def _call(lib, h, init, n_pairs=2, sequence=1, frames=_OK, flow=_OK):
    t = (ctypes.c_double * capi.N_TIMERS)()
    fr = _t(capi.DTYPE_U8) if frames is _OK else frames
    return lib.papof_flow_batch_tensor_init(h, n_pairs, sequence, _ref(fr), None, 8, 8, 1, 2, None, _ref(init),
                                            _ref(_flow() if flow is _OK else flow), _ref(_warp()), None, t)


def _call_fb(lib, h, init_fw, init_bw, occ=True):
    t = (ctypes.c_double * capi.N_TIMERS)()
    return lib.papof_flow_batch_tensor_fb_init(h, 2, 1, _ref(_t(capi.DTYPE_U8)), None, 8, 8, 1, 2, None, _ref(init_fw),
                                               _ref(init_bw), _ref(_flow()), _ref(_warp()), _ref(_flow()), _ref(_warp()),
                                               _ref(_t(capi.DTYPE_U8, (128, 8, 1, 64))) if occ else None, 0.01, 0.5, None,
                                               t)


_BAD_INITS = [
    _t(data=0),                                  # NULL data
    _t(capi.DTYPE_U8), _t(dtype=3), _t(dtype=-1),  # not F32 / F64
    _t(strides=(-128, 8, 1, 64)), _t(strides=(128, -8, 1, 64)), _t(strides=(128, 8, -1, 64)),
    _t(strides=(128, 8, 1, -64)),                # negative strides
]


@pytest.mark.parametrize("init", _BAD_INITS)
def test_c_abi_refuses_bad_init_descriptors(init):
    lib = _lib()
    h = ctypes.cast(_FAKE, ctypes.c_void_p)
    assert _call(lib, h, init) == -1
    assert _call_fb(lib, h, init, None) == -1
    assert _call_fb(lib, h, None, init) == -1
    assert _call_fb(lib, h, _t(strides=(0, 8, 1, 64)), init, occ=False) == -1


@pytest.mark.parametrize("kw", [dict(n_pairs=0), dict(frames=None), dict(frames=_t(data=0)), dict(flow=None),
                                dict(flow=_t(capi.DTYPE_U8, (128, 8, 1, 64))), dict(sequence=0)])
def test_c_abi_init_refuses_what_the_call_without_init_refuses(kw):
    lib = _lib()
    assert _call(lib, ctypes.cast(_FAKE, ctypes.c_void_p), _t(strides=(0, 8, 1, 64)), **kw) == -1


def test_c_abi_init_without_a_handle():
    lib = _lib()
    assert _call(lib, None, None) == -1
    assert _call_fb(lib, None, None, None) == -1


def test_version():
    assert _lib().papof_version() >= 112
