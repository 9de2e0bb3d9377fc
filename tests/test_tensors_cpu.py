"""CPU-side checks of the device-tensor entry points (papteam_opticalflow_amd/tensors.py; include/papof.h:
papof_flow_batch_tensor): the descriptors handed to the C ABI for the layouts and views PyTorch produces, every argument
error raised before a launch (CPU tensors, a stubbed handle), and the C ABI's own refusals through ctypes.  No device is
touched here."""
import ctypes
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402


@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def test_import_does_not_touch_torch():
    code = "import sys, papteam_opticalflow_amd, papteam_opticalflow_amd.tensors; print('torch' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False"


def test_descriptor_contiguous_nchw_and_nhwc():
    t = torch.zeros(5, 3, 7, 11, dtype=torch.uint8)  # N C H W
    assert tensors.descriptor(t, "NCHW") == ((5, 7, 11, 3), (3 * 7 * 11, 11, 1, 7 * 11), capi.DTYPE_U8)
    t = torch.zeros(5, 7, 11, 3, dtype=torch.float32)  # N H W C
    assert tensors.descriptor(t, "NHWC") == ((5, 7, 11, 3), (7 * 11 * 3, 11 * 3, 3, 1), capi.DTYPE_F32)
    assert tensors.descriptor(t.double(), "NHWC")[2] == capi.DTYPE_F64


def test_descriptor_of_views():
    base = torch.zeros(9, 7, 11, 3, dtype=torch.uint8)  # NHWC storage
    sl = base[::2]
    assert tensors.descriptor(sl, "NHWC") == ((5, 7, 11, 3), (2 * 7 * 11 * 3, 11 * 3, 3, 1), capi.DTYPE_U8)
    nchw = base.permute(0, 3, 1, 2)  # an NCHW view of NHWC storage: the same strides in logical order
    assert tensors.descriptor(nchw, "NCHW") == tensors.descriptor(base, "NHWC")
    one = torch.zeros(1, 3, 7, 11).expand(4, 3, 7, 11)  # one frame repeated: a zero frame stride
    assert tensors.descriptor(one, "NCHW") == ((4, 7, 11, 3), (0, 11, 1, 77), capi.DTYPE_F32)
    crop = torch.zeros(2, 3, 20, 30, dtype=torch.float64)[:, 1:2, 3:13, 5:25]
    assert tensors.descriptor(crop, "NCHW") == ((2, 10, 20, 1), (1800, 30, 1, 600), capi.DTYPE_F64)


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8), 2), ValueError),                          # CPU tensors
    (lambda: tensors.flow_pairs(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, device="meta"), 2), ValueError),  # mixed devices
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8, dtype=torch.int32), 2), TypeError),       # wrong dtype
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8, dtype=torch.float16), 2), TypeError),
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8), 2, out_dtype=torch.uint8), TypeError),
    (lambda: tensors.flow_pairs(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 9), 2), ValueError),  # mismatched shapes
    (lambda: tensors.flow_pairs(torch.zeros(2, 3, 8, 8), torch.zeros(3, 3, 8, 8), 2), ValueError),
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8), 2, layout="CHWN"), ValueError),          # unknown layout
    (lambda: tensors.flow_video(torch.zeros(1, 3, 8, 8), 2), ValueError),                         # fewer than 2 frames
    (lambda: tensors.flow_video(torch.zeros(3, 8, 8), 2), ValueError),                            # 3-D video: one frame
    (lambda: tensors.flow_video(torch.zeros(2, 2, 3, 8, 8), 2), ValueError),                      # 5-D
    (lambda: tensors.flow_pairs(torch.zeros(2, 3, 8, 8), None, 2), TypeError),                    # not a tensor
    (lambda: tensors.flow_video(torch.zeros(3, 3, 8, 8), 0), ValueError),                         # pyramid levels
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


def test_solver_arguments_refused_before_any_launch(stub, monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: True)  # the CPU tensor passes for a device one up to the handle
    with pytest.raises(TypeError):
        tensors.flow_video(torch.zeros(3, 3, 8, 8), 2, bogus=1)
    assert stub == []


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


def _call(lib, h, n_pairs=2, sequence=1, frames="ok", frames2=None, flow="ok", warp="ok", hwc=(8, 8, 1), levels=2):
    fr = _t(capi.DTYPE_U8) if frames == "ok" else frames
    fl = _t(capi.DTYPE_F32, (128, 8, 1, 64)) if flow == "ok" else flow
    wp = _t(capi.DTYPE_F64, (64, 8, 1, 1)) if warp == "ok" else warp
    ref = lambda d: ctypes.byref(d) if d is not None else None  # noqa: E731
    t = (ctypes.c_double * capi.N_TIMERS)()
    return lib.papof_flow_batch_tensor(h, n_pairs, sequence, ref(fr), ref(frames2), hwc[0], hwc[1], hwc[2], levels, None,
                                       ref(fl), ref(wp), None, t)


@pytest.mark.parametrize("kw", [
    dict(frames=None), dict(flow=None), dict(warp=None),
    dict(frames=_t(data=0)), dict(flow=_t(data=0)), dict(warp=_t(data=0)),                      # null data
    dict(frames=_t(dtype=3)), dict(frames=_t(dtype=-1)),                                        # unknown dtype
    dict(flow=_t(dtype=capi.DTYPE_U8, strides=(128, 8, 1, 64))),                                # uint8 output
    dict(warp=_t(dtype=capi.DTYPE_U8, strides=(64, 8, 1, 1))),
    dict(frames=_t(strides=(64, -8, 1, 0))), dict(flow=_t(strides=(128, 8, -1, 64))),           # negative strides
    dict(flow=_t(strides=(128, 8, 1, 0))), dict(warp=_t(strides=(0, 8, 1, 1))),                 # zero output strides
    dict(frames2=_t()),                                                                          # frames2 in sequence mode
    dict(sequence=0),                                                                            # pair mode without frames2
    dict(n_pairs=0), dict(hwc=(0, 8, 1)), dict(hwc=(8, 8, 0)), dict(levels=0),
])
def test_c_abi_refuses_bad_descriptors(kw):
    lib = _lib()
    assert _call(lib, ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle():
    lib = _lib()
    assert _call(lib, None) in (-1, -2)
    assert _call(lib, None, sequence=0, frames2=_t()) in (-1, -2)
