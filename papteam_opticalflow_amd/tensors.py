"""Flow on PyTorch device tensors (include/papof.h: papof_flow_batch_tensor): batches of frames that are already on the GPU go
in, flow tensors come out, and nothing crosses PCIe.

    from papteam_opticalflow_amd.tensors import flow_pairs, flow_video
    flow, warpI2, timing = flow_video(frames, 5, layout="NHWC")   # frames: (T, H, W, C) uint8 on cuda:0

Inputs are 4-D tensors on one HIP device (a 3-D tensor is a batch of one) of uint8, float32 or float64, with any non-negative
strides: slices, `permute`d and expanded views are read in place.  `layout` names the axes ("NCHW", PyTorch's convention, or
"NHWC", what video decoders return); it is not inferred, because C == W is ambiguous.  `flow` is (B, 2, H, W) (vx, vy),
`warpI2` has the input's layout; both are new tensors of `out_dtype` (float64, the reference's arithmetic, or float32) on the
input's device, with no autograd graph.  Every pair is bit-identical to the single call on the fp64 values of its frames
(uint8: x / 255.).

Stream contract: the call is ordered behind the work queued so far on `torch.cuda.current_stream(device)` and returns once the
outputs are written -- stream-ordered on entry, complete on return, not asynchronous.

torch is imported when a function is called, not when the package is imported.
"""
import ctypes
import threading

from . import capi

LAYOUTS = ("NCHW", "NHWC")

_lock = threading.Lock()
_handles = {}  # device ordinal -> (Papof, lock of its calls)


def _torch():
    import torch
    return torch


def dtype_code(dtype):
    """PAPOF_DTYPE_* of an input dtype (TypeError for anything else)"""
    torch = _torch()
    codes = {torch.uint8: capi.DTYPE_U8, torch.float32: capi.DTYPE_F32, torch.float64: capi.DTYPE_F64}
    if dtype not in codes:
        raise TypeError("frames must be uint8, float32 or float64, got %s" % dtype)
    return codes[dtype]


def descriptor(t, layout):
    """(sizes, strides, dtype code) of a 4-D tensor in the logical order (frame, row, column, channel) of the C ABI; strides
    in elements.  Plain function of the tensor's metadata: works on CPU tensors."""
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    if t.dim() != 4:
        raise ValueError("expected a 4-D tensor, got shape %s" % (tuple(t.shape),))
    order = (0, 2, 3, 1) if layout == "NCHW" else (0, 1, 2, 3)
    sizes = tuple(int(t.shape[i]) for i in order)
    strides = tuple(int(t.stride(i)) for i in order)
    return sizes, strides, dtype_code(t.dtype)


def _struct(t, strides, code):
    d = capi.PapofTensor()
    d.data = t.data_ptr()
    d.dtype = code
    for i in range(4):
        d.stride[i] = strides[i]
    return d


def _on_gpu(t):
    """the tensor lives on a HIP device (tests stub this to walk the argument path with CPU tensors)"""
    return t.device.type == "cuda"


def _as4d(name, t):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dim() == 3:
        return t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError("%s must be a 4-D tensor (or 3-D: a batch of one), got shape %s" % (name, tuple(t.shape)))
    return t


def _check(named, layout, out_dtype, levels, min_frames=1):
    """every argument error, before anything is launched: (4-D tensors, their descriptors, the output dtype)"""
    torch = _torch()
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (LAYOUTS, layout))
    if int(levels) < 1:
        raise ValueError("pyramidLevels must be >= 1")
    ts = [_as4d(n, t) for n, t in named]
    descs = [descriptor(t, layout) for t in ts]
    if out_dtype is None:
        out_dtype = torch.float64
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("out_dtype must be torch.float32 or torch.float64, got %s" % out_dtype)
    if len(ts) == 2 and descs[1][0] != descs[0][0]:
        raise ValueError("im1 %s and im2 %s differ in shape" % (tuple(ts[0].shape), tuple(ts[1].shape)))
    if min(descs[0][0][1:]) < 1:
        raise ValueError("empty frames: shape %s" % (tuple(ts[0].shape),))
    if descs[0][0][0] < min_frames:
        raise ValueError("%s needs at least %d frames, got %d" % (named[0][0], min_frames, descs[0][0][0]))
    dev = ts[0].device
    for (n, _), t in zip(named, ts):
        if t.device != dev:
            raise ValueError("%s is on %s, %s on %s: all frames must be on one device" % (n, t.device, named[0][0], dev))
    if not _on_gpu(ts[0]):
        raise ValueError("frames must be on a HIP device (cuda:N), got %s" % dev)
    return ts, descs, out_dtype


def _handle(device):
    """one Papof handle per device ordinal for the process, and the lock that serialises its calls"""
    with _lock:
        if device not in _handles:
            _torch().cuda.init()  # PyTorch first, then the handle: both share PyTorch's HIP runtime (README)
            _handles[device] = (capi.Papof(device), threading.Lock())
        return _handles[device]


def _run(ts, descs, sequence, n_pairs, layout, out_dtype, levels, solver):
    torch = _torch()
    params = capi.default_params(**solver) if solver else None
    (_, H, W, C), _, _ = descs[0]
    dev = ts[0].device
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    flow = torch.empty((n_pairs, 2, H, W), dtype=out_dtype, device=dev)
    if layout == "NCHW":
        warp = torch.empty((n_pairs, C, H, W), dtype=out_dtype, device=dev)
    else:
        warp = torch.empty((n_pairs, H, W, C), dtype=out_dtype, device=dev)
    out_code = capi.DTYPE_F32 if out_dtype == torch.float32 else capi.DTYPE_F64
    d_in = [_struct(t, s, c) for t, (_, s, c) in zip(ts, descs)]
    d_flow = _struct(flow, (2 * H * W, W, 1, H * W), out_code)
    d_warp = _struct(warp, descriptor(warp, layout)[1], out_code)
    t = (ctypes.c_double * capi.N_TIMERS)()
    gpu, lock = _handle(index)
    with lock, torch.cuda.device(index):
        stream = torch.cuda.current_stream(index).cuda_stream
        rc = gpu.L.papof_flow_batch_tensor(gpu.h, n_pairs, 1 if sequence else 0, ctypes.byref(d_in[0]),
                                           None if sequence else ctypes.byref(d_in[1]), H, W, C, int(levels),
                                           ctypes.byref(params) if params is not None else None, ctypes.byref(d_flow),
                                           ctypes.byref(d_warp), ctypes.c_void_p(stream or None), t)
    capi._chk(rc, "papof_flow_batch_tensor")
    return flow, warp, capi.format_timing(list(t))


def flow_pairs(im1, im2, pyramidLevels, *, layout="NCHW", out_dtype=None, **solver):
    """Flow of the independent pairs (im1[i], im2[i]): two tensors of one shape, (B, C, H, W) or (B, H, W, C) by `layout`.
    Returns (flow (B, 2, H, W), warpI2 (B, ...) in `layout`, the reference's dict of ten timers)."""
    ts, descs, out_dtype = _check([("im1", im1), ("im2", im2)], layout, out_dtype, pyramidLevels)
    return _run(ts, descs, False, descs[0][0][0], layout, out_dtype, pyramidLevels, solver)


def flow_video(frames, pyramidLevels, *, layout="NCHW", out_dtype=None, **solver):
    """Flow of the consecutive pairs (frames[i], frames[i + 1]) of T >= 2 frames (each frame's pyramid is built once).
    Returns (flow (T - 1, 2, H, W), warpI2 (T - 1, ...) in `layout`, the reference's dict of ten timers)."""
    ts, descs, out_dtype = _check([("frames", frames)], layout, out_dtype, pyramidLevels, min_frames=2)
    return _run(ts, descs, True, descs[0][0][0] - 1, layout, out_dtype, pyramidLevels, solver)
