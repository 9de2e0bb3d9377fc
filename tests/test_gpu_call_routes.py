"""Every route through the single call (csrc/api.hip: flow_pass) returns the oracle's bytes.

One 37 x 53 three-channel uint8 pair -- an image and its shift by (1, 2) -- at 3 pyramid levels (every level derived from
level 0) and at 7 (the pyramid chains through finer levels), through: the host call with and without stream overlap, the
three timing modes, the device-resident call, the uint8 and the float64 entry, a sequence from host and from device
frames, page-locked result arrays, and a batch of two identical pairs through the tensor call.  `.tobytes()` equality: the
sign of a zero counts.  The timers are checked for what is measured, never for how long it took.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:  # loaded ahead of the library, as in test_gpu_tensors.py (both bring a HIP runtime); only the tensor route needs it
    import torch
except ImportError:
    torch = None

H, W, C = 37, 53, 3
LEVELS = (3, 7)
NAMES = ("vx", "vy", "warpI2")
T_SOR, T_TOTAL = 6, 9  # Phase5_SOR, Total C++ Execution (include/papof.h: the order of the ten timers)


def _pair():
    rng = np.random.default_rng(37 * 53)
    a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    return a, np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))


def _f64(u8):
    return u8.astype(np.float64) / 255.0


@pytest.fixture(scope="module")
def pair():
    return _pair()


@pytest.fixture(scope="module")
def want(oracle, pair):
    """the oracle's (vx, vy, warpI2) per level count: computed once, never written to"""
    out = {}
    for levels in LEVELS:
        r = oracle.coarse2fine_flow(_f64(pair[0]), _f64(pair[1]), levels)[:3]
        for x in r:
            x.flags.writeable = False
        out[levels] = r
    return out


@pytest.fixture(scope="module")
def gpu():
    from papteam_opticalflow_amd import Papof
    g = Papof(0)
    yield g
    g.close()


def _same(got, want, route):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %s differs from the oracle" % (route, name)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("overlap", [True, False])
def test_host_call_u8_and_f64_with_and_without_overlap(gpu, pair, want, levels, overlap):
    gpu.set_stream_overlap(overlap)
    try:
        _same(gpu.coarse2fine_flow_u8(pair[0], pair[1], levels)[:3], want[levels], "uint8 host call")
        _same(gpu.coarse2fine_flow(_f64(pair[0]), _f64(pair[1]), levels)[:3], want[levels], "float64 host call")
    finally:
        gpu.set_stream_overlap(True)


@pytest.mark.parametrize("levels", LEVELS)
def test_timing_modes(gpu, pair, want, levels):
    from papteam_opticalflow_amd import default_params
    timers = {}
    for mode in (0, 1, 2):
        r = gpu.coarse2fine_flow_u8(pair[0], pair[1], levels, default_params(phase_timing=mode))
        _same(r[:3], want[levels], "phase_timing = %d" % mode)
        timers[mode] = r[3]
        print("L%d phase_timing %d: %s" % (levels, mode, " ".join("%.3e" % x for x in r[3])))
    t1 = timers[1]  # all ten phases on one stream
    assert len(t1) == 10 and np.all(np.isfinite(t1)) and np.all(t1 >= 0)
    assert t1[T_TOTAL] > 0 and t1[T_SOR] > 0
    # only the total and the solver kernels' own time are measured (the set the parent commit's library gives)
    assert {i for i in range(10) if timers[2][i] == 0.0} == set(range(10)) - {T_SOR, T_TOTAL}


def _device_call(gpu, a, b, levels, u8):
    n = H * W
    d = [gpu.dev_alloc(x.nbytes) for x in (a, b)] + [gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n * C)]
    try:
        gpu.dev_upload(d[0], a)
        gpu.dev_upload(d[1], b)
        if u8:
            t = np.zeros(10)
            rc = gpu.L.papof_flow_device_u8(gpu.h, d[0], d[1], H, W, C, levels, None, d[2], d[3], d[4],
                                            t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
            assert rc == 0
        else:
            gpu.flow_device(d[0], d[1], H, W, C, levels, None, d[2], d[3], d[4])
        out = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, C))
        for arr, p in zip(out, d[2:]):
            gpu.dev_download(arr, p)
        return out
    finally:
        for p in d:
            gpu.dev_free(p)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("u8", [True, False])
def test_device_resident_call(gpu, pair, want, levels, u8):
    a, b = pair if u8 else (_f64(pair[0]), _f64(pair[1]))
    _same(_device_call(gpu, a, b, levels, u8), want[levels], "device-resident call")


@pytest.mark.parametrize("levels", LEVELS)
def test_sequence_from_host_and_from_device_frames(gpu, pair, want, levels):
    gpu.seq_reset()
    assert gpu.seq_push(pair[0], levels) is None  # primes
    _same(gpu.seq_push(pair[1], levels)[:3], want[levels], "sequence, host frames")
    gpu.seq_reset()
    n = H * W
    d = [gpu.dev_alloc(pair[0].nbytes), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n), gpu.dev_alloc(8 * n * C)]
    try:
        gpu.dev_upload(d[0], pair[0])
        assert gpu.seq_push_device(d[0], True, H, W, C, levels, None, d[1], d[2], d[3]) is None
        gpu.dev_upload(d[0], pair[1])
        assert gpu.seq_push_device(d[0], True, H, W, C, levels, None, d[1], d[2], d[3]) is not None
        out = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W, C))
        for arr, p in zip(out, d[1:]):
            gpu.dev_download(arr, p)
        _same(out, want[levels], "sequence, device frames")
    finally:
        gpu.seq_reset()
        for p in d:
            gpu.dev_free(p)


@pytest.mark.parametrize("levels", LEVELS)
def test_page_locked_result_arrays(gpu, pair, want, levels):
    """page-locked (vx, vy, warpI2): the call queues their copies itself, beside and behind the final warp"""
    from papteam_opticalflow_amd import capi
    shapes = ((H, W), (H, W), (H, W, C))
    addrs = [capi._pinned_alloc(8 * int(np.prod(s))) for s in shapes]
    assert all(addrs)
    try:
        out = tuple(np.frombuffer((ctypes.c_char * (8 * int(np.prod(s)))).from_address(p), dtype=np.float64).reshape(s)
                    for s, p in zip(shapes, addrs))
        for x in out:
            x[...] = np.nan
        gpu.seq_reset()
        assert gpu.seq_push(pair[0], levels, None, out) is None
        assert gpu.seq_push(pair[1], levels, None, out) is not None
        _same(out, want[levels], "sequence into page-locked arrays")
        for x in out:
            x[...] = np.nan
        D = ctypes.POINTER(ctypes.c_double)
        a, b, t = _f64(pair[0]), _f64(pair[1]), np.zeros(10)
        rc = gpu.L.papof_flow(gpu.h, a.ctypes.data_as(D), b.ctypes.data_as(D), H, W, C, levels, None,
                              out[0].ctypes.data_as(D), out[1].ctypes.data_as(D), out[2].ctypes.data_as(D), t.ctypes.data_as(D))
        assert rc == 0
        _same(out, want[levels], "host call into page-locked arrays")
        del out, x
    finally:
        gpu.seq_reset()
        for p in addrs:
            capi._pinned_free(p)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.skipif(torch is None, reason="the tensor call takes torch tensors")
def test_batch_of_two_identical_pairs_through_the_tensor_call(pair, want, levels):
    from papteam_opticalflow_amd import tensors
    a = torch.from_numpy(np.stack([pair[0], pair[0]])).cuda()
    b = torch.from_numpy(np.stack([pair[1], pair[1]])).cuda()
    flow, warp, _ = tensors.flow_pairs(a, b, levels, layout="NHWC", out_dtype=torch.float64)
    flow, warp = flow.cpu().numpy(), warp.cpu().numpy()
    for p in range(2):
        _same((np.ascontiguousarray(flow[p, 0]), np.ascontiguousarray(flow[p, 1]), np.ascontiguousarray(warp[p])),
              want[levels], "tensor call, pair %d" % p)
