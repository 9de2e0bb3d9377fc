"""CPU-side checks of blind video temporal consistency (papteam_opticalflow_amd/tensors.py: temporal_consistency,
consistent_video; include/papof.h: papof_temporal_consistency_tensor, papof_consistency_workspace): known answers of the
numpy fp64 restatement in tests/_consistency_ref.py that tests/test_gpu_consistency.py compares the device's output with,
the quality calibration of the defaults on the committed frames with the oracle's flows, every Python argument error raised
before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _consistency_ref import consistency_reference, frame_terms, jacobi, start_value  # noqa: E402
from _inpaint_ref import level_sizes  # noqa: E402
from _interp_ref import as_f64, convert  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import consistent_video, temporal_consistency  # noqa: E402

CHECK = (0.01, 0.5)


def _zero_flows(T, H, W):
    return np.zeros((T - 1, 2, H, W)), np.zeros((T - 1, 2, H, W))


def _random(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.random(shape).astype(dtype)


# ---- known answers
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_lambda_zero_gives_the_processed_bytes(dtype):
    T, H, W = 4, 9, 13
    I = _random((T, H, W, 3), np.uint8, 1)
    P = _random((T, H, W, 2), dtype, 2)
    fw = np.random.default_rng(3).normal(0, 1.5, (T - 1, 2, H, W))
    for sigma, iters in ((0.0, 0), (0.1, 7)):
        out = consistency_reference(I, P, fw, -fw, 0.0, sigma, iters, CHECK)
        assert out.dtype == P.dtype and out.tobytes() == P.tobytes()
    # in another dtype: P converted, as store(P + 0.0)
    for odt in (np.uint8, np.float32, np.float64):
        assert (consistency_reference(I, P, fw, -fw, 0.0, 0.1, 5, None, out_dtype=odt) == convert(as_f64(P), odt)).all()


def test_lambda_zero_turns_a_negative_zero_positive():
    P = np.full((2, 3, 4, 1), -0.0)
    out = consistency_reference(np.zeros((2, 3, 4, 1)), P, *_zero_flows(2, 3, 4), 0.0, 0.0, 3, None)
    assert (out == 0).all() and not np.signbit(out[1:]).any()  # P + 0.0 from frame 1 on
    assert np.signbit(out[0]).all()  # frame 0 is stored from P_0 as it is


def test_a_global_offset_flicker_under_zero_flow_gives_back_frame_0():
    """a static scene, P_t = I + o_t: r = O_{t-1} - P_t is constant, and a constant is the solve's exact answer"""
    T, H, W = 5, 17, 23
    I = _random((1, H, W, 3), np.float64, 4).repeat(T, 0)
    o = np.random.default_rng(5).uniform(-0.1, 0.1, (T, 1, 1, 3))
    P = I + o
    fw, bw = _zero_flows(T, H, W)
    for sigma in (0.0, 0.05):
        out = consistency_reference(I, P, fw, bw, 4.0, sigma, 50, CHECK)
        assert np.abs(out - P[0]).max() < 1e-12
        assert np.abs(P - P[0]).max() > 0.05


def test_identical_processed_frames_under_zero_flow_come_back_unchanged():
    T, H, W = 4, 11, 19
    I = _random((T, H, W, 1), np.uint8, 6)
    P = _random((1, H, W, 3), np.float64, 7).repeat(T, 0)
    fw, bw = _zero_flows(T, H, W)
    for lam, sigma, iters, cons in ((4.0, 0.05, 20, CHECK), (1.0, 0.0, 0, None)):
        assert consistency_reference(I, P, fw, bw, lam, sigma, iters, cons).tobytes() == P.tobytes()
    P8 = (P * 255).astype(np.uint8)
    assert consistency_reference(I, P8, fw, bw, 4.0, 0.05, 20, CHECK).tobytes() == P8.tobytes()


def test_first_replaces_frame_0():
    T, H, W = 4, 10, 14
    I = _random((T, H, W, 3), np.uint8, 8)
    P = _random((T, H, W, 3), np.uint8, 9)
    fw, bw = _zero_flows(T, H, W)
    first = _random((H, W, 3), np.float64, 10)
    a = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CHECK)
    b = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CHECK, first=first)
    assert (b[0] == convert(first, np.uint8)).all() and (a[0] == P[0]).all()
    assert (a[1:] != b[1:]).any()
    c = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CHECK, first=P[0])  # first = P_0: no change
    assert c.tobytes() == a.tobytes()


@pytest.mark.parametrize("odt", [np.uint8, np.float32, np.float64])
def test_chunks_overlapping_by_one_frame_equal_one_call(odt):
    T, H, W = 8, 12, 21
    I = _random((T, H, W, 3), np.uint8, 11)
    P = _random((T, H, W, 3), np.float32, 12)
    fw = np.random.default_rng(13).normal(0, 1.0, (T - 1, 2, H, W))
    bw = -fw + np.random.default_rng(14).normal(0, 0.1, fw.shape)
    whole = consistency_reference(I, P, fw, bw, 4.0, 0.05, 20, CHECK, out_dtype=odt)
    parts, first = [], None
    for a, b in ((0, 3), (2, 6), (5, 8)):
        o = consistency_reference(I[a:b], P[a:b], fw[a:b - 1], bw[a:b - 1], 4.0, 0.05, 20, CHECK, first=first,
                                  out_dtype=odt)
        parts.append(o if a == 0 else o[1:])
        first = o[-1]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


def test_the_pull_push_start_by_hand():
    """2 x 2, one confident pixel (a = 1, r = 1): level 1 (1 x 1) is 1 with confidence 1, and the push gives every pixel
    a v + (1 - a) 1 = 1.  Half confidence (a = 0.5, r = 2): level 1 is (0.5 * 2) / 0.5 = 2 with confidence 0.5; the pixel
    keeps 0.5 * 2 + 0.5 * 2 = 2, the others take 2."""
    r = np.zeros((2, 2, 1))
    a = np.zeros((2, 2))
    r[1, 0, 0], a[1, 0] = 1.0, 1.0
    assert (start_value(r, a) == 1.0).all()
    r[1, 0, 0], a[1, 0] = 2.0, 0.5
    assert (start_value(r, a) == 2.0).all()
    assert (start_value(np.zeros((5, 7, 2)), np.zeros((5, 7))) == 0).all()
    one = np.array([[[0.75]]])
    assert start_value(one, np.array([[0.3]]))[0, 0, 0] == 0.75  # 1 x 1: r itself


def test_jacobi_converges_to_the_screened_poisson_solution():
    """(L + diag w) delta = w r solved densely on a 6 x 9 frame with a hole in the weights"""
    H, W = 6, 9
    rng = np.random.default_rng(15)
    w = rng.uniform(0.5, 4.0, (H, W))
    w[2:4, 3:7] = 0.0
    r = rng.normal(0, 1, (H, W, 1))
    n = H * W
    A = np.diag(w.ravel())
    for i in range(H):
        for j in range(W):
            p = i * W + j
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= i + di < H and 0 <= j + dj < W:
                    A[p, p] += 1.0
                    A[p, (i + di) * W + j + dj] -= 1.0
    exact = np.linalg.solve(A, (w[..., None] * r).reshape(n)).reshape(H, W, 1)
    a = w / 4.0
    d0 = start_value(r, a)
    e0 = np.abs(d0 - exact).max()
    e = np.abs(jacobi(d0, w, r, 400) - exact).max()
    assert e < 1e-8 < e0, (e0, e)


def test_the_weight_follows_the_frames_and_the_check():
    """zero flows: w = lambda / (1 + D / sigma^2) with D the mean squared frame difference; sigma 0: lambda; a flow that
    leaves the image or fails the check: 0"""
    H, W = 3, 4
    It = np.full((H, W, 2), 0.5)
    Ip = np.full((H, W, 2), 0.3)
    O = np.zeros((H, W, 1))
    P = np.ones((H, W, 1))
    f = np.zeros((2, H, W))
    w, a, r = frame_terms(It, Ip, O, P, f, f, 4.0, 0.1, CHECK)
    D = ((0.5 - 0.3) * (0.5 - 0.3) + (0.5 - 0.3) * (0.5 - 0.3)) / 2
    assert (w == 4.0 / (1.0 + D / (0.1 * 0.1))).all() and (a == w / 4.0).all() and (r == -1.0).all()
    w, a, _ = frame_terms(It, Ip, O, P, f, f, 4.0, 0.0, CHECK)
    assert (w == 4.0).all() and (a == 1.0).all()
    b = f.copy()
    b[0, 1, 3] = 1.0  # leaves the image
    b[0, 1, 1] = 2.0  # lands inside, but flow_fw there does not bring it back
    w, a, r = frame_terms(It, Ip, O, P, f, b, 4.0, 0.0, CHECK)
    assert w[1, 3] == 0 and w[1, 1] == 0 and r[1, 3, 0] == 0 and r[1, 1, 0] == 0 and (w[0] == 4.0).all()
    w, _, _ = frame_terms(It, Ip, O, P, f, b, 4.0, 0.0, None)
    assert w[1, 1] == 4.0 and w[1, 3] == 0


# ---- quality calibration of the defaults with the oracle's flows
PSNR_MIN = 37.0          # dB against the flicker-free target: measured 39.10 with the defaults (processed: 19.98)
WARP_RATIO_MAX = 0.01    # warping error of O over P's: measured 1.38e-5 / 1.44e-2
NO_FLICKER_MIN = 52.0    # dB of O against P = I: measured 55.69


def _panned(T=8, H=120, W=200, origin=(300, 800)):
    import cases
    img = cases.load_frame_u8("1920", 1)
    oy, ox = origin
    return np.stack([img[oy + t:oy + t + H, ox + 2 * t:ox + 2 * t + W] for t in range(T)])


def _psnr(a, b):
    return 10.0 * math.log10(1.0 / float(np.mean((a - b) ** 2)))


def warping_error(I, O, fw, bw, consistency=CHECK):
    """the mean over t of the mean of (O_t - O_{t-1} warped along flow_bw[t - 1])^2 over the valid pixels of the hop"""
    If, Of = as_f64(I), as_f64(O)
    e = []
    for t in range(1, len(O)):
        w, _, r = frame_terms(If[t], If[t - 1], Of[t - 1], Of[t], fw[t - 1], bw[t - 1], 1.0, 0.0, consistency)
        e.append(float(np.mean(r[w > 0] ** 2)))
    return float(np.mean(e))


def test_quality_calibration():
    """8 frames of 200x120 panned by (2, 1) px per frame across the committed 1080p frame, the oracle's flows of every
    pair both ways (4 levels).  Processed: P_t = g_t I_t + o_t, per-frame, per-channel gains in [0.8, 1.2] and offsets in
    [-0.1, 0.1] (seed 7); the target is g_0 I_t + o_0.  Measured here (PSNR against the target; warping error, the mean
    squared O_t - warped O_{t-1} over the valid pixels; PSNR of O against P with P = I, no flicker):
        processed as is                      19.98 dB   1.44e-2
        lam 0.1,  sigma 0.1,  iters 50       33.43 dB   3.00e-4    69.16 dB
        lam 0.5,  sigma 0.1,  iters 10       35.82 dB   1.11e-4    61.67 dB
        lam 0.5,  sigma 0.1,  iters 50       35.58 dB   1.21e-4    63.67 dB
        lam 1,    sigma 0,    iters 20       36.71 dB   6.64e-5    59.62 dB
        lam 1,    sigma 0.05, iters 20       36.73 dB   6.68e-5    61.56 dB
        lam 2,    sigma 0.1,  iters 50       37.95 dB   3.21e-5    57.55 dB
        lam 4,    sigma 0,    iters 20       39.03 dB   1.36e-5    54.33 dB
        lam 4,    sigma 0.05, iters 5        39.00 dB   1.35e-5    54.74 dB  (sigma 0.1)
        lam 4,    sigma 0.05, iters 20       39.10 dB   1.38e-5    55.69 dB  <- the defaults
        lam 4,    sigma 0.2,  iters 20       39.04 dB   1.36e-5    54.46 dB
        lam 8,    sigma 0.05, iters 20       39.99 dB   5.29e-6    53.11 dB
    A larger lambda follows the warped past more closely and removes more flicker, and blurs more where nothing flickers
    (the bilinear warp's blur accumulates).  sigma 0.05 keeps the most detail without flicker; past 20 sweeps nothing
    changes at lambda >= 0.5.  The defaults are lambda 4, sigma 0.05, 20 sweeps, the check on."""
    assert (tensors.LAM, tensors.SIGMA, tensors.ITERS) == (4.0, 0.05, 20)
    for f in (temporal_consistency, consistent_video):
        kw = f.__kwdefaults__
        assert (kw["lam"], kw["sigma"], kw["iters"], kw["consistency"]) == (4.0, 0.05, 20, tensors.CONSISTENCY)
    from test_inpaint_cpu import oracle_flows
    I = _panned()
    T = len(I)
    fw, bw = oracle_flows(I)
    rng = np.random.default_rng(7)
    g, o = rng.uniform(0.8, 1.2, (T, 1, 1, 3)), rng.uniform(-0.1, 0.1, (T, 1, 1, 3))
    If = as_f64(I)
    P, target = g * If + o, g[0] * If + o[0]
    O = consistency_reference(I, P, fw, bw, tensors.LAM, tensors.SIGMA, tensors.ITERS, tensors.CONSISTENCY)
    p_O, p_P = _psnr(O, target), _psnr(P, target)
    e_O, e_P = warping_error(I, O, fw, bw), warping_error(I, P, fw, bw)
    assert p_P < 21.0 and p_O > PSNR_MIN, (p_P, p_O)
    assert e_O < WARP_RATIO_MAX * e_P, (e_O, e_P)
    clean = consistency_reference(I, If, fw, bw, tensors.LAM, tensors.SIGMA, tensors.ITERS, tensors.CONSISTENCY)
    assert _psnr(clean, If) > NO_FLICKER_MIN
    assert (O[0] == P[0]).all()


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_V = lambda: _z(3, 3, 8, 8)  # noqa: E731
_F = lambda: _z(2, 2, 8, 8)  # noqa: E731


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: temporal_consistency(_V(), _V(), _F(), _F()), ValueError),                   # CPU tensors
    (lambda: temporal_consistency(None, _V(), _F(), _F()), TypeError),
    (lambda: consistent_video(_V(), _V(), 2), ValueError),
    (lambda: consistent_video(None, _V(), 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_BAD = [
    (dict(lam=-1.0), ValueError), (dict(lam=math.inf), ValueError), (dict(lam=math.nan), ValueError),     # lam, sigma
    (dict(lam="1"), TypeError), (dict(lam=True), TypeError), (dict(lam=None), TypeError),
    (dict(sigma=-0.1), ValueError), (dict(sigma=math.inf), ValueError), (dict(sigma=None), TypeError),
    (dict(iters=-1), ValueError), (dict(iters=65537), ValueError), (dict(iters=2.0), ValueError),         # iters
    (dict(iters=True), ValueError),
    (dict(consistency=(0.01, -1.0)), ValueError), (dict(consistency="yes"), TypeError),                 # consistency
    (dict(layout="CHWN"), ValueError), (dict(out_dtype=torch.float16), TypeError),
    (dict(frames=_z(1, 3, 8, 8), processed=_z(1, 3, 8, 8)), ValueError),                                 # frames
    (dict(frames=_z(3, 5, 8, 8)), ValueError), (dict(frames=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(frames=_z(3, 3, 0, 8)), ValueError),
    (dict(processed=_z(3, 5, 8, 8)), ValueError), (dict(processed=_z(4, 3, 8, 8)), ValueError),          # processed
    (dict(processed=_z(3, 3, 8, 9)), ValueError), (dict(processed=_z(3, 3, 8, 8, dtype=torch.int32)), TypeError),
    (dict(processed=_z(3, 3, 8, 8, device="meta")), ValueError), (dict(processed=[[0]]), TypeError),
    (dict(processed=_z(3, 0, 8, 8)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_bw=None), TypeError),        # flows
    (dict(flow_fw=_z(3, 2, 8, 8), flow_bw=_z(3, 2, 8, 8)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 9), flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 8, device="meta"), flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),
    (dict(first=_z(2, 8, 8)), ValueError), (dict(first=_z(3, 8, 9)), ValueError),                        # first
    (dict(first=_z(2, 3, 8, 8)), ValueError), (dict(first=_z(3, 8, 8, dtype=torch.int64)), TypeError),
    (dict(first=_z(3, 8, 8, device="meta")), ValueError), (dict(first=np.zeros((3, 8, 8))), TypeError),
    (dict(first=_z(8, 8, 3)), ValueError),
]


@pytest.mark.parametrize("kw,exc", _BAD)
def test_temporal_consistency_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), processed=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        temporal_consistency(args.pop("frames"), args.pop("processed"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [(k, e) for k, e in _BAD if "flow_fw" not in k and "flow_bw" not in k] + [
    (dict(levels=0), ValueError), (dict(bogus=1), TypeError),
    (dict(flows=_F()), TypeError), (dict(flows=(_F(),)), TypeError), (dict(flows=(_F(), _z(2, 2, 8, 7))), ValueError),
    (dict(flows=(_F(), _z(2, 2, 8, 8, dtype=torch.uint8))), TypeError),
])
def test_consistent_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, processed, levels = kw.pop("frames", _V()), kw.pop("processed", _V()), kw.pop("levels", 2)
    with pytest.raises(exc):
        consistent_video(frames, processed, levels, **kw)
    assert stub == []


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_F64, strides=(192, 24, 3, 1), data=0x100000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_WS = ctypes.create_string_buffer(1 << 16)
_OK = "ok"
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
# distinct, far apart fake addresses: 3 frames of 8 x 8 x 3 float64 are 4.6 kB
_ADDR = {"fr": 0x100000, "pr": 0x200000, "fw": 0x300000, "bw": 0x400000, "first": 0x500000, "out": 0x600000}


def test_consistency_workspace_bytes():
    lib = _lib()
    for H, W, C in [(1, 1, 1), (8, 8, 3), (5, 3, 2), (1080, 1920, 3), (1, 33, 4), (135, 240, 1)]:
        s = level_sizes(H, W)
        want = 8 * ((2 + 3 * C) * H * W + sum((1 + C) * h * w for h, w in s[1:]))
        assert lib.papof_consistency_workspace(H, W, C) == want
    for bad in [(0, 8, 3), (8, 0, 3), (8, 8, 0), (8, 8, 5), (-1, 8, 1)]:
        assert lib.papof_consistency_workspace(*bad) == -1


def _tc_call(lib, h, n=3, size=(8, 8), ci=3, co=3, fr=_OK, pr=_OK, fw=_OK, bw=_OK, first=None, out=_OK, lam=4.0,
             sigma=0.05, iters=20, check=1, a1=0.01, a2=0.5, ws=_OK, nbytes=None):
    make = {"fr": lambda: _t(capi.DTYPE_U8, data=_ADDR["fr"]), "pr": lambda: _t(capi.DTYPE_F32, data=_ADDR["pr"]),
            "fw": lambda: _t(strides=(128, 8, 1, 64), data=_ADDR["fw"]),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64), data=_ADDR["bw"]),
            "first": lambda: _t(capi.DTYPE_U8, (0, 24, 3, 1), data=_ADDR["first"]),
            "out": lambda: _t(capi.DTYPE_F64, data=_ADDR["out"])}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, pr=pr, fw=fw, bw=bw, first=first,
                                                                  out=out).items()}
    need = lib.papof_consistency_workspace(size[0], size[1], co)
    w = ctypes.cast(_WS, ctypes.c_void_p) if isinstance(ws, str) else ws
    return lib.papof_temporal_consistency_tensor(h, n, size[0], size[1], ci, co, _ref(d["fr"]), _ref(d["pr"]),
                                                 _ref(d["fw"]), _ref(d["bw"]), _ref(d["first"]), lam, sigma, iters, check,
                                                 a1, a2, _ref(d["out"]), w, need if nbytes is None else nbytes, None)


_WS_ADDR = ctypes.cast(_WS, ctypes.c_void_p).value


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(pr=None), dict(fw=None), dict(bw=None), dict(out=None),                       # NULL descriptors
    dict(fr=_t(data=0)), dict(pr=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(out=_t(data=0)),
    dict(first=_t(data=0)),
    dict(fr=_t(dtype=3)), dict(pr=_t(dtype=-1)), dict(out=_t(dtype=7)), dict(first=_t(dtype=5, data=_ADDR["first"])),
    dict(fw=_t(capi.DTYPE_U8, data=_ADDR["fw"])), dict(bw=_t(dtype=7, data=_ADDR["bw"])),              # dtypes
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(pr=_t(strides=(192, 24, 3, -1), data=_ADDR["pr"])),     # negative strides
    dict(fw=_t(strides=(128, 8, -1, 64), data=_ADDR["fw"])), dict(bw=_t(strides=(-128, 8, 1, 64), data=_ADDR["bw"])),
    dict(first=_t(strides=(0, -24, 3, 1), data=_ADDR["first"])),
    dict(out=_t(strides=(192, 24, -3, 1), data=_ADDR["out"])),
    dict(out=_t(strides=(0, 24, 3, 1), data=_ADDR["out"])), dict(out=_t(strides=(192, 24, 3, 0), data=_ADDR["out"])),
    dict(out=_t(data=_ADDR["pr"] + 64)), dict(out=_t(data=_ADDR["fr"])), dict(out=_t(data=_ADDR["fw"] + 800)),  # overlap
    dict(out=_t(data=_ADDR["bw"] - 8)), dict(first=_t(capi.DTYPE_U8, (0, 24, 3, 1), data=_ADDR["out"] + 100)),
    dict(out=_t(data=_WS_ADDR + 256)), dict(fr=_t(capi.DTYPE_U8, data=_WS_ADDR)),                       # the workspace
    dict(n=1), dict(n=0), dict(size=(0, 8)), dict(size=(8, -1)),                                        # sizes
    dict(ci=0), dict(ci=5), dict(co=0), dict(co=5),                                                     # channels
    dict(lam=-1.0), dict(lam=math.inf), dict(lam=math.nan), dict(sigma=-0.5), dict(sigma=math.nan),      # lambda, sigma
    dict(iters=-1), dict(iters=65537),                                                                  # iters
    dict(a1=-0.01), dict(a2=math.inf), dict(a1=math.nan, check=0),                                      # alphas
    dict(ws=None), dict(ws=ctypes.c_void_p(_WS_ADDR + 4)), dict(nbytes=100),                            # workspace
])
def test_c_abi_refuses(kw):
    assert _tc_call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle():
    assert _tc_call(_lib(), None) == -1


def test_the_new_symbols_are_exported_and_listed():
    lib = _lib()
    for name in ("papof_temporal_consistency_tensor", "papof_consistency_workspace"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert lib.papof_version() == 115
