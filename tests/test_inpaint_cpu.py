"""CPU-side checks of flow-guided video completion (papteam_opticalflow_amd/tensors.py: fill_holes, complete_flows,
propagate, inpaint_video; include/papof.h: papof_fill_holes_tensor, papof_fill_workspace, papof_propagate_tensor): known
answers of the numpy fp64 restatement in tests/_inpaint_ref.py that tests/test_gpu_inpaint.py compares the device's outputs
with, a panning video with a moving occluder and its exact flows, the quality calibration of the defaults with the oracle's
flows, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI
through ctypes.  No device is touched here."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _inpaint_ref import fill_reference, level_sizes, propagate_reference  # noqa: E402
from _interp_ref import as_f64  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import fill_holes, inpaint_video, propagate  # noqa: E402


# ---- the synthetic video: the committed 1920x1080 frame panned by integer crop offsets, a flat occluder moving across it
PAN = (2, 1)              # the crop moves by (2, 1) px per frame: the background flow is (-2, -1) forward, (2, 1) backward
COLOUR = (220, 40, 200)   # the occluder's colour


def synthetic_video(T=8, H=120, W=200, box=(24, 20), box_v=(4, 1), box0=(40, 50), dilate=3, origin=(300, 800)):
    """(clean (T, H, W, 3) uint8, frames with the occluder, masks (T, H, W) bool: the occluder dilated by `dilate` px,
    flow_fw, flow_bw (T - 1, 2, H, W) float64: the background's exact flows).  The occluder is box = (w, h) px, at box0 + t
    box_v in frame t: it moves at (4, 1) px per frame against the background's (-2, -1)."""
    import cases
    I = cases.load_frame_u8("1920", 1)
    oy, ox = origin
    clean = np.stack([I[oy + t * PAN[1]:oy + t * PAN[1] + H, ox + t * PAN[0]:ox + t * PAN[0] + W] for t in range(T)])
    frames, masks = clean.copy(), np.zeros((T, H, W), bool)
    bw, bh = box
    for t in range(T):
        x0, y0 = box0[0] + t * box_v[0], box0[1] + t * box_v[1]
        frames[t, y0:y0 + bh, x0:x0 + bw] = COLOUR
        masks[t, max(y0 - dilate, 0):y0 + bh + dilate, max(x0 - dilate, 0):x0 + bw + dilate] = True
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = -PAN[0], -PAN[1]
    return clean, frames, masks, fw, -fw


def visible_set(masks, R):
    """the hole pixels of each frame that some frame within R shows, by the geometry of the pan: the chain of (x, r) reaches
    (x - j dx, r - j dy) in frame t + j (and (x + j dx, r + j dy) in frame t - j) while it stays in the image, and the frame
    shows it where its four clamped taps are all outside that frame's mask"""
    T, H, W = masks.shape
    r, x = np.mgrid[0:H, 0:W]
    vis = np.zeros((T, H, W), bool)
    for t in range(T):
        for d, steps in ((1, min(R, T - 1 - t)), (-1, min(R, t))):
            alive = np.ones((H, W), bool)
            for j in range(1, steps + 1):
                X, Y = x - d * j * PAN[0], r - d * j * PAN[1]
                alive &= (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
                Xc, Yc = np.clip(X, 0, W - 1), np.clip(Y, 0, H - 1)
                X1, Y1 = np.clip(Xc + 1, 0, W - 1), np.clip(Yc + 1, 0, H - 1)
                m = masks[t + d * j]
                clear = ~m[Yc, Xc] & ~m[Yc, X1] & ~m[Y1, Xc] & ~m[Y1, X1]
                vis[t] |= alive & clear
        vis[t] &= masks[t]
    return vis


def _psnr_masked(out, clean, masks):
    d = (out.astype(np.float64) - clean.astype(np.float64))[masks]
    return 10.0 * math.log10(255.0 ** 2 / float(np.mean(d * d)))


# ---- known answers of the fill
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("relax", [0, 3])
def test_fill_without_holes_gives_back_the_input_bytes(dtype, relax):
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (3, 9, 14, 3)).astype(dtype) if dtype == np.uint8 else rng.random((3, 9, 14, 3)).astype(dtype)
    out = fill_reference(x, np.zeros((3, 9, 14), np.uint8), relax, dtype)
    assert out.dtype == x.dtype and out.tobytes() == x.tobytes()


@pytest.mark.parametrize("relax", [0, 1, 6])
@pytest.mark.parametrize("shape", [(17, 23), (1, 40), (40, 1), (64, 64)])
def test_a_dyadic_constant_stays_exactly_constant(relax, shape):
    rng = np.random.default_rng(2)
    H, W = shape
    x = np.full((2, H, W, 2), 0.5)
    mask = rng.random((2, H, W)) < 0.6
    mask[:, 0, 0] = False  # some pixel is known
    out = fill_reference(x, mask, relax)
    assert (out == 0.5).all()


def test_a_single_pixel_hole_by_hand():
    """3 x 3, the centre a hole.  Level 1 (2 x 2): (0 + 1 + 3) / 3, (2 + 5) / 2, (6 + 7) / 2, 8.  The centre (1, 1) samples
    level 1 at (0.25, 0.25): 0.5625 * 4/3 + 0.1875 * 6.5 + 0.1875 * 3.5 + 0.0625 * 8 = 3.125; one sweep gives the mean of
    its four neighbours, (1 + 7) + (3 + 5) = 16 / 4"""
    x = np.arange(9, dtype=np.float64).reshape(1, 3, 3, 1)
    m = np.zeros((1, 3, 3), bool)
    m[0, 1, 1] = True
    out = fill_reference(x, m, 0)
    want = x.copy()
    want[0, 1, 1, 0] = ((0.0 + (4.0 / 3.0) * 0.5625) + 6.5 * 0.1875) + 3.5 * 0.1875 + 8.0 * 0.0625
    assert out[0, 1, 1, 0] == 3.125 and (out == want).all()
    assert fill_reference(x, m, 1)[0, 1, 1, 0] == 4.0
    assert fill_reference(x, m, 7)[0, 1, 1, 0] == 4.0  # (its neighbours are known: every sweep gives the same)


def test_one_by_one_frames():
    x = np.array([0.25, 0.75]).reshape(2, 1, 1, 1)
    out = fill_reference(x, np.array([0, 1]).reshape(2, 1, 1), 5)
    assert out.ravel().tolist() == [0.25, 0.0]


@pytest.mark.parametrize("relax", [0, 4])
def test_a_frame_with_no_known_pixel_comes_out_as_zeros(relax):
    rng = np.random.default_rng(3)
    x = rng.random((2, 7, 11, 3))
    m = np.zeros((2, 7, 11), bool)
    m[1] = True
    out = fill_reference(x, m, relax)
    assert (out[1] == 0).all() and (out[0] == x[0]).all()


def test_many_sweeps_approach_a_linear_ramp():
    """a linear ramp is harmonic: with enough Jacobi sweeps the hole converges to it.  Measured on a 10 x 14 hole of a
    16 x 24 ramp: max error 1.3e-2 after 0 sweeps, 3.4e-3 after 10, 4.1e-6 after 100, 2.2e-16 after 500"""
    H, W = 16, 24
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = (0.01 * x + 0.02 * y)[None, ..., None]
    m = np.zeros((1, H, W), bool)
    m[0, 3:13, 5:19] = True
    err = [np.abs(fill_reference(ramp, m, s) - ramp).max() for s in (0, 100, 500)]
    assert err[0] > 1e-3 and err[1] < 1e-5 and err[2] < 1e-12, err


def test_level_sizes():
    assert level_sizes(1, 1) == [(1, 1)]
    assert level_sizes(5, 3) == [(5, 3), (3, 2), (2, 1), (1, 1)]
    assert len(level_sizes(1080, 1920)) == 12


# ---- the propagation on the synthetic video with its exact flows
@pytest.mark.parametrize("R", [2, 4, 7])
def test_propagation_writes_the_clean_background_on_the_visible_set(R):
    clean, frames, masks, fw, bw = synthetic_video()
    for cons in ((0.01, 0.5), None):
        out, st = propagate_reference(frames, masks, fw, bw, R, cons, np.uint8)
        vis = visible_set(masks, R)
        assert ((st == 1) == vis).all()
        assert ((st == 0) == ~masks).all() and ((st == 2) == (masks & ~vis)).all()
        assert (out[vis] == clean[vis]).all()  # the background's bytes, wherever it was filled
        assert (out[~vis] == frames[~vis]).all()  # the input elsewhere (the occluder's colour in what is still a hole)
    assert vis.sum() > 0.2 * masks.sum()
    assert (masks & ~vis).any() == (R < 7)  # (at R = T - 1 every hole pixel is shown by some frame)


def test_chains_stop_at_a_failed_check_the_image_edge_and_the_ends():
    """a static scene (zero flows), T = 4, one hole pixel p = (x 3, r 2) in frames 1 and 2"""
    rng = np.random.default_rng(4)
    T, H, W = 4, 5, 6
    F = rng.random((T, H, W, 1))
    M = np.zeros((T, H, W), bool)
    M[1:3, 2, 3] = True
    fw = np.zeros((T - 1, 2, H, W))
    bw = np.zeros((T - 1, 2, H, W))

    def run(R, cons=(0.01, 0.5), f=fw, b=bw):
        out, st = propagate_reference(F, M, f, b, R, cons)
        return out[:, 2, 3, 0], st[:, 2, 3]

    # frame 1: backward frame 0 at distance 1; forward frame 2 is a hole there, frame 3 at distance 2 (R >= 2)
    out, st = run(1)
    assert st.tolist() == [0, 1, 1, 0]
    assert out[1] == F[0, 2, 3, 0] and out[2] == F[3, 2, 3, 0]
    out, _ = run(3)
    assert out[1] == (1.0 * F[0, 2, 3, 0] + 0.5 * F[3, 2, 3, 0]) / (1.0 + 0.5)
    assert out[2] == (1.0 * F[3, 2, 3, 0] + 0.5 * F[0, 2, 3, 0]) / (1.0 + 0.5)
    # a failed check: flow_bw[2] does not undo flow_fw[2] = 0 at p, so frame 2's forward chain dies (and frame 1's, at its
    # second hop); without the check it goes on
    b2 = bw.copy()
    b2[2, 0, 2, 3] = 2.0
    out, st = run(3, b=b2)
    assert out[2] == F[0, 2, 3, 0] and out[1] == F[0, 2, 3, 0] and st.tolist() == [0, 1, 1, 0]
    out, _ = run(3, cons=None, b=b2)
    assert out[2] == (1.0 * F[3, 2, 3, 0] + 0.5 * F[0, 2, 3, 0]) / (1.0 + 0.5)
    # the image edge: flow_bw[0] at p leaves the image, so frame 1's backward chain dies; with frame 3 beyond R = 1 nothing
    # is left: status 2, the input value
    b0 = bw.copy()
    b0[0, 0, 2, 3] = -4.0
    out, st = run(1, cons=None, b=b0)
    assert st.tolist() == [0, 2, 1, 0] and out[1] == F[1, 2, 3, 0]
    # the ends of the video: a hole in frame 0 has only forward chains, in frame T - 1 only backward ones
    M2 = np.zeros((T, H, W), bool)
    M2[0, 2, 3] = M2[T - 1, 2, 3] = True
    out, st = propagate_reference(F, M2, fw, bw, T - 1)
    assert st[:, 2, 3].tolist() == [1, 0, 0, 1]
    assert out[0, 2, 3, 0] == F[1, 2, 3, 0] and out[T - 1, 2, 3, 0] == F[T - 2, 2, 3, 0]


def test_the_stopping_point_needs_all_four_taps_clear():
    """zero flows but a fractional one at p: (0.5, 0) lands between two pixels, the right one a hole of frame 1"""
    T, H, W = 2, 3, 5
    F = np.arange(T * H * W, dtype=np.float64).reshape(T, H, W, 1)
    M = np.zeros((T, H, W), bool)
    M[0, 1, 1] = True
    fw = np.zeros((1, 2, H, W))
    fw[0, 0, 1, 1] = 0.5
    _, st = propagate_reference(F, M, fw, -fw, 1, None)
    assert st[0, 1, 1] == 1
    M[1, 1, 2] = True
    _, st = propagate_reference(F, M, fw, -fw, 1, None)
    assert st[0, 1, 1] == 2


# ---- quality calibration of the defaults with the oracle's flows
RELAX = 0
PIPELINE_MARGIN = 8.0  # dB over spatial fill alone: the measured 11.15 dB (below) with a margin


def oracle_flows(frames, levels=4):
    from _libs import OracleLib, build_oracle
    build_oracle()
    L = OracleLib()
    f = as_f64(frames)
    fw = np.stack([np.stack(L.coarse2fine_flow(f[i], f[i + 1], levels)[:2]) for i in range(len(f) - 1)])
    bw = np.stack([np.stack(L.coarse2fine_flow(f[i + 1], f[i], levels)[:2]) for i in range(len(f) - 1)])
    return fw, bw


def pipeline_reference(frames, masks, fw, bw, relax, consistency, R=None, out_dtype=np.uint8):
    """inpaint_video's composition in numpy: complete_flows, propagate (into float64), fill_holes of what is still a hole"""
    T = len(frames)
    cfw = np.moveaxis(fill_reference(np.moveaxis(fw, 1, -1), masks[:-1], relax), -1, 1)
    cbw = np.moveaxis(fill_reference(np.moveaxis(bw, 1, -1), masks[1:], relax), -1, 1)
    p, st = propagate_reference(frames, masks, cfw, cbw, T - 1 if R is None else R, consistency)
    return fill_reference(p, st == 2, relax, out_dtype), st


def test_quality_calibration():
    """The synthetic video (8 frames of 200x120, a 24x20 occluder moving at (4, 1) px per frame over a background panning at
    (-2, -1), masks dilated by 3 px), the oracle's flows of every pair both ways (4 levels, computed on the frames with the
    occluder), R = T - 1.  PSNR over the masked pixels against the clean video, measured here:
        relax  spatial fill alone   pipeline, check (0.01, 0.5)   pipeline, no check
          0        17.886 dB          21.436 dB (34.0 % temporal)   29.040 dB (99.9 % temporal)
          2        18.213             21.625 (33.8 %)               26.577 (99.9 %)
          8        18.305             22.211 (34.7 %)               25.400 (99.8 %)
         32        18.336             22.546 (35.6 %)               25.137 (99.9 %)
    Inside completed flows the check only shortens the chains: two thirds of the hole pixels lose every candidate.  Sweeps
    help the spatial fill a little and the completed flows' chains not at all.  The defaults are relax = 0 and no check
    (consistency=None); the pipeline must beat spatial fill alone by PIPELINE_MARGIN."""
    assert tensors.RELAX == RELAX
    for f in (fill_holes, inpaint_video):
        assert f.__kwdefaults__["relax"] == RELAX
    for f in (propagate, inpaint_video):
        assert f.__kwdefaults__["consistency"] is None
    clean, frames, masks, _, _ = synthetic_video()
    fw, bw = oracle_flows(frames)
    spatial = fill_reference(frames, masks, RELAX, np.uint8)
    full, st = pipeline_reference(frames, masks, fw, bw, RELAX, None)
    checked, _ = pipeline_reference(frames, masks, fw, bw, RELAX, (0.01, 0.5))
    ps, pf, pc = (_psnr_masked(o, clean, masks) for o in (spatial, full, checked))
    assert pf > ps + PIPELINE_MARGIN, (ps, pf)
    assert pf > pc, (pf, pc)
    assert (st == 1).sum() > 0.95 * masks.sum()
    assert (full[~masks] == frames[~masks]).all()


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
_M = lambda: _z(3, 8, 8, dtype=torch.bool)  # noqa: E731
_F = lambda: _z(2, 2, 8, 8)  # noqa: E731


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.fill_holes(_V(), _M()), ValueError),                                         # CPU tensors
    (lambda: tensors.fill_holes(None, _M()), TypeError),
    (lambda: tensors.propagate(_V(), _M(), _F(), _F()), ValueError),
    (lambda: tensors.complete_flows(_F(), _F(), _M()), ValueError),
    (lambda: tensors.inpaint_video(_V(), _M(), 2), ValueError),
    (lambda: tensors.inpaint_video(None, _M(), 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(relax=-1), ValueError), (dict(relax=65537), ValueError), (dict(relax=2.0), ValueError),      # relax
    (dict(relax=True), ValueError), (dict(relax="1"), ValueError),
    (dict(layout="CHWN"), ValueError), (dict(out_dtype=torch.float16), TypeError),
    (dict(x=_z(3, 5, 8, 8)), ValueError), (dict(x=_z(3, 8, 8, 5), layout="NHWC"), ValueError),          # channels
    (dict(x=_z(3, 0, 8, 8)), ValueError), (dict(x=_z(3, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(mask=None), TypeError), (dict(mask=_z(3, 8, 8)), TypeError),                                  # masks
    (dict(mask=_z(3, 8, 8, dtype=torch.int32)), TypeError), (dict(mask=_z(2, 8, 8, dtype=torch.bool)), ValueError),
    (dict(mask=_z(3, 8, 9, dtype=torch.uint8)), ValueError), (dict(mask=_z(8, 8, dtype=torch.bool)), ValueError),
    (dict(mask=_z(3, 8, 8, dtype=torch.bool, device="meta")), ValueError),
])
def test_fill_holes_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(x=_V(), mask=_M())
    args.update(kw)
    with pytest.raises(exc):
        tensors.fill_holes(args.pop("x"), args.pop("mask"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(radius=0), ValueError), (dict(radius=3), ValueError), (dict(radius=1.0), ValueError),        # radius 1 .. T - 1
    (dict(radius=True), ValueError),
    (dict(consistency=(0.01, -1.0)), ValueError), (dict(consistency="yes"), TypeError),
    (dict(out_dtype=torch.int32), TypeError), (dict(layout="HWC"), ValueError),
    (dict(frames=_z(1, 3, 8, 8)), ValueError), (dict(frames=_z(3, 5, 8, 8)), ValueError),              # frames
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(masks=_z(2, 8, 8, dtype=torch.bool)), ValueError),     # masks
    (dict(masks=[[0]]), TypeError),
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_bw=None), TypeError),    # flows
    (dict(flow_fw=_z(3, 2, 8, 8), flow_bw=_z(3, 2, 8, 8)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 9), flow_bw=_z(2, 2, 8, 9)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 8, device="meta"), flow_bw=_z(2, 2, 8, 8, device="meta")), ValueError),
])
def test_propagate_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), masks=_M(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        tensors.propagate(args.pop("frames"), args.pop("masks"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(relax=-1), ValueError), (dict(masks=_z(4, 8, 8, dtype=torch.bool)), ValueError),
    (dict(masks=_z(3, 8, 8, dtype=torch.float64)), TypeError), (dict(flow_fw=_z(2, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(2, 2, 8, 8, dtype=torch.int64)), TypeError),
])
def test_complete_flows_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(flow_fw=_F(), flow_bw=_F(), masks=_M())
    args.update(kw)
    with pytest.raises(exc):
        tensors.complete_flows(args.pop("flow_fw"), args.pop("flow_bw"), args.pop("masks"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", [
    (dict(relax=-1), ValueError), (dict(radius=3), ValueError), (dict(consistency=(1, 2, 3)), TypeError),
    (dict(out_dtype=torch.int16), TypeError), (dict(bogus=1), TypeError), (dict(levels=0), ValueError),
    (dict(masks=_z(3, 8, 8)), TypeError), (dict(frames=_z(3, 5, 8, 8)), ValueError),
    (dict(flows=_F()), TypeError), (dict(flows=(_F(),)), TypeError), (dict(flows=(_F(), _z(2, 2, 8, 7))), ValueError),
    (dict(flows=(_F(), _z(2, 2, 8, 8, dtype=torch.uint8))), TypeError),
])
def test_inpaint_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    frames, masks, levels = kw.pop("frames", _V()), kw.pop("masks", _M()), kw.pop("levels", 2)
    with pytest.raises(exc):
        tensors.inpaint_video(frames, masks, levels, **kw)
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
_WS = ctypes.create_string_buffer(1 << 16)
_OK = "ok"
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731


def test_fill_workspace_bytes():
    lib = _lib()
    for n, H, W, C in [(1, 1, 1, 1), (3, 8, 8, 3), (2, 5, 3, 2), (16, 1080, 1920, 3), (7, 1, 33, 4)]:
        want = sum(16 * C * n * h * w + 8 * -(-(n * h * w) // 8) for h, w in level_sizes(H, W))
        assert lib.papof_fill_workspace(n, H, W, C) == want
    for bad in [(0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 0), (1, 8, 8, 5), (-1, 8, 8, 1)]:
        assert lib.papof_fill_workspace(*bad) == -1


def _fill_call(lib, h, n=3, size=(8, 8, 3), x=_OK, mask=_OK, relax=2, out=_OK, ws=_OK, nbytes=None):
    make = {"x": lambda: _t(capi.DTYPE_U8), "mask": lambda: _t(capi.DTYPE_U8, (64, 8, 1, 0)),
            "out": lambda: _t(capi.DTYPE_F32)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(x=x, mask=mask, out=out).items()}
    need = lib.papof_fill_workspace(n, size[0], size[1], size[2])
    w = ctypes.cast(_WS, ctypes.c_void_p) if isinstance(ws, str) else ws
    return lib.papof_fill_holes_tensor(h, n, size[0], size[1], size[2], _ref(d["x"]), _ref(d["mask"]), relax, _ref(d["out"]),
                                       w, need if nbytes is None else nbytes, None)


@pytest.mark.parametrize("kw", [
    dict(x=None), dict(mask=None), dict(out=None),                                                    # NULL descriptors
    dict(x=_t(data=0)), dict(mask=_t(capi.DTYPE_U8, data=0)), dict(out=_t(data=0)),                  # NULL data
    dict(x=_t(dtype=3)), dict(out=_t(dtype=7)), dict(mask=_t(capi.DTYPE_F32)), dict(mask=_t()),       # dtypes
    dict(x=_t(strides=(-192, 24, 3, 1))), dict(mask=_t(capi.DTYPE_U8, (64, 8, -1, 0))),              # negative strides
    dict(out=_t(strides=(192, 24, -3, 1))),
    dict(out=_t(strides=(0, 24, 3, 1))), dict(out=_t(strides=(192, 24, 3, 0))),                     # zero strides of out
    dict(n=0), dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(8, 8, 0)), dict(size=(8, 8, 5)),  # sizes
    dict(relax=-1), dict(relax=65537),                                                                # relax
    dict(ws=None), dict(ws=ctypes.c_void_p(ctypes.cast(_WS, ctypes.c_void_p).value + 4)),           # workspace
    dict(nbytes=100),
])
def test_c_abi_fill_refuses(kw):
    assert _fill_call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def _prop_call(lib, h, n=3, size=(8, 8, 3), fr=_OK, mk=_OK, fw=_OK, bw=_OK, out=_OK, st=_OK, radius=2, check=1, a1=0.01,
               a2=0.5):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "mk": lambda: _t(capi.DTYPE_U8, (64, 8, 1, 0)),
            "fw": lambda: _t(strides=(128, 8, 1, 64)), "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)),
            "out": lambda: _t(capi.DTYPE_F32), "st": lambda: _t(capi.DTYPE_U8, (64, 8, 1, 0))}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, mk=mk, fw=fw, bw=bw, out=out, st=st).items()}
    return lib.papof_propagate_tensor(h, n, size[0], size[1], size[2], _ref(d["fr"]), _ref(d["mk"]), _ref(d["fw"]),
                                      _ref(d["bw"]), radius, check, a1, a2, _ref(d["out"]), _ref(d["st"]), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(mk=None), dict(fw=None), dict(bw=None), dict(out=None), dict(st=None),         # NULL descriptors
    dict(fr=_t(data=0)), dict(mk=_t(capi.DTYPE_U8, data=0)), dict(fw=_t(data=0)), dict(out=_t(data=0)),
    dict(st=_t(capi.DTYPE_U8, data=0)),
    dict(fr=_t(dtype=3)), dict(out=_t(dtype=7)), dict(mk=_t(capi.DTYPE_F64)), dict(st=_t(capi.DTYPE_F32)),  # dtypes
    dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),
    dict(fr=_t(strides=(192, -24, 3, 1))), dict(mk=_t(capi.DTYPE_U8, (-64, 8, 1, 0))),               # negative strides
    dict(fw=_t(strides=(128, 8, -1, 64))), dict(out=_t(strides=(192, 24, 3, -1))),
    dict(out=_t(strides=(192, 0, 3, 1))), dict(st=_t(capi.DTYPE_U8, (64, 8, 0, 0))),                # zero strides
    dict(st=_t(capi.DTYPE_U8, (0, 8, 1, 0))),
    dict(n=1), dict(n=0), dict(size=(0, 8, 3)), dict(size=(8, -1, 3)), dict(size=(8, 8, 0)), dict(size=(8, 8, 5)),
    dict(radius=0), dict(radius=3), dict(radius=-1),                                                   # radius 1 .. T - 1
    dict(a1=-0.01), dict(a2=math.inf), dict(a1=math.nan, check=0),                                     # alphas
])
def test_c_abi_propagate_refuses(kw):
    assert _prop_call(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_without_a_handle():
    lib = _lib()
    assert _fill_call(lib, None) == -1
    assert _prop_call(lib, None) == -1


def test_version():
    assert _lib().papof_version() == 115
