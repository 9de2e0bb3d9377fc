"""CPU-side checks of motion-compensated deinterlacing (papteam_opticalflow_amd/tensors.py: split_fields, bob_fields,
field_flows, deinterlace_fields, deinterlace_video; include/papof.h: papof_deinterlace_tensor): known answers of the numpy
fp64 restatement in tests/_deinterlace_ref.py that tests/test_gpu_deinterlace.py compares the device's output with, the
calibration of sigma and of the bars on panning crops of the committed 1080p frame, with exact flows and with the oracle's,
every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through
ctypes.  No device is touched here."""
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _deinterlace_ref import deinterlace_reference, fields_of, split_reference  # noqa: E402
from _interp_ref import as_f64  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (bob_fields, deinterlace_fields, deinterlace_video, field_flows,  # noqa: E402
                                             split_fields)

SIGMA = 0.05


def _flows(T, Hf, W, u=0.0, v=0.0):
    """the exact pair flows of a scene that moves by (u, v) field units from field k to field k + 2"""
    fw = np.zeros((T - 2, 2, Hf, W))
    fw[:, 0], fw[:, 1] = u, v
    return fw, -fw


def _progressive(T, H, W, C, dtype, seed=1, dy=0):
    """a progressive video (T, H, W, C) whose scene moves down by dy frame rows per frame"""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + T * abs(dy), W, C)).astype(np.uint8) if dtype == np.uint8 else \
        rng.random((H + T * abs(dy), W, C)).astype(dtype)
    return np.stack([big[(T - 1 - t) * dy:(T - 1 - t) * dy + H] if dy >= 0 else big[t * -dy:t * -dy + H] for t in range(T)])


# ---- known answers
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_a_static_video_comes_back_exactly(dtype, first):
    """zero flows land on the field lines of both neighbours: c0 = c1 = 1, D = 0, q = 1 and out = 0 s + m -- which is why
    the blend is (1 - q) s + q m and not s + q (m - s)"""
    T, H, W, C = 6, 10, 7, 3
    V = np.stack([_progressive(1, H, W, C, dtype)[0]] * T)
    video, conf = deinterlace_reference(fields_of(V, first), *_flows(T, H // 2, W), first=first, sigma=SIGMA)
    assert video.dtype == dtype and video.shape == V.shape
    assert video[1:-1].tobytes() == V[1:-1].tobytes()
    assert (conf[1:-1] == 1.0).all() and (conf[[0, -1]] == 0.5).all()


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dy", [2, -2])
def test_two_frame_rows_per_field_come_back_exactly_away_from_the_borders(dy, first):
    """the scene moves by two frame rows per field: the pair flow is v = +-2 field rows, both samples land on field lines"""
    T, H, W, C = 6, 24, 5, 2
    for dtype in (np.uint8, np.float64):
        V = _progressive(T, H, W, C, dtype, 2, dy)
        video, conf = deinterlace_reference(fields_of(V, first), *_flows(T, H // 2, W, 0.0, float(dy)), first=first, sigma=SIGMA)
        assert video[1:-1, 4:-4].tobytes() == V[1:-1, 4:-4].tobytes()
        assert (conf[1:-1, 2:-2] == 1.0).all()
        assert (conf[1:-1, 0] == 0.5).all() and (conf[1:-1, -1] == 0.5).all()  # one sample has left the image


@pytest.mark.parametrize("first", [0, 1])
def test_at_the_critical_velocity_the_output_is_the_bobs(first):
    """one frame row per field: the neighbouring fields hold the current field's lines, every sample lands halfway between
    two of them, c = 0 everywhere"""
    T, H, W, C = 5, 12, 6, 3
    V = _progressive(T, H, W, C, np.uint8, 3, 1)
    F = fields_of(V, first)
    video, conf = deinterlace_reference(F, *_flows(T, H // 2, W, 3.0, 1.0), first=first, sigma=SIGMA)
    bob, zero = deinterlace_reference(F, first=first, mode=0)
    assert video.tobytes() == bob.tobytes() and (conf == 0.0).all() and (zero == 0.0).all()


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf, 1e300, 40.0])
def test_bad_flows_and_points_out_of_the_image_give_the_bob(bad):
    T, H, W, C = 5, 12, 6, 2
    F = fields_of(_progressive(T, H, W, C, np.uint8, 4), 0)
    bob, _ = deinterlace_reference(F, mode=0)
    for comp in (0, 1):  # (40: both points leave the image, on opposite sides)
        fw, bw = _flows(T, H // 2, W)
        fw[:, comp], bw[:, comp] = bad, -bad
        video, conf = deinterlace_reference(F, fw, bw, sigma=SIGMA)
        assert video.tobytes() == bob.tobytes() and (conf == 0.0).all(), comp
    # a bad flow at one pixel of a static video: that pixel is the bob's, the others are untouched, no NaN in the output
    fw, bw = _flows(T, H // 2, W)
    fw[:, 0, 2, 3] = bad
    Ff = as_f64(F)
    video, conf = deinterlace_reference(Ff, fw, bw, sigma=SIGMA)
    assert np.isfinite(video).all() and (conf[1:-1, 2, 3] == 0.0).all() and (np.delete(conf[2].ravel(), 2 * W + 3) == 1.0).all()


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("Hf", [1, 2, 3, 7])
def test_the_cubics_weights_and_its_clamped_rows(Hf, first):
    """s = (9 (a1 + b1) - (a3 + b3)) / 16 of the own field's lines at frame distance -+1 and -+3, clamped into the field:
    derived here from the frame rows, not from the rule's table of field rows"""
    T, W = 4, 3
    rng = np.random.default_rng(5)
    F = rng.random((T, Hf, W, 1))
    video, conf = deinterlace_reference(F, first=first, mode=0)
    assert (conf == 0.0).all()
    for t in range(T):
        p = (t + first) & 1
        row = lambda R: F[t, min(max((R - p) // 2, 0), Hf - 1)]  # noqa: E731  the field row of frame row R (parity p), clamped
        for R in range(2 * Hf):
            if R % 2 == p:
                assert (video[t, R] == F[t, R // 2]).all()
            else:
                want = (9.0 * (row(R - 1) + row(R + 1)) - (row(R - 3) + row(R + 3))) * 0.0625
                assert (video[t, R] == want).all(), (t, R)
    if Hf == 1:  # all four taps are the one line: (18 v - 2 v) / 16
        assert np.allclose(video[:, 0], video[:, 1], rtol=0, atol=1e-15)
    # an impulse shows the weights themselves
    if Hf == 7:
        F = np.zeros((T, Hf, W, 1))
        F[:, 3] = 1.0
        video, _ = deinterlace_reference(F, first=0, mode=0)
        assert video[0, :, 0, 0].tolist() == [0, 0, 0, -0.0625, 0, 0.5625, 1.0, 0.5625, 0, -0.0625, 0, 0, 0, 0]


@pytest.mark.parametrize("first", [0, 1])
def test_the_end_frames_sample_the_one_field_the_rule_names(first):
    """frame 0 samples field 1 along half of flow_fw[1], frame T - 1 field T - 2 along half of flow_bw[T - 4]: every other
    field and flow may hold anything"""
    T, Hf, W, C = 6, 8, 9, 2
    rng = np.random.default_rng(6)
    F = rng.random((T, Hf, W, C))
    fw, bw = rng.normal(0, 3, (T - 2, 2, Hf, W)), rng.normal(0, 3, (T - 2, 2, Hf, W))
    fw[1, 0], fw[1, 1] = 2.0, -4.0   # half of it: (1, -2), on the field lines
    bw[T - 4, 0], bw[T - 4, 1] = -4.0, 2.0
    video, conf = deinterlace_reference(F, fw, bw, first=first, sigma=SIGMA)
    bob, _ = deinterlace_reference(F, first=first, mode=0)
    for t, src, dx, dy in ((0, 1, 1, -2), (T - 1, T - 2, -2, 1)):
        pm = 1 - ((t + first) & 1)
        for j in range(Hf):
            for x in range(W):
                inside = 0 <= j + dy <= Hf - 1 and 0 <= x + dx <= W - 1
                assert conf[t, j, x] == (0.5 if inside else 0.0)
                want = 0.5 * bob[t, 2 * j + pm, x] + 0.5 * F[src, j + dy, x + dx] if inside else bob[t, 2 * j + pm, x]
                assert (video[t, 2 * j + pm, x] == want).all(), (t, j, x)
    # nothing else is read: scrambling every other flow and the fields the end frames do not name changes neither
    fw2, bw2 = fw.copy(), bw.copy()
    fw2[[0, 2, 3]] = math.nan
    bw2[[0, 1, 3]] = math.nan
    v2, c2 = deinterlace_reference(F, fw2, bw2, first=first, sigma=SIGMA)
    assert v2[[0, T - 1]].tobytes() == video[[0, T - 1]].tobytes() and c2[[0, T - 1]].tobytes() == conf[[0, T - 1]].tobytes()
    assert (c2[1:-1] == 0.0).all()
    # frame 0 reads flow_fw only, frame T - 1 flow_bw only
    fw3, bw3 = fw.copy(), bw.copy()
    bw3[1], fw3[T - 4] = math.nan, math.nan
    v3, _ = deinterlace_reference(F, fw3, bw3, first=first, sigma=SIGMA)
    assert v3[[0, T - 1]].tobytes() == video[[0, T - 1]].tobytes()


def test_the_agreement_weight():
    """two samples that differ by d in every channel: q = 1 / (1 + d^2 / sigma^2), m their mean"""
    T, Hf, W = 4, 4, 4
    F = np.zeros((T, Hf, W, 2))
    F[0], F[1], F[2], F[3] = 0.2, 0.9, 0.2 + 0.1, 0.9
    video, conf = deinterlace_reference(F, *_flows(T, Hf, W), sigma=0.1)
    d = 0.2 - (0.2 + 0.1)
    q = 1.0 / (1.0 + ((d * d + d * d) / 2.0) / (0.1 * 0.1))
    assert (conf[1] == q).all() and 0.49 < q < 0.51
    s = (9.0 * (0.9 + 0.9) - (0.9 + 0.9)) * 0.0625
    assert (video[1, 0::2] == (1.0 - q) * s + q * ((1.0 * 0.2 + 1.0 * (0.2 + 0.1)) / (1.0 + 1.0))).all()
    assert deinterlace_reference(F, *_flows(T, Hf, W), sigma=1e-3)[1][1].max() < 1e-3


def test_split_reference_and_fields_of():
    rng = np.random.default_rng(7)
    V = rng.integers(0, 256, (3, 6, 4, 2)).astype(np.uint8)
    for top_first, first in ((True, 0), (False, 1)):
        F, f = split_reference(V, top_first)
        assert f == first and F.shape == (6, 3, 4, 2)
        for k in range(6):
            assert (F[k] == V[k // 2, (k + first) & 1::2]).all()
        got = split_fields(torch.from_numpy(V), top_first, layout="NHWC")
        assert got.dtype == torch.uint8 and (got.numpy() == F).all()
        got = split_fields(torch.from_numpy(V).permute(0, 3, 1, 2), top_first)
        assert (got.permute(0, 2, 3, 1).numpy() == F).all()
    assert split_fields(torch.from_numpy(V[0]), layout="NHWC").shape == (2, 3, 4, 2)


# ---- the calibration of sigma and of the bars
T_SCENE, H_SCENE, W_SCENE = 8, 120, 200
SCENES = [(0.0, 0.0), (3.0, 2.0), (2.5, 0.25), (1.5, 0.5), (3.0, 1.0)]  # pan (vx, vy) in frame pixels per field
CRITICAL = (3.0, 1.0)
JUDGED = (3, 4)  # the frames whose made lines are measured
CAP = 99.0  # dB: the PSNR written for identical bytes


def deint_scene(vx, vy):
    """The committed 1920x1080 frame sampled bilinearly on a 120 x 200 window whose origin is (row 300 + k vy, column 800 +
    k vx) at field k, k = 0 .. 7, rounded to uint8 -> (progressive (T, H, W, 3) uint8, fields (T, H / 2, W, 3) with first 0,
    the exact flow_fw, flow_bw in field coordinates: the scene moves by (-2 vx, -vy) field units per pair)"""
    import cases
    img = cases.load_frame_u8("1920", 1).astype(np.float64)
    T, H, W = T_SCENE, H_SCENE, W_SCENE
    out = np.empty((T, H, W, 3), np.uint8)
    for k in range(T):
        Y, X = 300.0 + k * vy + np.arange(H)[:, None], 800.0 + k * vx + np.arange(W)[None, :]
        y0, x0 = np.floor(Y).astype(int), np.floor(X).astype(int)
        fy, fx = (Y - y0)[..., None], (X - x0)[..., None]
        v = (img[y0, x0] * (1 - fx) + img[y0, x0 + 1] * fx) * (1 - fy) + (img[y0 + 1, x0] * (1 - fx) + img[y0 + 1, x0 + 1] * fx) * fy
        out[k] = np.rint(v).astype(np.uint8)
    fw, bw = _flows(T, H // 2, W, -2.0 * vx, -vy)
    return out, fields_of(out, 0), fw, bw


def made_psnr(video, truth, first=0, frames=JUDGED):
    """PSNR in dB over the made lines of `frames`, CAP for identical bytes"""
    err, n = 0.0, 0
    for t in frames:
        pm = 1 - ((t + first) & 1)
        d = as_f64(video[t, pm::2]) - as_f64(truth[t, pm::2])
        err, n = err + float((d * d).sum()), n + d.size
    return CAP if err == 0 else min(CAP, 10.0 * math.log10(n / err))


# measured on the restatement (test_quality_calibration's docstring): PSNR of the cubic bob, with exact flows, with the
# oracle's flows (4 levels, on the fields)
MEASURED = {
    (0.0, 0.0): (25.805, CAP, CAP),
    (3.0, 2.0): (25.952, 41.987, 34.323),
    (2.5, 0.25): (27.035, 29.704, 29.587),
    (1.5, 0.5): (27.589, 28.255, 28.326),
    (3.0, 1.0): (25.929, 25.929, 25.960),
}


def bar(scene):
    """the least PSNR with estimated flows: within 0.1 dB of the bob at the critical velocity, elsewhere the bob's PSNR plus
    half of the gain measured with the oracle's flows -- the slack is for the device's flows differing from the oracle's"""
    bob, _, oracle = MEASURED[scene]
    return bob - 0.1 if scene == CRITICAL else bob + 0.5 * (oracle - bob)


def oracle_field_flows(fields, levels=4):
    """field_flows with the oracle: pair k from field k to field k + 2 and back"""
    from _libs import OracleLib, build_oracle
    build_oracle()
    L = OracleLib()
    f = as_f64(fields)
    fw = np.stack([np.stack(L.coarse2fine_flow(f[i], f[i + 2], levels)[:2]) for i in range(len(f) - 2)])
    bw = np.stack([np.stack(L.coarse2fine_flow(f[i + 2], f[i], levels)[:2]) for i in range(len(f) - 2)])
    return fw, bw


@pytest.mark.parametrize("scene", SCENES)
def test_quality_calibration(scene):
    """Eight fields of 60 x 200 of the 1080p frame panning at (vx, vy) frame pixels per field; PSNR in dB over the made lines
    of frames 3 and 4 against the progressive frames, measured here on the restatement (99 stands for identical bytes):
        pan (vx, vy)    cubic bob   exact flows   oracle's flows (4 levels, on the fields)   sigma 0.03 / 0.1 (oracle's flows)
        (0, 0)            25.81       99 (exact)     99 (the field flows come out 0.000)        99 / 99
        (3, 2)            25.95       41.99          34.32                                      33.81 / 34.78
        (2.5, 0.25)       27.04       29.70          29.59                                      29.20 / 29.90
        (1.5, 0.5)        27.59       28.26          28.33                                      28.24 / 28.41
        (3, 1)            25.93       25.93          25.96                                      25.96 / 25.96
    The oracle's field flows are off by 0.06 .. 0.09 px on average; the mean q over the judged frames is 1.00, 0.97, 0.65,
    0.41 and 0.00 with exact flows.  (3, 2) with exact flows is exact inside the image: the 42 dB are the columns and rows
    whose samples leave it.  sigma = 0.1 gains 0.1 .. 0.5 dB on the three moving scenes and ties on (0, 0) and (3, 1); it
    does not win on every scene, so sigma = 0.05 stays the default.  Bars: at the critical velocity (3, 1) exactly the bob's bytes with exact flows
    and within 0.1 dB of the bob with the oracle's; elsewhere the bob's PSNR plus half of the gain measured with the
    oracle's flows."""
    assert tensors.DEINT_SIGMA == SIGMA
    for f in (tensors.deinterlace_fields, tensors.deinterlace_video):
        assert f.__kwdefaults__["sigma"] == SIGMA
    truth, F, fw, bw = deint_scene(*scene)
    bob, _ = deinterlace_reference(F, mode=0)
    exact, q = deinterlace_reference(F, fw, bw, sigma=SIGMA)
    ofw, obw = oracle_field_flows(F, 4)
    est = {s: deinterlace_reference(F, ofw, obw, sigma=s)[0] for s in (SIGMA, 0.03, 0.1)}
    got = (made_psnr(bob, truth), made_psnr(exact, truth), made_psnr(est[SIGMA], truth))
    print("pan %s: bob %.2f dB, exact flows %.2f dB, oracle's flows %.2f dB (sigma 0.03: %.2f, 0.1: %.2f); mean q %.3f; "
          "oracle flow error %.3f px" % (scene, *got, made_psnr(est[0.03], truth), made_psnr(est[0.1], truth),
                                         q[list(JUDGED)].mean(), np.abs(ofw - fw).mean()))
    assert np.allclose(got, MEASURED[scene], rtol=0, atol=0.02), (got, MEASURED[scene])
    for t in range(T_SCENE):  # the kept lines are the fields' bytes
        assert (exact[t, t & 1::2] == F[t]).all() and (est[SIGMA][t, t & 1::2] == F[t]).all()
    if scene == CRITICAL:
        assert exact.tobytes() == bob.tobytes() and (q == 0.0).all()
    elif scene == (0.0, 0.0):
        assert exact[1:-1].tobytes() == truth[1:-1].tobytes() and est[SIGMA][1:-1].tobytes() == truth[1:-1].tobytes()
        assert np.abs(ofw).max() == 0.0 and np.abs(obw).max() == 0.0
    else:
        assert got[1] > got[0] + 0.5  # exact flows gain
    assert got[2] >= bar(scene), (got, bar(scene))


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_V = lambda: _z(5, 3, 8, 8)  # noqa: E731
_F = lambda: _z(3, 2, 8, 8)  # noqa: E731


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: bob_fields(_V()), ValueError),                                                   # CPU tensors
    (lambda: bob_fields(None), TypeError),
    (lambda: field_flows(_V(), 2), ValueError),
    (lambda: field_flows(None, 2), TypeError),
    (lambda: deinterlace_fields(_V(), _F(), _F()), ValueError),
    (lambda: deinterlace_fields(None, _F(), _F()), TypeError),
    (lambda: deinterlace_video(_V(), 2), ValueError),
    (lambda: deinterlace_video(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_COMMON = [
    (dict(layout="CHWN"), ValueError),
    (dict(fields=_z(5, 5, 8, 8)), ValueError), (dict(fields=_z(5, 8, 8, 5), layout="NHWC"), ValueError),   # channels
    (dict(fields=_z(5, 0, 8, 8)), ValueError), (dict(fields=_z(5, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(fields=_z(3, 3, 8, 8)), ValueError),                                                          # fewer than 4 fields
    (dict(fields=_z(8, 8)), ValueError), (dict(fields=np.zeros((5, 3, 8, 8))), TypeError),
    (dict(fields=_z(5, 3, 8, 8, device="meta")), ValueError),
]
_PARITY = [
    (dict(first=2), ValueError), (dict(first=-1), ValueError), (dict(first=1.0), ValueError), (dict(first=True), ValueError),
    (dict(first=None), ValueError),
]
_OUT = [(dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError)]
_SIGMA = [
    (dict(sigma=0.0), ValueError), (dict(sigma=-0.1), ValueError), (dict(sigma=math.nan), ValueError),
    (dict(sigma=math.inf), ValueError), (dict(sigma="0.1"), TypeError), (dict(sigma=True), TypeError), (dict(sigma=None), TypeError),
]
_FLOWS = [
    (dict(fields=_z(4, 3, 8, 8)), ValueError),                                                          # 2 pairs, 3 given
    (dict(flow_fw=_z(3, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_bw=_z(3, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(3, 3, 8, 8), flow_bw=_z(3, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(4, 2, 8, 8), flow_bw=_z(4, 2, 8, 8)), ValueError),                               # T - 1, not T - 2 pairs
    (dict(flow_fw=_z(3, 2, 16, 8), flow_bw=_z(3, 2, 16, 8)), ValueError),                             # frame, not field rows
    (dict(flow_fw=_z(3, 2, 8, 9), flow_bw=_z(3, 2, 8, 9)), ValueError), (dict(flow_bw=_z(3, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError), (dict(flow_bw=np.zeros((3, 2, 8, 8))), TypeError),
    (dict(flow_fw=_z(3, 2, 8, 8, device="meta"), flow_bw=_z(3, 2, 8, 8, device="meta")), ValueError),  # devices
    (dict(flow_bw=_z(3, 2, 8, 8, device="meta")), ValueError),
]


@pytest.mark.parametrize("kw,exc", _COMMON + _PARITY + _OUT + [(dict(sigma=0.05), TypeError), (dict(bogus=1), TypeError)])
def test_bob_fields_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    with pytest.raises(exc):
        bob_fields(kw.pop("fields", _V()), **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _PARITY + _OUT + _SIGMA + _FLOWS + [(dict(bogus=1), TypeError)])
def test_deinterlace_fields_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(fields=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        deinterlace_fields(args.pop("fields"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _PARITY + _OUT + _SIGMA + [(dict(levels=0), ValueError), (dict(bogus=1), TypeError)])
def test_deinterlace_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    fields, levels = kw.pop("fields", _V()), kw.pop("levels", 2)
    with pytest.raises(exc):
        deinterlace_video(fields, levels, **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + [(dict(levels=0), ValueError), (dict(bogus=1), TypeError),
                                             (dict(first=0), TypeError), (dict(out_dtype=torch.float32), TypeError)])
def test_field_flows_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    fields, levels = kw.pop("fields", _V()), kw.pop("levels", 2)
    with pytest.raises(exc):
        field_flows(fields, levels, **kw)
    assert stub == []


@pytest.mark.parametrize("frames,kw,exc", [
    (_z(2, 3, 7, 8), {}, ValueError), (_z(2, 7, 8, 3), dict(layout="NHWC"), ValueError),               # odd heights
    (_z(2, 3, 8, 8), dict(layout="HWC"), ValueError), (_z(2, 3, 0, 8), {}, ValueError), (_z(8, 8), {}, ValueError),
    (np.zeros((2, 3, 8, 8)), {}, TypeError), (None, {}, TypeError),
    (_z(2, 3, 8, 8), dict(top_first=2), ValueError), (_z(2, 3, 8, 8), dict(top_first="yes"), ValueError),
    (_z(2, 3, 8, 8), dict(top_first=None), ValueError),
])
def test_split_fields_errors(frames, kw, exc):
    with pytest.raises(exc):
        split_fields(frames, **kw)


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
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
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
_P = (64, 8, 1, 0)  # a (frame, row, column) plane of 8 x 8
_VS = (384, 24, 3, 1)  # the video of 16 x 8 x 3


def _deint(lib, h, n=4, size=(8, 8, 3), fl=_OK, fw=_OK, bw=_OK, out=_OK, conf=_OK, first=0, mode=1, sigma=0.05):
    make = {"fl": lambda: _t(capi.DTYPE_U8), "fw": lambda: _t(strides=(128, 8, 1, 64)),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)), "out": lambda: _t(capi.DTYPE_U8, _VS, data=0x9000),
            "conf": lambda: _t(capi.DTYPE_F32, _P)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fl=fl, fw=fw, bw=bw, out=out, conf=conf).items()}
    return lib.papof_deinterlace_tensor(h, n, size[0], size[1], size[2], _ref(d["fl"]), first, mode, _ref(d["fw"]), _ref(d["bw"]),
                                        sigma, _ref(d["out"]), _ref(d["conf"]), None)


@pytest.mark.parametrize("kw", [
    dict(fl=None), dict(fw=None), dict(bw=None), dict(out=None),                                        # NULL descriptors
    dict(fl=None, mode=0), dict(out=None, mode=0),
    dict(fl=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(out=_t(capi.DTYPE_U8, _VS, data=0)),  # NULL data
    dict(conf=_t(capi.DTYPE_F64, _P, data=0)), dict(conf=_t(capi.DTYPE_F64, _P, data=0), mode=0),
    dict(fl=_t(dtype=3)), dict(fl=_t(dtype=-1)), dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),      # dtypes
    dict(out=_t(3, _VS, data=0x9000)), dict(out=_t(-1, _VS, data=0x9000)),
    dict(conf=_t(capi.DTYPE_U8, _P)), dict(conf=_t(3, _P)),
    dict(fl=_t(strides=(-192, 24, 3, 1))), dict(fl=_t(strides=(192, 24, 3, -1))),                      # negative strides
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),
    dict(out=_t(capi.DTYPE_U8, (384, -24, 3, 1), data=0x9000)), dict(conf=_t(capi.DTYPE_F64, (64, 8, -1, 0))),
    dict(out=_t(capi.DTYPE_U8, (0, 24, 3, 1), data=0x9000)), dict(out=_t(capi.DTYPE_U8, (384, 0, 3, 1), data=0x9000)),  # zero
    dict(out=_t(capi.DTYPE_U8, (384, 24, 0, 1), data=0x9000)), dict(out=_t(capi.DTYPE_U8, (384, 24, 3, 0), data=0x9000)),
    dict(conf=_t(capi.DTYPE_F32, (0, 8, 1, 0))), dict(conf=_t(capi.DTYPE_F32, (64, 0, 1, 0))),
    dict(conf=_t(capi.DTYPE_F32, (64, 8, 0, 0))),
    dict(out=_t(capi.DTYPE_U8, _VS)), dict(out=_t(capi.DTYPE_U8, _VS), mode=0),                          # video is fields
    dict(n=3), dict(n=1), dict(n=0), dict(n=-4), dict(n=3, mode=0),                                     # sizes
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(-1, 8, 3)), dict(size=(8, 8, 0)), dict(size=(8, 8, 5)),
    dict(size=(1 << 30, 8, 3)),
    dict(first=2), dict(first=-1), dict(mode=2), dict(mode=-1),                                         # parity and mode
    dict(sigma=0.0), dict(sigma=-0.05), dict(sigma=math.nan), dict(sigma=math.inf), dict(sigma=0.0, mode=0),  # sigma
])
def test_c_abi_deinterlace_refuses(kw):
    assert _deint(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_deinterlace_without_a_handle():
    lib = _lib()
    assert _deint(lib, None) == -1
    assert _deint(lib, None, conf=None) == -1
    assert _deint(lib, None, mode=0, fw=None, bw=None, conf=None) == -1
