"""CPU-side checks of dirt and dropout removal (papteam_opticalflow_amd/tensors.py: detect_defects, dilate_masks,
repair_defects, restore_video; include/papof.h: papof_defect_detect_tensor, papof_mask_dilate_tensor): known answers of the
numpy fp64 restatement in tests/_restore_ref.py that tests/test_gpu_restore.py compares the device's output with, the
calibration of the defaults on a panning crop of the committed 1080p frame with blotches, with exact flows and with the
oracle's, every Python argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C
ABI through ctypes.  No device is touched here."""
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _interp_ref import as_f64  # noqa: E402
from _restore_ref import detect_reference, dilate_reference, repair_reference, restore_reference  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402

THR = 0.08


def _zero_flows(T, H, W):
    return np.zeros((T - 1, 2, H, W)), np.zeros((T - 1, 2, H, W))


def _static(T, H, W, C, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random((H, W, C))] * T)


# ---- known answers of the detector
@pytest.mark.parametrize("T", [3, 4, 6])
@pytest.mark.parametrize("consistency", [None, (0.01, 0.5)])
def test_a_static_scene_scores_zero(T, consistency):
    F = _static(T, 6, 9, 3)
    mask, score, support = detect_reference(F, *_zero_flows(T, 6, 9), 0.0, consistency)
    assert (score == 0.0).all() and not mask.any() and (support == 2).all()
    assert mask.dtype == np.uint8 and score.dtype == np.float64 and support.dtype == np.uint8


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_pixel_off_by_delta_scores_exactly_delta(sign):
    """a brighter pixel scores (v + d) - v, a darker one v - (v - d): flagged only when strictly above the threshold"""
    T, H, W = 5, 5, 7
    v, d = 0.3, 0.1
    F = np.full((T, H, W, 1), v)
    F[2, 1, 4, 0] = v + sign * d
    want = (v + d) - v if sign > 0 else v - (v - d)
    fw, bw = _zero_flows(T, H, W)
    mask, score, _ = detect_reference(F, fw, bw, want)
    assert score[2, 1, 4] == want and not mask.any()  # score == threshold: not flagged
    mask, score, _ = detect_reference(F, fw, bw, np.nextafter(want, 0.0))
    assert mask[2, 1, 4] == 1 and mask.sum() == 1
    only = np.zeros((T, H, W))
    only[2, 1, 4] = want
    assert (score == only).all()  # its neighbours in time see it as one end of their range: 0


def test_a_centre_between_its_references_scores_zero():
    T, H, W = 3, 4, 4
    F = np.empty((T, H, W, 1))
    F[0], F[1], F[2] = 0.2, 0.3, 0.5
    _, score, _ = detect_reference(F, *_zero_flows(T, H, W), THR)
    assert (score[1] == 0.0).all()
    # the end frames lie outside the range of the two frames beside them: by 0.3 - 0.2 and 0.5 - 0.3
    assert (score[0] == 0.3 - 0.2).all() and (score[2] == 0.5 - 0.3).all()


def test_a_defect_that_persists_is_not_flagged():
    T, H, W = 6, 5, 5
    F = np.full((T, H, W, 1), 0.4)
    F[2, 2, 2, 0] = F[3, 2, 2, 0] = 0.9
    mask, score, _ = detect_reference(F, *_zero_flows(T, H, W), THR)
    assert not mask.any() and (score == 0.0).all()
    # the end frames are weaker: a defect of frames 1 and 2 is both references of frame 0, whose sound pixel is flagged
    F[:] = 0.4
    F[1, 2, 2, 0] = F[2, 2, 2, 0] = 0.9
    mask, score, _ = detect_reference(F, *_zero_flows(T, H, W), THR)
    assert mask.sum() == 1 and mask[0, 2, 2] == 1 and score[0, 2, 2] == 0.9 - 0.4


def test_the_maximum_over_the_channels_is_taken():
    T, H, W = 3, 3, 3
    F = np.full((T, H, W, 4), 0.5)
    F[1, 1, 1] = (0.5 + 0.05, 0.5 - 0.2, 0.5 + 0.1, 0.5)
    _, score, _ = detect_reference(F, *_zero_flows(T, H, W), THR)
    assert score[1, 1, 1] == 0.5 - (0.5 - 0.2)
    _, score, _ = detect_reference(F[..., :1], *_zero_flows(T, H, W), THR)
    assert score[1, 1, 1] == (0.5 + 0.05) - 0.5


@pytest.mark.parametrize("T", [3, 4, 5])
def test_the_end_frames_use_the_two_frames_beside_them(T):
    """frame 0 is judged against frames 1 and 2, frame T - 1 against T - 2 and T - 3, along one chain of two hops"""
    H, W, dx, dy = 9, 12, 2, 1
    rng = np.random.default_rng(2)
    big = rng.random((H + T * dy, W + T * dx, 2))
    F = np.stack([big[t * dy:t * dy + H, t * dx:t * dx + W] for t in range(T)])  # the scene moves by (-dx, -dy) per frame
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = -dx, -dy
    F[0, 5, 7, 1] += 0.25
    F[T - 1, 3, 4, 0] -= 0.125
    mask, score, support = detect_reference(F, fw, -fw, 0.1)
    want = np.zeros((T, H, W))
    want[0, 5, 7], want[T - 1, 3, 4] = 0.25, 0.125
    assert np.abs(score - want).max() < 1e-15 and mask.sum() == 2 and mask[0, 5, 7] == 1 and mask[T - 1, 3, 4] == 1
    # frame 0's chain goes forward twice: it leaves through the left and top borders after one hop (support 0) or two (1)
    x, r = np.meshgrid(np.arange(W), np.arange(H))
    hops = lambda x, r: (x >= 0) & (r >= 0) & (x <= W - 1) & (r <= H - 1)  # noqa: E731
    assert (support[0] == hops(x - dx, r - dy).astype(int) + (hops(x - dx, r - dy) & hops(x - 2 * dx, r - 2 * dy))).all()
    assert (support[T - 1] == hops(x + dx, r + dy).astype(int) + (hops(x + dx, r + dy) & hops(x + 2 * dx, r + 2 * dy))).all()
    for t in range(1, T - 1):
        assert (support[t] == hops(x - dx, r - dy).astype(int) + hops(x + dx, r + dy)).all()
    # the same defect in frame 1 (where frame 0's pixel lands) hides frame 0's: frame 1 is its first reference
    F[1, 5 - dy, 7 - dx, 1] += 0.25
    mask, _, _ = detect_reference(F, fw, -fw, 0.1)
    assert mask[0, 5, 7] == 0


def test_a_reference_that_leaves_the_image_is_not_judged():
    T, H, W = 3, 4, 6
    F = np.full((T, H, W, 1), 0.5)
    F[1, 2, 1, 0] = 1.0
    F[1, 2, 3, 0] = 1.0
    fw, bw = _zero_flows(T, H, W)
    fw[1, 0, 2, 1] = -4.0  # frame 1's forward hop at (1, 2) leaves the image
    mask, score, support = detect_reference(F, fw, bw, THR)
    assert support[1, 2, 1] == 1 and score[1, 2, 1] == 0.0 and mask[1, 2, 1] == 0
    assert support[1, 2, 3] == 2 and score[1, 2, 3] == 0.5 and mask[1, 2, 3] == 1
    fw[1, 0, 2, 1] = math.nan
    assert detect_reference(F, fw, bw, THR)[2][1, 2, 1] == 1


def test_a_failed_check_is_not_judged_when_consistency_is_set():
    T, H, W = 4, 4, 8
    F = np.full((T, H, W, 1), 0.5)
    F[1, 2, 1, 0] = 1.0
    fw, bw = _zero_flows(T, H, W)
    bw[1, 0, 2, 1] = 3.0  # pair 1 at (1, 2): the backward flow does not undo the forward one
    mask, score, support = detect_reference(F, fw, bw, THR, (0.01, 0.5))
    assert support[1, 2, 1] == 1 and score[1, 2, 1] == 0.0 and mask[1, 2, 1] == 0
    # frame 0's chain dies on its second hop there: reference 1 alive, reference 2 not
    assert support[0, 2, 1] == 1 and (np.delete(support[0].ravel(), 2 * W + 1) == 2).all()
    mask, score, support = detect_reference(F, fw, bw, THR, None)
    assert support[1, 2, 1] == 2 and score[1, 2, 1] == 0.5 and mask[1, 2, 1] == 1


def test_nan_samples_never_flag():
    T, H, W = 5, 3, 3
    F = np.full((T, H, W, 2), 0.5)
    F[2, 1, 1, 0] = math.nan
    mask, score, support = detect_reference(F, *_zero_flows(T, H, W), 0.0)
    assert not mask.any() and (score == 0.0).all() and (support == 2).all()
    # a NaN first reference silences its channel: frame 3's bump in channel 0 goes unseen, the one in channel 1 is seen
    F[3, 1, 1] = (0.9, 0.75)
    mask, score, _ = detect_reference(F, *_zero_flows(T, H, W), THR)
    assert score[3, 1, 1] == 0.75 - 0.5 and mask[3, 1, 1] == 1
    mask, score, _ = detect_reference(F[..., :1], *_zero_flows(T, H, W), THR)
    assert score[3, 1, 1] == 0.0 and mask[3, 1, 1] == 0
    # a NaN second reference (frame 4's: frame 2) leaves the first alone, a range of one point: the finite sample decides
    assert score[4, 1, 1] == 0.9 - 0.5 and mask[4, 1, 1] == 1 and mask.sum() == 1


# ---- known answers of the dilation
def test_radius_zero_is_the_mask_as_zero_and_one():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 3, (2, 5, 9)).astype(np.uint8) * 127
    out = dilate_reference(m, 0)
    assert out.dtype == np.uint8 and (out == (m != 0)).all()


@pytest.mark.parametrize("radius", [1, 2, 5])
def test_one_pixel_becomes_a_square_clipped_at_the_borders(radius):
    H, W = 9, 13
    for r, x in ((4, 6), (0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 6), (4, W - 1), (1, 1)):
        m = np.zeros((1, H, W), bool)
        m[0, r, x] = True
        want = np.zeros((1, H, W), np.uint8)
        want[0, max(r - radius, 0):r + radius + 1, max(x - radius, 0):x + radius + 1] = 1
        assert (dilate_reference(m, radius) == want).all(), (r, x)


def test_a_radius_beyond_the_image():
    m = np.zeros((3, 4, 7), np.uint8)
    m[1, 3, 0] = 9
    out = dilate_reference(m, 32)
    assert (out[1] == 1).all() and not out[0].any() and not out[2].any()
    m = np.zeros((1, 1, 70), np.uint8)
    m[0, 0, 3] = 1
    want = np.zeros((1, 1, 70), np.uint8)
    want[0, 0, :36] = 1
    assert (dilate_reference(m, 32) == want).all()


# ---- the calibration of the defaults
T_SCENE, H_SCENE, W_SCENE = 7, 120, 200


def defect_scene(heavy=False):
    """The committed 1920x1080 frame cropped to 120 x 200 at (row 300, column 800) and panned by (2, 1) px per frame, 7
    frames, with opaque elliptical blotches at random places: 6 per frame with axes of 2 .. 9 px (default_rng(5)), or --
    heavy -- 10 per frame with axes of 3 .. 14 px (default_rng(6)); a blotch is one value of [0, 40) or [215, 256), equal
    chance, in all channels.  -> (clean, damaged (T, H, W, 3) uint8, truth (T, H, W) bool: where they differ, the exact
    flow_fw, flow_bw)"""
    import cases
    T, H, W = T_SCENE, H_SCENE, W_SCENE
    rng = np.random.default_rng(6 if heavy else 5)
    img = cases.load_frame_u8("1920", 1)
    clean = np.stack([img[300 + t:300 + t + H, 800 + 2 * t:800 + 2 * t + W] for t in range(T)])
    n, lo, hi = (10, 3.0, 14.0) if heavy else (6, 2.0, 9.0)
    y, x = np.mgrid[0:H, 0:W]
    damaged = clean.copy()
    for t in range(T):
        for _ in range(n):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            a, b = rng.uniform(lo, hi, 2)
            v = rng.integers(0, 40) if rng.random() < 0.5 else rng.integers(215, 256)
            damaged[t][((x - cx) / (a / 2)) ** 2 + ((y - cy) / (b / 2)) ** 2 <= 1.0] = v
    fw = np.zeros((T - 1, 2, H, W))
    fw[:, 0], fw[:, 1] = -2.0, -1.0
    return clean, damaged, (damaged != clean).any(-1), fw, -fw


def _psnr(a, b, where=None):
    d = (as_f64(a) - as_f64(b)) ** 2
    return 10.0 * math.log10(1.0 / float((d if where is None else d[where]).mean()))


def figures(video, detected, clean, damaged, truth, threshold=THR):
    """(recall over all defect pixels, recall over those damaged by more than 2 x threshold, false alarms as a share of the
    sound pixels, PSNR over the true defects, PSNR of the whole video)"""
    significant = truth & (np.abs(as_f64(damaged) - as_f64(clean)).max(-1) > 2 * threshold)
    return (float((detected & truth).sum() / truth.sum()), float((detected & significant).sum() / significant.sum()),
            float((detected & ~truth).sum() / (~truth).sum()), _psnr(video, clean, truth), _psnr(video, clean))


# measured on the restatement (test_quality_calibration's docstring): recall, significant recall, false alarms, PSNR over
# the true defects, whole-frame PSNR
EXACT = (0.8914, 0.9630, 0.0, 29.91, 51.82)
ESTIMATED = {1: (0.8497, 0.9038, 0.00151, 16.57, 38.39), 2: (0.8768, 0.9346, 0.00164, 19.87, 41.96)}
HEAVY = {1: (0.8200, 0.8455, 0.00570, 15.96, 30.81), 2: (0.9118, 0.9415, 0.00627, 21.44, 36.81)}
UNJUDGED = 0.05


def meets(got, measured, exact=False):
    """the bars of a calibrated tuple: recall minus 0.03, false alarms at most twice the measured share (none with exact
    flows), PSNR minus 3 dB"""
    recall, significant, false, over_defects, whole = got
    assert recall >= measured[0] - 0.03 and significant >= measured[1] - 0.03, (got, measured)
    assert false == 0.0 if exact else false <= 2 * measured[2], (got, measured)
    assert over_defects >= measured[3] - 3.0 and whole >= measured[4] - 3.0, (got, measured)


def _passes(damaged, flows_of, n):
    """restore_reference's passes one by one: [(video, masks, detected so far)]"""
    out, detected, video = [], None, damaged
    for _ in range(n):
        video, m, det, _ = repair_reference(damaged, *flows_of(video), masks=detected, threshold=THR, dilate=tensors.DEFECT_DILATE)
        detected = det if detected is None else detected | det
        out.append((video, m, detected))
    return out


def _calibrate(heavy, measured):
    from test_inpaint_cpu import oracle_flows
    clean, damaged, truth, fw, bw = defect_scene(heavy)
    print("%d defect pixels; damaged: PSNR %.2f dB over them, %.2f dB whole" % (truth.sum(), _psnr(damaged, clean, truth),
                                                                                 _psnr(damaged, clean)))
    runs = _passes(damaged, lambda v: oracle_flows(v, 4), 2)
    for k, (video, m, detected) in enumerate(runs):
        got = figures(video, detected, clean, damaged, truth)
        print("oracle's flows, %d pass(es): recall %.4f, significant %.4f, false alarms %.5f, PSNR %.2f dB over the defects, "
              "%.2f dB whole" % ((k + 1,) + got))
        assert (video[~m] == damaged[~m]).all()  # outside the repaired set: the input's bytes
        meets(got, measured[k + 1])
    return clean, damaged, truth, fw, bw, runs


def test_quality_calibration():
    """The scene of defect_scene(): 958 defect pixels, 28.14 dB whole and 5.70 dB over the defects as damaged.  The defaults
    (threshold 0.08, dilate 2, 2 passes), measured here on the restatement:
                                    recall   significant   false alarms   PSNR over defects   whole
        exact flows, 1 pass         0.8914     0.9630        0 (exactly)      29.91 dB        51.82 dB   (2 passes: the same)
        oracle's flows (4 levels), 1 pass
                                    0.8497     0.9038        0.00151          16.57           38.39
        2 passes                    0.8768     0.9346        0.00164          19.87           41.96
    (significant: damaged by more than 2 x threshold).  The detector alone with exact flows flags nothing outside the
    defects at thresholds 0.06, 0.08 and 0.1 and finds 0.9175, 0.8914 and 0.8685 of them.  3.63 % of the pixels are not
    judged with exact flows -- the strips that the pan carries out of the frame in one or two hops -- and 37 of the 958
    defect pixels, in blotches that straddle those strips, are never in a repaired set: they carry 86 % of the squared
    error that is left after one pass with the oracle's flows, and hold the PSNR over the defects where it is.  With dilate
    1 and 3 the oracle's flows gave 15.58 and 21.43 dB over the defects after two passes (37.94 and 43.38 dB whole); 2, what
    inpaint_video's calibration used, stays the default.  Bars: recall minus 0.03, twice the false alarms (exactly none with
    exact flows), PSNR minus 3 dB, less than 5 % unjudged."""
    assert (tensors.DEFECT_THRESHOLD, tensors.DEFECT_DILATE, tensors.DEFECT_PASSES) == (THR, 2, 2)
    for f in (tensors.detect_defects, tensors.repair_defects, tensors.restore_video):
        assert f.__kwdefaults__["threshold"] == THR and f.__kwdefaults__["consistency"] is None
    for f in (tensors.repair_defects, tensors.restore_video):
        assert f.__kwdefaults__["dilate"] == 2 and f.__kwdefaults__["relax"] == tensors.RELAX
    assert tensors.restore_video.__kwdefaults__["passes"] == 2
    clean, damaged, truth, fw, bw, runs = _calibrate(False, ESTIMATED)
    for thr in (0.06, THR, 0.1):
        mask, _, support = detect_reference(damaged, fw, bw, thr)
        print("exact flows, threshold %.2f: recall %.4f, %d flagged outside the defects, %.4f unjudged"
              % (thr, (mask[truth] != 0).mean(), (mask[~truth] != 0).sum(), (support < 2).mean()))
        assert not mask[~truth].any() and (support < 2).mean() < UNJUDGED
    exact = _passes(damaged, lambda v: (fw, bw), 2)
    for k, (video, m, detected) in enumerate(exact):
        got = figures(video, detected, clean, damaged, truth)
        print("exact flows, %d pass(es): recall %.4f, significant %.4f, false alarms %.5f, PSNR %.2f dB over the defects, %.2f dB "
              "whole" % ((k + 1,) + got))
        assert (video[~m] == damaged[~m]).all()
        meets(got, EXACT, exact=True)
    # two passes beat one, and both beat the damaged video by far
    assert _psnr(runs[1][0], clean) > _psnr(runs[0][0], clean) > _psnr(damaged, clean) + 6.0
    # restore_reference is those passes
    flows = iter([(fw, bw), (fw, bw)])
    video, m, detected, _, _ = restore_reference(damaged, lambda v: next(flows), 2, threshold=THR, dilate=2)
    assert (video == exact[1][0]).all() and (m == exact[1][1]).all() and (detected == exact[1][2]).all()


def test_quality_calibration_heavy():
    """defect_scene(heavy=True): 4173 defect pixels, 22.32 dB whole as damaged.  With the oracle's flows: 30.81 dB whole after
    one pass (recall 0.8200, false alarms 0.00570), 36.81 dB after two (0.9118, 0.00627); with exact flows 41.02 dB, recall
    0.9137, and 15 sound pixels flagged, where blotches of the two neighbouring frames bracket them."""
    _calibrate(True, HEAVY)


def test_pixels_outside_the_masks_are_the_inputs_bytes():
    rng = np.random.default_rng(7)
    T, H, W = 4, 12, 17
    frames = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    fw = rng.normal(0, 0.5, (T - 1, 2, H, W))
    given = rng.random((T, H, W)) < 0.05
    video, m, detected, st = repair_reference(frames, fw, -fw, masks=given, threshold=0.3, dilate=1)
    assert (video[~m] == frames[~m]).all() and video.dtype == np.uint8
    assert (m >= given).all() and (m >= detected).all() and ((st > 0) == m).all()
    assert (m == (dilate_reference(detected | given, 1) != 0)).all()
    v32, m32, _, _ = repair_reference(frames.astype(np.float32) / 255, fw, -fw, masks=given, threshold=0.3, dilate=1)
    assert v32.dtype == np.float32 and (v32[~m32] == (frames.astype(np.float32) / 255)[~m32]).all()


# ---- Python argument errors, before any launch
@pytest.fixture
def stub(monkeypatch):
    """a handle that records calls: none may be made when the arguments are refused"""
    calls = []
    monkeypatch.setattr(tensors, "_handle", lambda device: calls.append(device))
    return calls


def _z(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


_V = lambda: _z(4, 3, 8, 8)  # noqa: E731
_M = lambda: _z(4, 8, 8, dtype=torch.bool)  # noqa: E731
_F = lambda: _z(3, 2, 8, 8)  # noqa: E731


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: tensors.detect_defects(_V(), _F(), _F()), ValueError),                                  # CPU tensors
    (lambda: tensors.detect_defects(None, _F(), _F()), TypeError),
    (lambda: tensors.dilate_masks(_M(), 2), ValueError),
    (lambda: tensors.dilate_masks(None, 2), TypeError),
    (lambda: tensors.repair_defects(_V(), _F(), _F()), ValueError),
    (lambda: tensors.repair_defects(None, _F(), _F()), TypeError),
    (lambda: tensors.restore_video(_V(), 2), ValueError),
    (lambda: tensors.restore_video(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_COMMON = [
    (dict(threshold=-0.1), ValueError), (dict(threshold=math.nan), ValueError), (dict(threshold=math.inf), ValueError),
    (dict(threshold="0.1"), TypeError), (dict(threshold=True), TypeError), (dict(threshold=None), TypeError),
    (dict(consistency=(0.01, -1.0)), ValueError), (dict(consistency=(math.nan, 0.5)), ValueError),
    (dict(consistency="yes"), TypeError), (dict(consistency=(1, 2, 3)), TypeError),
    (dict(layout="CHWN"), ValueError),
    (dict(frames=_z(4, 5, 8, 8)), ValueError), (dict(frames=_z(4, 8, 8, 5), layout="NHWC"), ValueError),   # channels
    (dict(frames=_z(4, 0, 8, 8)), ValueError), (dict(frames=_z(4, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(frames=_z(2, 3, 8, 8)), ValueError),                                                          # fewer than 3 frames
]
_FLOWS = [
    (dict(frames=_z(2, 3, 8, 8), flow_fw=_z(1, 2, 8, 8), flow_bw=_z(1, 2, 8, 8)), ValueError),
    (dict(flow_fw=_z(3, 2, 8, 8, dtype=torch.uint8)), TypeError), (dict(flow_bw=_z(3, 2, 8, 8, dtype=torch.float16)), TypeError),
    (dict(flow_fw=_z(3, 3, 8, 8), flow_bw=_z(3, 3, 8, 8)), ValueError),
    (dict(flow_fw=_z(4, 2, 8, 8), flow_bw=_z(4, 2, 8, 8)), ValueError),                               # not (T - 1, 2, H, W)
    (dict(flow_fw=_z(3, 2, 8, 9), flow_bw=_z(3, 2, 8, 9)), ValueError), (dict(flow_bw=_z(3, 2, 4, 8)), ValueError),
    (dict(flow_fw=None), TypeError), (dict(flow_bw=np.zeros((3, 2, 8, 8))), TypeError),
    (dict(flow_fw=_z(3, 2, 8, 8, device="meta"), flow_bw=_z(3, 2, 8, 8, device="meta")), ValueError),  # devices
    (dict(flow_bw=_z(3, 2, 8, 8, device="meta")), ValueError),
]
_REPAIR = [
    (dict(dilate=-1), ValueError), (dict(dilate=33), ValueError), (dict(dilate=2.0), ValueError), (dict(dilate=True), ValueError),
    (dict(relax=-1), ValueError), (dict(relax=65537), ValueError), (dict(relax=1.0), ValueError),
    (dict(radius=0), ValueError), (dict(radius=4), ValueError), (dict(radius=1.0), ValueError),
    (dict(out_dtype=torch.float16), TypeError), (dict(out_dtype=torch.int32), TypeError),
    (dict(masks=_z(4, 8, 8)), TypeError), (dict(masks=np.zeros((4, 8, 8), bool)), TypeError),           # masks
    (dict(masks=_z(3, 8, 8, dtype=torch.bool)), ValueError), (dict(masks=_z(4, 8, 9, dtype=torch.uint8)), ValueError),
    (dict(masks=_z(4, 8, 8, dtype=torch.bool, device="meta")), ValueError),
]


@pytest.mark.parametrize("kw,exc", _COMMON + _FLOWS + [(dict(out_dtype=torch.float64), TypeError), (dict(dilate=2), TypeError)])
def test_detect_defects_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        tensors.detect_defects(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _FLOWS + _REPAIR + [(dict(bogus=1), TypeError)])
def test_repair_defects_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    args = dict(frames=_V(), flow_fw=_F(), flow_bw=_F())
    args.update(kw)
    with pytest.raises(exc):
        tensors.repair_defects(args.pop("frames"), args.pop("flow_fw"), args.pop("flow_bw"), **args)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _REPAIR + [
    (dict(passes=0), ValueError), (dict(passes=9), ValueError), (dict(passes=2.0), ValueError), (dict(passes=True), ValueError),
    (dict(levels=0), ValueError), (dict(bogus=1), TypeError),
])
def test_restore_video_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, levels = kw.pop("frames", _V()), kw.pop("levels", 2)
    with pytest.raises(exc):
        tensors.restore_video(frames, levels, **kw)
    assert stub == []


@pytest.mark.parametrize("masks,radius,exc", [
    (_M(), -1, ValueError), (_M(), 33, ValueError), (_M(), 1.0, ValueError), (_M(), True, ValueError), (_M(), None, ValueError),
    (_z(4, 8, 8), 1, TypeError), (_z(4, 8, 8, dtype=torch.int8), 1, TypeError), (np.zeros((4, 8, 8), bool), 1, TypeError),
    (_z(8, dtype=torch.bool), 1, ValueError), (_z(1, 4, 8, 8, dtype=torch.bool), 1, ValueError),
    (_z(4, 0, 8, dtype=torch.bool), 1, ValueError), (_z(4, 8, 8, dtype=torch.bool, device="meta"), 1, ValueError),
])
def test_dilate_masks_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, masks, radius, exc):
    _on_gpu_stub(monkeypatch)
    with pytest.raises(exc):
        tensors.dilate_masks(masks, radius)
    assert stub == []


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


def _detect(lib, h, n=3, size=(8, 8, 3), fr=_OK, fw=_OK, bw=_OK, mk=_OK, sc=_OK, sup=_OK, thr=0.08, check=1, a1=0.01, a2=0.5):
    make = {"fr": lambda: _t(capi.DTYPE_U8), "fw": lambda: _t(strides=(128, 8, 1, 64)),
            "bw": lambda: _t(capi.DTYPE_F32, (128, 8, 1, 64)), "mk": lambda: _t(capi.DTYPE_U8, _P),
            "sc": lambda: _t(capi.DTYPE_F32, _P), "sup": lambda: _t(capi.DTYPE_U8, _P)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(fr=fr, fw=fw, bw=bw, mk=mk, sc=sc, sup=sup).items()}
    return lib.papof_defect_detect_tensor(h, n, size[0], size[1], size[2], _ref(d["fr"]), _ref(d["fw"]), _ref(d["bw"]), thr,
                                          check, a1, a2, _ref(d["mk"]), _ref(d["sc"]), _ref(d["sup"]), None)


@pytest.mark.parametrize("kw", [
    dict(fr=None), dict(fw=None), dict(bw=None), dict(mk=None),                                         # NULL descriptors
    dict(fr=_t(data=0)), dict(fw=_t(data=0)), dict(bw=_t(data=0)), dict(mk=_t(capi.DTYPE_U8, _P, data=0)),  # NULL data
    dict(sc=_t(capi.DTYPE_F64, _P, data=0)), dict(sup=_t(capi.DTYPE_U8, _P, data=0)),
    dict(fr=_t(dtype=3)), dict(fr=_t(dtype=-1)), dict(fw=_t(capi.DTYPE_U8)), dict(bw=_t(dtype=7)),      # dtypes
    dict(mk=_t(capi.DTYPE_F32, _P)), dict(mk=_t(capi.DTYPE_F64, _P)), dict(sc=_t(capi.DTYPE_U8, _P)), dict(sc=_t(3, _P)),
    dict(sup=_t(capi.DTYPE_F32, _P)), dict(sup=_t(capi.DTYPE_F64, _P)),
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr=_t(strides=(192, 24, 3, -1))),                      # negative strides
    dict(fw=_t(strides=(128, -8, 1, 64))), dict(bw=_t(strides=(128, 8, 1, -64))),
    dict(mk=_t(capi.DTYPE_U8, (64, -8, 1, 0))), dict(sc=_t(capi.DTYPE_F64, (64, 8, -1, 0))),
    dict(sup=_t(capi.DTYPE_U8, (-64, 8, 1, 0))),
    dict(mk=_t(capi.DTYPE_U8, (0, 8, 1, 0))), dict(mk=_t(capi.DTYPE_U8, (64, 0, 1, 0))),               # zero strides
    dict(mk=_t(capi.DTYPE_U8, (64, 8, 0, 0))), dict(sc=_t(capi.DTYPE_F32, (0, 8, 1, 0))),
    dict(sc=_t(capi.DTYPE_F32, (64, 0, 1, 0))), dict(sc=_t(capi.DTYPE_F32, (64, 8, 0, 0))),
    dict(sup=_t(capi.DTYPE_U8, (0, 8, 1, 0))), dict(sup=_t(capi.DTYPE_U8, (64, 0, 1, 0))),
    dict(sup=_t(capi.DTYPE_U8, (64, 8, 0, 0))),
    dict(n=2), dict(n=1), dict(n=0), dict(n=-3),                                                        # sizes
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(-1, 8, 3)), dict(size=(8, 8, 0)), dict(size=(8, 8, 5)),
    dict(thr=-0.01), dict(thr=math.nan), dict(thr=math.inf), dict(thr=-math.inf),                       # threshold
    dict(a1=-0.01), dict(a2=-0.5), dict(a1=math.nan), dict(a2=math.inf), dict(a1=math.nan, check=0),   # alphas
])
def test_c_abi_defect_detect_refuses(kw):
    assert _detect(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_defect_detect_without_a_handle():
    lib = _lib()
    assert _detect(lib, None) == -1
    assert _detect(lib, None, sc=None, sup=None) == -1


def _dilate(lib, h, n=2, size=(8, 8), mk=_OK, out=_OK, radius=2):
    make = {"mk": lambda: _t(capi.DTYPE_U8, _P), "out": lambda: _t(capi.DTYPE_U8, _P, data=0x2000)}
    d = {k: make[k]() if isinstance(v, str) else v for k, v in dict(mk=mk, out=out).items()}
    return lib.papof_mask_dilate_tensor(h, n, size[0], size[1], _ref(d["mk"]), radius, _ref(d["out"]), None)


@pytest.mark.parametrize("kw", [
    dict(mk=None), dict(out=None), dict(mk=_t(capi.DTYPE_U8, _P, data=0)), dict(out=_t(capi.DTYPE_U8, _P, data=0)),
    dict(mk=_t(capi.DTYPE_F32, _P)), dict(mk=_t(3, _P)), dict(out=_t(capi.DTYPE_F64, _P, data=0x2000)),
    dict(out=_t(-1, _P, data=0x2000)),
    dict(mk=_t(capi.DTYPE_U8, (-64, 8, 1, 0))), dict(mk=_t(capi.DTYPE_U8, (64, 8, -1, 0))),
    dict(out=_t(capi.DTYPE_U8, (64, -8, 1, 0), data=0x2000)),
    dict(out=_t(capi.DTYPE_U8, (0, 8, 1, 0), data=0x2000)), dict(out=_t(capi.DTYPE_U8, (64, 0, 1, 0), data=0x2000)),
    dict(out=_t(capi.DTYPE_U8, (64, 8, 0, 0), data=0x2000)),
    dict(out=_t(capi.DTYPE_U8, _P)),                                                                     # out is mask
    dict(n=0), dict(n=-1), dict(size=(0, 8)), dict(size=(8, 0)), dict(size=(-2, 8)),
    dict(radius=-1), dict(radius=33), dict(radius=1 << 20),
])
def test_c_abi_mask_dilate_refuses(kw):
    assert _dilate(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_mask_dilate_without_a_handle():
    assert _dilate(_lib(), None) == -1


def test_version():
    assert _lib().papof_version() == 115  # two parallel calls: no call of the ABI changed
