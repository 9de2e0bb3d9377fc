"""CPU-side checks of the shot boundaries (papteam_opticalflow_amd/tensors.py: shot_histograms, shot_distances, detect_cuts,
split_shots, detect_shots, cut_flows, flow_video_shots; include/papof.h: papof_cell_hist_tensor): the numpy restatement in
tests/_shots_ref.py on fifteen scenes with known cuts, cropped from the committed 1080p frame with a fixed seed -- the
package's rule on the restatement's histograms must return exactly the truth at its defaults --, the rule of the package
against the restatement's, properties of the counts and of the pooling, split_shots, cut_flows on host tensors, every Python
argument error raised before a launch (CPU tensors, a stubbed handle), and each refusal of the C ABI through ctypes.  No device
is touched here."""
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _shots_ref import cell_pixels, cuts_reference, distances_reference, hist_reference, luma_reference, quantise  # noqa: E402
from papteam_opticalflow_amd import capi, tensors  # noqa: E402
from papteam_opticalflow_amd.tensors import (FlowFB, ShotHist, cut_flows, detect_cuts, detect_shots, flow_video_shots,  # noqa: E402
                                             shot_distances, shot_histograms, split_shots)

H_SCENE, W_SCENE, T_SCENE = 120, 200, 12
SEED = 7
A, FAR, NEAR, BELOW, THIRD = (300, 200), (700, 1400), (300, 400), (420, 200), (60, 900)  # (row, column) origins of the shots

_CACHE = {}


def _image():
    if "img" not in _CACHE:
        import cases
        _CACHE["img"] = cases.load_frame_u8("1920", 1)
    return _CACHE["img"]


def crop(origin, k=0, pan=(0, 0)):
    """the 120 x 200 x 3 window of the committed 1920 x 1080 frame at origin + k * pan (rows, columns), float64 levels"""
    r, c = origin[0] + k * pan[0], origin[1] + k * pan[1]
    return _image()[r:r + H_SCENE, c:c + W_SCENE].astype(np.float64)


def finish(frames, sigma, rng):
    """Gaussian noise of sigma levels, rounded and clipped to uint8"""
    out = []
    for f in frames:
        if sigma:
            f = f + rng.normal(0.0, sigma, f.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return np.stack(out)


def shots_scene(shots, pan=(1, 3), sigma=2.0, gains=None, seed=SEED):
    """frames (T, 120, 200, 3) uint8: `shots` is a list of (origin, number of frames); every frame k of the video is its
    shot's window moved by k * pan; gains: {frame: gain}"""
    rng = np.random.default_rng(seed)
    frames, k = [], 0
    for origin, n in shots:
        for _ in range(n):
            frames.append(crop(origin, k, pan) * (gains or {}).get(k, 1.0))
            k += 1
    return finish(frames, sigma, rng)


def dissolve_scene(seed=SEED):
    """frames 0 .. 4 of shot A, 5 .. 7 blends of 1/4, 1/2 and 3/4 of the far shot, 8 .. 11 the far shot: the pairs 4 .. 7 change"""
    rng = np.random.default_rng(seed)
    alpha = [0.0] * 5 + [0.25, 0.5, 0.75] + [1.0] * 4
    return finish([(1 - a) * crop(A, k, (1, 3)) + a * crop(FAR, k, (1, 3)) for k, a in enumerate(alpha)], 2.0, rng)


def ramp_scene(seed=SEED):
    """an exposure ramp of 5 % per frame"""
    return shots_scene([(A, T_SCENE)], gains={k: 0.75 * 1.05 ** k for k in range(T_SCENE)}, seed=seed)


def occluder_scene(seed=SEED):
    """a 48 x 48 block of mid grey that crosses the static shot at 15 pixels per frame"""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(T_SCENE):
        f = crop(A)
        f[36:84, 15 * k:15 * k + 48] = 128.0
        frames.append(f)
    return finish(frames, 2.0, rng)


# name: (builder, cuts, flashes) -- the issue's list; the last three have their own assertions
SCENES = {
    "static": (lambda: shots_scene([(A, 12)], pan=(0, 0)), [], []),
    "pan (4, 25) noise 5": (lambda: shots_scene([(A, 12)], pan=(4, 25), sigma=5.0), [], []),
    "cut at 7": (lambda: shots_scene([(A, 8), (FAR, 4)]), [7], []),
    "cut at 7, pan (4, 25)": (lambda: shots_scene([(A, 8), (FAR, 4)], pan=(4, 25), sigma=5.0), [7], []),
    "near cut": (lambda: shots_scene([(A, 8), (NEAR, 4)], pan=(0, 0)), [7], []),
    "two-frame shot": (lambda: shots_scene([(A, 8), (FAR, 2), (THIRD, 2)]), [7, 9], []),
    "one-frame shot": (lambda: shots_scene([(A, 8), (FAR, 1), (THIRD, 3)]), [7, 8], []),
    "first frame alone": (lambda: shots_scene([(A, 1), (FAR, 11)]), [0], []),
    "last frame alone": (lambda: shots_scene([(A, 11), (FAR, 1)]), [10], []),
    "flash at 4": (lambda: shots_scene([(A, 12)], gains={4: 1.8}), [], [4]),
    "flash at 3, cut at 7": (lambda: shots_scene([(A, 8), (FAR, 4)], gains={3: 1.8}), [7], [3]),
    "noise 10": (lambda: shots_scene([(A, 12)], sigma=10.0), [], []),
    "dissolve": (dissolve_scene, [4, 5, 6, 7], []),
    "exposure ramp": (ramp_scene, [], []),
    "occluder": (occluder_scene, [], []),
}
SCENE_NAMES = list(SCENES)
TRUTHS = SCENE_NAMES[:12]


def scene_frames(name):
    if name not in _CACHE:
        _CACHE[name] = SCENES[name][0]()
    return _CACHE[name]


def scene_hist(name):
    key = ("hist", name)
    if key not in _CACHE:
        _CACHE[key] = hist_reference(scene_frames(name))
    return _CACHE[key]


def _host(hist, cell_rows=16, size=(H_SCENE, W_SCENE)):
    return ShotHist(torch.from_numpy(np.ascontiguousarray(hist)), cell_rows, int(hist.shape[-1]), size)


# ---- the scenes
@pytest.mark.parametrize("name", TRUTHS)
def test_the_cuts_are_the_truth_on_every_scene(name):
    """defaults: cells of 16 rows, 16 bins, pool (4, 2), floor 0.2, ratio 3, window 4"""
    _, cuts, flashes = SCENES[name]
    s = detect_cuts(_host(scene_hist(name)))
    print("%s: cuts %s flashes %s d %s" % (name, s.cuts, s.flashes, " ".join("%.3f" % x for x in s.distances)))
    assert (s.cuts, s.flashes, s.gradual) == (cuts, flashes, []), name
    assert s.ranges == split_shots(T_SCENE, cuts) and s.distances.shape == (T_SCENE - 1,) and s.distances.dtype == np.float64


def test_a_dissolve_is_a_run_of_cuts_and_a_gradual_range():
    s = detect_cuts(_host(scene_hist("dissolve")))
    assert s.cuts == [4, 5, 6, 7] and s.gradual == [(4, 7)] and s.flashes == []
    assert s.ranges == [(0, 5), (5, 6), (6, 7), (7, 8), (8, 12)]


@pytest.mark.parametrize("name", ["exposure ramp", "occluder"])
def test_what_is_not_a_cut(name):
    s = detect_cuts(_host(scene_hist(name)))
    print("%s: d %s" % (name, " ".join("%.3f" % x for x in s.distances)))
    assert s.cuts == [] and s.flashes == [] and s.gradual == [] and s.ranges == [(0, T_SCENE)]
    assert s.distances.max() < tensors.CUT_FLOOR


def test_the_distances_of_the_docstrings():
    """the figures that detect_cuts' docstring and tensors.CUT_FLOOR's comment quote"""
    d = lambda name: distances_reference(scene_hist(name))  # noqa: E731
    assert d("static").max() < 0.03 and 0.1 < d("pan (4, 25) noise 5").max() < 0.139
    assert d("exposure ramp").max() < 0.059 and d("occluder").max() < 0.055
    assert d("cut at 7")[7] > 0.85 and 0.33 < d("near cut")[7] < 0.34
    flash = d("flash at 4")
    assert min(flash[3], flash[4]) > 0.306 and distances_reference(scene_hist("flash at 4"), step=2)[3] < 0.035
    below = distances_reference(hist_reference(shots_scene([(A, 8), (BELOW, 4)], pan=(0, 0))))
    assert below[7] > 0.3 and np.delete(below, 7).max() < 0.03


def test_the_packages_rule_is_the_restatements_on_every_scene():
    for name in SCENE_NAMES:
        h = scene_hist(name)
        cuts, flashes, gradual, d, ranges = cuts_reference(h)
        s = detect_cuts(_host(h))
        assert (s.cuts, s.flashes, s.gradual, s.ranges) == (cuts, flashes, gradual, ranges), name
        assert s.distances.tobytes() == d.tobytes(), name
        for step in (2, 3):
            assert shot_distances(_host(h), step=step).tobytes() == distances_reference(h, step=step).tobytes(), name
        assert shot_distances(_host(h), pool=(1, 3)).tobytes() == distances_reference(h, pool=(1, 3)).tobytes(), name
    h = scene_hist("flash at 3, cut at 7")
    for kw in (dict(floor=0.3), dict(ratio=1.0, floor=0.01), dict(window=1), dict(pool=(8, 4))):
        want = cuts_reference(h, **kw)
        s = detect_cuts(_host(h), **kw)
        assert (s.cuts, s.flashes, s.gradual) == want[:3], kw


# ---- properties
def test_quantisation_and_luma():
    assert quantise(np.array([0, 1, 255], np.uint8)).tolist() == [0, 257, 65535]
    v = np.array([np.nan, -np.inf, -0.5, 0.0, 0.5 / 65535, 1.5 / 65535, 2.5 / 65535, 1.0, 1.5, np.inf])
    assert quantise(v).tolist() == [0, 0, 0, 0, 0, 2, 2, 65535, 65535, 65535]  # half to even
    px = np.array([[[[255, 255, 255, 0], [255, 0, 0, 9], [0, 255, 0, 9], [0, 0, 255, 9]]]], np.uint8)
    assert luma_reference(px)[0, 0].tolist() == [65535, (77 * 65535) >> 8, (150 * 65535) >> 8, (29 * 65535) >> 8]
    assert luma_reference(px[..., :3]).tolist() == luma_reference(px).tolist()          # a fourth channel is not read
    assert luma_reference(px[..., :2])[0, 0].tolist() == [65535, 65535, 0, 0]            # nor a second
    h = hist_reference(px, cell_rows=1, bins=4)
    assert h.shape == (1, 1, 1, 4) and h[0, 0, 0].tolist() == [1, 1, 1, 1]  # 65535 -> 3, 19712 -> 1, 38399 -> 2, 7423 -> 0


@pytest.mark.parametrize("H,W,cell_rows,bins", [(120, 200, 16, 16), (37, 150, 64, 4), (17, 63, 1, 64), (33, 65, 16, 8)])
def test_cell_sums_are_the_cells_pixel_counts(H, W, cell_rows, bins):
    rng = np.random.default_rng(H)
    f = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    h = hist_reference(f, cell_rows, bins)
    assert h.dtype == np.int32 and h.shape == (3, -(-H // cell_rows), -(-W // 64), bins)
    assert (h.sum(-1) == cell_pixels(H, W, cell_rows)[None]).all() and h.sum() == 3 * H * W


def test_pooling():
    h = scene_hist("cut at 7").astype(np.int64)
    assert tensors.pool_cells(h, (1, 1)).tobytes() == h.tobytes()                         # the identity
    whole = tensors.pool_cells(h, (100, 100))
    assert whole.shape == (T_SCENE, 1, 1, 16) and (whole[:, 0, 0] == h.sum((1, 2))).all()   # one clipped region
    p = tensors.pool_cells(h, (4, 2))                                                     # 8 x 4 cells -> 2 x 2 regions
    assert p.shape == (T_SCENE, 2, 2, 16) and (p[:, 1, 1] == h[:, 4:, 2:].sum((1, 2))).all()
    assert (p.sum((1, 2)) == h.sum((1, 2))).all()
    d = shot_distances(_host(scene_hist("cut at 7")), pool=(1, 1))
    assert d.shape == (T_SCENE - 1,) and (d >= 0).all() and (d <= 1).all()
    assert shot_distances(_host(scene_hist("cut at 7")), step=T_SCENE).shape == (0,)
    one = hist_reference(np.zeros((2, 8, 8, 1), np.uint8))
    one[1] = np.roll(one[1], 1, -1)  # every pixel in another bin: disjoint histograms
    assert shot_distances(_host(one, size=(8, 8))).tolist() == [1.0]


def test_split_shots():
    assert split_shots(5, []) == [(0, 5)] and split_shots(1, []) == [(0, 1)]
    assert split_shots(5, [0, 3]) == [(0, 1), (1, 4), (4, 5)]             # cuts at 0 and T - 2
    assert split_shots(6, [2, 3]) == [(0, 3), (3, 4), (4, 6)]             # adjacent cuts: a one-frame shot
    assert split_shots(4, (2, 0, 1)) == [(0, 1), (1, 2), (2, 3), (3, 4)]  # any order; every pair a cut
    assert split_shots(5, np.array([1])) == [(0, 2), (2, 5)] and split_shots(5, torch.tensor([1])) == [(0, 2), (2, 5)]
    for bad, exc in (([4], ValueError), ([-1], ValueError), ([1, 1], ValueError), ([0.5], TypeError), (None, TypeError),
                     ([True], TypeError), ([[1]], TypeError)):
        with pytest.raises(exc):
            split_shots(5, bad)
    for n in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            split_shots(n, [])


def _fb(B=4, H=3, W=5, occlusion=True, warp=True, dtype=torch.float64):
    g = torch.Generator().manual_seed(3)
    flow = lambda: torch.randn((B, 2, H, W), generator=g, dtype=dtype)  # noqa: E731
    warps = (torch.rand((B, H, W, 2), generator=g), torch.rand((B, H, W, 2), generator=g)) if warp else (None, None)
    occ = torch.rand((B, 2, H, W), generator=g) < 0.3 if occlusion else None
    return FlowFB(flow(), flow(), *warps, occ, {"Total C++ Execution": "0.100000"})


def test_cut_flows_on_host_tensors():
    fb = _fb()
    kept = [t.clone() for t in fb[:5]]
    out = cut_flows(fb, [2, 0])
    for t, k in zip(fb[:5], kept):
        assert torch.equal(t, k)                                                    # the input is left as it was
    for o, k in zip(out[:5], kept):
        assert o.data_ptr() != k.data_ptr() and torch.equal(o[[1, 3]], k[[1, 3]])   # a copy; the other pairs unchanged
    for f in (out.flow_fw, out.flow_bw):
        assert (f[[0, 2]].view(torch.int64) == 0x7ff8000000000000).all()            # the quiet NaN
    assert out.occlusion[[0, 2]].all() and not out.warpI2_fw[[0, 2]].any() and not out.warpI2_bw[[0, 2]].any()
    assert out.timing is fb.timing
    bare = cut_flows(_fb(occlusion=False, warp=False, dtype=torch.float32), [3])
    assert bare.occlusion is None and bare.warpI2_fw is None and (bare.flow_fw[3].view(torch.int32) == 0x7fc00000).all()
    none = cut_flows(fb, [])
    assert all(torch.equal(o, k) and o.data_ptr() != k.data_ptr() for o, k in zip(none[:5], kept))
    for bad, exc in (([4], ValueError), ([-1], ValueError), ([1, 1], ValueError), ([0.5], TypeError), (None, TypeError)):
        with pytest.raises(exc):
            cut_flows(fb, bad)
    with pytest.raises(TypeError):
        cut_flows(tuple(fb), [0])
    with pytest.raises(ValueError):
        cut_flows(fb._replace(flow_bw=fb.flow_bw[:3]), [0])
    with pytest.raises(ValueError):
        cut_flows(fb._replace(occlusion=fb.occlusion[:3]), [0])
    with pytest.raises(TypeError):
        cut_flows(fb._replace(flow_fw=fb.flow_fw.to(torch.float16)), [0])


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


def _on_gpu_stub(monkeypatch):
    monkeypatch.setattr(tensors, "_on_gpu", lambda t: t.device.type != "meta")  # CPU tensors pass for device ones


@pytest.mark.parametrize("call,exc", [
    (lambda: shot_histograms(_V()), ValueError), (lambda: shot_histograms(None), TypeError),   # CPU tensors
    (lambda: detect_shots(_V()), ValueError), (lambda: detect_shots(None), TypeError),
    (lambda: flow_video_shots(_V(), 2), ValueError), (lambda: flow_video_shots(None, 2), TypeError),
])
def test_argument_errors_before_any_launch(stub, call, exc):
    with pytest.raises(exc):
        call()
    assert stub == []


_COMMON = [
    (dict(layout="CHWN"), ValueError),
    (dict(frames=_z(5, 5, 8, 8)), ValueError), (dict(frames=_z(5, 8, 8, 5), layout="NHWC"), ValueError),   # channels
    (dict(frames=_z(5, 0, 8, 8)), ValueError), (dict(frames=_z(5, 3, 8, 8, dtype=torch.int16)), TypeError),
    (dict(frames=_z(0, 3, 8, 8)), ValueError),
    (dict(frames=_z(8, 8)), ValueError), (dict(frames=np.zeros((5, 3, 8, 8))), TypeError),
    (dict(frames=_z(5, 3, 8, 8, device="meta")), ValueError),
]
_CELLS = [
    (dict(cell_rows=0), ValueError), (dict(cell_rows=65), ValueError), (dict(cell_rows=16.0), ValueError),
    (dict(cell_rows=True), ValueError), (dict(bins=0), ValueError), (dict(bins=12), ValueError), (dict(bins=128), ValueError),
    (dict(bins=16.0), ValueError), (dict(bins=True), ValueError), (dict(bins=None), ValueError),
]
_RULE = [
    (dict(floor=-0.1), ValueError), (dict(floor=1.5), ValueError), (dict(floor=math.nan), ValueError), (dict(floor="0.2"), TypeError),
    (dict(floor=None), TypeError), (dict(floor=True), TypeError),
    (dict(ratio=0.5), ValueError), (dict(ratio=math.inf), ValueError), (dict(ratio=None), TypeError), (dict(ratio=True), TypeError),
    (dict(window=0), ValueError), (dict(window=2.0), ValueError), (dict(window=True), ValueError), (dict(window=None), ValueError),
    (dict(pool=(0, 2)), ValueError), (dict(pool=(4, 2.0)), ValueError), (dict(pool=(True, 2)), ValueError),
    (dict(pool=4), TypeError), (dict(pool=(4, 2, 1)), TypeError), (dict(pool=None), TypeError),
]


@pytest.mark.parametrize("kw,exc", _COMMON + _CELLS + [(dict(bogus=1), TypeError), (dict(floor=0.3), TypeError)])
def test_shot_histograms_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    with pytest.raises(exc):
        shot_histograms(kw.pop("frames", _V()), **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON + _CELLS + _RULE + [(dict(bogus=1), TypeError), (dict(step=2), TypeError)])
def test_detect_shots_errors_of_tensors_that_pass_for_device_ones(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    with pytest.raises(exc):
        detect_shots(kw.pop("frames", _V()), **kw)
    assert stub == []


@pytest.mark.parametrize("kw,exc", _COMMON[:3] + _COMMON[4:] + [
    (dict(frames=_z(1, 3, 8, 8)), ValueError),                                                           # one frame
    (dict(levels=0), ValueError), (dict(bogus=1), TypeError),
    (dict(init_flow=_z(4, 2, 8, 8)), TypeError), (dict(init_flow_bw=_z(4, 2, 8, 8)), TypeError), (dict(init_flow=None), TypeError),
    (dict(cuts=[4]), ValueError), (dict(cuts=[-1]), ValueError), (dict(cuts=[0, 0]), ValueError), (dict(cuts=[0.5]), TypeError),
    (dict(cuts="12"), TypeError),
    (dict(out_dtype=torch.float16), TypeError), (dict(consistency=(1.0,)), TypeError), (dict(consistency=(-1.0, 0.5)), ValueError),
    (dict(frames=_z(5, 8, 8, 6), layout="NHWC"), ValueError),            # more than 4 channels: the cuts cannot be detected
])
def test_flow_video_shots_errors_before_any_launch(stub, monkeypatch, kw, exc):
    _on_gpu_stub(monkeypatch)
    kw = dict(kw)
    frames, levels = kw.pop("frames", _V()), kw.pop("levels", 2)
    with pytest.raises(exc):
        flow_video_shots(frames, levels, **kw)
    assert stub == []


_H = lambda **kw: ShotHist(**{**dict(hist=torch.zeros((3, 2, 2, 16), dtype=torch.int32), cell_rows=16, bins=16, size=(32, 128)), **kw})  # noqa: E731


@pytest.mark.parametrize("hist,kw,exc", [
    (None, {}, TypeError), (torch.zeros((3, 2, 2, 16), dtype=torch.int32), {}, TypeError),
    (_H(hist=torch.zeros((3, 2, 2, 16))), {}, TypeError), (_H(hist=np.zeros((3, 2, 2, 16), np.int32)), {}, TypeError),
    (_H(hist=torch.zeros((3, 2, 16), dtype=torch.int32)), {}, ValueError),
    (_H(hist=torch.zeros((3, 0, 2, 16), dtype=torch.int32)), {}, ValueError),
] + [(_H(hist=torch.ones((3, 2, 2, 16), dtype=torch.int32)), kw, exc) for kw, exc in _RULE])
def test_detect_cuts_errors(hist, kw, exc):
    with pytest.raises(exc):
        detect_cuts(hist, **kw)


@pytest.mark.parametrize("kw,exc", [(dict(step=0), ValueError), (dict(step=1.0), ValueError), (dict(step=True), ValueError),
                                    (dict(pool=(0, 1)), ValueError), (dict(pool=3), TypeError), (dict(floor=0.2), TypeError)])
def test_shot_distances_errors(kw, exc):
    with pytest.raises(exc):
        shot_distances(_H(hist=torch.ones((3, 2, 2, 16), dtype=torch.int32)), **kw)
    with pytest.raises(TypeError):
        shot_distances(None)


def test_detect_cuts_on_one_and_two_frames():
    one = detect_cuts(_H(hist=torch.ones((1, 2, 2, 16), dtype=torch.int32)))
    assert (one.cuts, one.flashes, one.gradual, one.ranges) == ([], [], [], [(0, 1)]) and one.distances.shape == (0,)
    h = torch.zeros((2, 1, 1, 16), dtype=torch.int32)
    h[0, 0, 0, 0], h[1, 0, 0, 5] = 64, 64
    two = detect_cuts(_H(hist=h))  # no other pair: the baseline is 0 and the floor alone decides
    assert two.cuts == [0] and two.ranges == [(0, 1), (1, 2)] and two.distances.tolist() == [1.0]


# ---- the C ABI's refusals, through ctypes.  A refused call never dereferences the handle: a zeroed block stands in for one.
def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def _t(dtype=capi.DTYPE_U8, strides=(192, 24, 3, 1), data=0x1000):
    d = capi.PapofTensor()
    d.data, d.dtype = data, dtype
    for i, s in enumerate(strides):
        d.stride[i] = s
    return d


_FAKE = ctypes.create_string_buffer(1 << 20)
_OK = "ok"
_ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731


def c_abi_hist(lib, h, n=4, size=(8, 8, 3), fr=_OK, cell_rows=16, bins=16, out=0x9000):
    fr = _t() if isinstance(fr, str) else fr
    return lib.papof_cell_hist_tensor(h, n, size[0], size[1], size[2], _ref(fr), cell_rows, bins, out, None)


C_ABI_REFUSALS = [
    dict(fr=None), dict(fr=_t(data=0)), dict(out=None), dict(out=0),                                   # NULL
    dict(fr=_t(dtype=3)), dict(fr=_t(dtype=-1)),                                                       # dtypes
    dict(fr=_t(strides=(-192, 24, 3, 1))), dict(fr=_t(strides=(192, -24, 3, 1))),                     # negative strides
    dict(fr=_t(strides=(192, 24, -3, 1))), dict(fr=_t(strides=(192, 24, 3, -1))),
    dict(n=0), dict(n=-3),                                                                             # sizes
    dict(size=(0, 8, 3)), dict(size=(8, 0, 3)), dict(size=(-1, 8, 3)), dict(size=(8, -1, 3)), dict(size=(8, 8, 0)),
    dict(size=(8, 8, 5)), dict(size=(8, 8, -1)),
    dict(cell_rows=0), dict(cell_rows=65), dict(cell_rows=-16),                                        # cells
    dict(bins=0), dict(bins=2), dict(bins=12), dict(bins=17), dict(bins=128), dict(bins=-16),          # bins
]


@pytest.mark.parametrize("kw", C_ABI_REFUSALS)
def test_c_abi_cell_hist_refuses(kw):
    assert c_abi_hist(_lib(), ctypes.cast(_FAKE, ctypes.c_void_p), **kw) == -1


def test_c_abi_cell_hist_without_a_handle():
    assert c_abi_hist(_lib(), None) == -1
