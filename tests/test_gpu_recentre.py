"""The re-centred block search on device tensors (papteam_opticalflow_amd/tensors.py: match_pairs / match_video with
recentre, flow_pairs_ld with match_recentre -> papof_match_recentre_tensor).  The device's displacements and costs must be
the BYTES of the numpy restatement (tests/_recentre_ref.py) on the shapes where it can go wrong -- 16 x 40 and 33 x 70 at
stride 1 (clipped tiles on one axis and on both), 64 x 96 at stride 4, 135 x 240 at stride 2 with 3 levels (the scenes of a
small object against a large pan) -- with windows 1, 20 and 32, patches 1, 3 and 7, refinements 1 and 3, 1, 3 and 4 channels,
uint8 / float32 / float64 frames with a NaN, sliced and permuted views, one and both directions, a sequence, penalties 0 and
5; two runs and an item alone or in a batch; the two properties that follow from the rule, on the device's outputs;
recentre=None and levels=1 unchanged; and flow_pairs_ld with match_recentre against its parts chained by hand."""
import numpy as np
import pytest

from _hmatch_ref import hmatch_reference
from _match_ref import epe, match_reference, object_scene, texture
from _recentre_ref import SCENES, cells_of, key_of, pan_object_scene, recentre_reference, shares, tile_origins

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_NP = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


def _same(got, want, what):
    """a device tensor and an array, byte for byte"""
    g, w = np.ascontiguousarray(got.cpu().numpy()), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = g.view(np.uint8) != w.view(np.uint8)
    if bad.any():
        i = tuple(int(k[0]) for k in np.nonzero(g != w)) if (g != w).any() else None
        raise AssertionError("%s: %d of %d bytes differ; first element at %s: %r against %r" % (
            what, int(bad.sum()), bad.size, i, g[i] if i else None, w[i] if i else None))


def _frames(n, H, W, C, dtype, seed, shift, shift2):
    """(a, b): n textured frames (n, H, W, C) of `dtype`; b is the texture moved by `shift`, its middle third in both axes
    by `shift2` (two motions: tiles with an origin of either, and cells whose d_h lies outside their tile's window), with a
    little noise; floats reach beyond 0 .. 1 and hold a NaN"""
    rng = np.random.default_rng(seed)
    pad = 2 + max(abs(v) for v in shift + shift2)
    a, b = [], []
    for _ in range(n):
        t = texture(rng, H + 2 * pad, W + 2 * pad, C)
        a.append(t[pad:pad + H, pad:pad + W])
        f = t[pad - shift[1]:pad - shift[1] + H, pad - shift[0]:pad - shift[0] + W].copy()
        g = t[pad - shift2[1]:pad - shift2[1] + H, pad - shift2[0]:pad - shift2[0] + W]
        f[H // 3:2 * H // 3, W // 3:2 * W // 3] = g[H // 3:2 * H // 3, W // 3:2 * W // 3]
        b.append(f)
    a, b = np.stack(a), np.stack(b)
    b = np.clip(b.astype(np.int64) + rng.integers(-2, 3, b.shape), 0, 255).astype(np.uint8)
    if dtype == torch.uint8:
        return a, b
    a, b = (a / 255.0 * 1.2 - 0.1).astype(_NP[dtype]), (b / 255.0 * 1.2 - 0.1).astype(_NP[dtype])
    a[0, H // 2, W // 2, 0] = np.nan
    return a, b


def _as_layout(a, layout):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "NHWC" else t.permute(0, 3, 1, 2).contiguous()


def _check_pairs(a, b, layout, what, both=True, out_dtype=None, **kw):
    """match_pairs(recentre=window) against the restatement; kw holds `window` for the restatement's name of it"""
    from papteam_opticalflow_amd.tensors import match_pairs
    ta, tb = (a, b) if isinstance(a, torch.Tensor) else (_as_layout(a, layout), _as_layout(b, layout))
    na, nb = (t.cpu().numpy() if layout == "NHWC" else t.permute(0, 2, 3, 1).cpu().numpy() for t in (ta, tb))
    dev_kw = dict(kw)
    dev_kw["recentre"] = dev_kw.pop("window")
    got = match_pairs(ta, tb, both=both, layout=layout, out_dtype=out_dtype, **dev_kw)
    np_dtype = _NP[out_dtype or torch.float64]
    fw = recentre_reference(na, nb, out_dtype=np_dtype, **kw)
    _same(got.disp_fw, fw[0], what + ": disp_fw")
    _same(got.cost_fw, fw[1], what + ": cost_fw")
    if both:
        bw = recentre_reference(nb, na, out_dtype=np_dtype, **kw)
        _same(got.disp_bw, bw[0], what + ": disp_bw")
        _same(got.cost_bw, bw[1], what + ": cost_bw")
    else:
        assert got.disp_bw is None and got.cost_bw is None
    return got


# ((H, W), stride, levels, window, patch, refine, C, dtype, layout, out_dtype, both, penalty, search, shift, shift2): every
# value of window, patch, refine, C, dtype, both and penalty at least once on the three small shapes (patch 7 on one pair,
# the others on two: the restatement of the hierarchy is slow on large patches)
_SWEEP = [
    ((16, 40), 1, 2, 1, 1, 1, 1, torch.uint8, "NHWC", None, True, 0, 4, (5, -3), (-2, 1)),
    ((16, 40), 1, 2, 32, 7, 3, 4, torch.float64, "NCHW", torch.float32, False, 5, 4, (-9, 2), (3, 0)),
    ((16, 40), 1, 2, 20, 3, 1, 3, torch.uint8, "NCHW", None, True, 5, 3, (6, 1), (-6, -1)),
    ((33, 70), 1, 2, 20, 3, 1, 3, torch.float32, "NHWC", None, True, 0, 6, (13, -6), (-4, 2)),
    ((33, 70), 1, 2, 1, 7, 1, 3, torch.uint8, "NCHW", None, False, 5, 5, (-8, 5), (7, -2)),
    ((33, 70), 1, 2, 32, 1, 3, 1, torch.float64, "NHWC", None, False, 0, 6, (10, 4), (-12, 0)),
    ((64, 96), 4, 2, 32, 3, 1, 3, torch.uint8, "NHWC", None, True, 0, 4, (24, -8), (-8, 4)),
    ((64, 96), 4, 2, 20, 1, 3, 4, torch.float32, "NCHW", torch.float32, False, 5, 3, (-16, 12), (4, 0)),
    ((64, 96), 4, 2, 1, 7, 1, 1, torch.uint8, "NHWC", None, True, 0, 4, (20, 8), (0, -12)),
]


@pytest.mark.parametrize("size,stride,levels,window,patch,refine,C,dtype,layout,out_dtype,both,penalty,search,shift,shift2", _SWEEP)
def test_sweep(size, stride, levels, window, patch, refine, C, dtype, layout, out_dtype, both, penalty, search, shift, shift2):
    a, b = _frames(1 if patch == 7 else 2, size[0], size[1], C, dtype, 11 * window + patch + refine, shift, shift2)
    got = _check_pairs(a, b, layout, "%r stride %d window %d patch %d refine %d" % (size, stride, window, patch, refine), both=both,
                       out_dtype=out_dtype, stride=stride, levels=levels, patch=patch, search=search, refine=refine, window=window,
                       penalty=penalty)
    assert (got.disp_fw != 0).any()


@pytest.fixture(scope="module", params=range(len(SCENES)))
def scene(request):
    """a scene of the table with its forward fields from the device (flat, 3 levels, re-centred) and from the restatement"""
    from papteam_opticalflow_amd.tensors import match_pairs
    pan, rel, origin = SCENES[request.param]
    im1, im2, background, inside = pan_object_scene(4, pan, rel, origin)
    t1, t2 = torch.from_numpy(im1[None]).cuda(), torch.from_numpy(im2[None]).cuda()
    fields = {name: match_pairs(t1, t2, layout="NHWC", both=False, **kw) for name, kw in (
        ("flat", dict()), ("3 levels", dict(levels=3)), ("re-centred", dict(levels=3, recentre=20)))}
    want = recentre_reference(im1[None], im2[None], stride=2, levels=3, patch=3, search=20, refine=1, window=20)
    return dict(pan=pan, rel=rel, frames=(im1, im2, t1, t2), masks=(background, inside), fields=fields, want=want)


def test_the_scenes_bytes_and_shares(scene):
    """135 x 240, stride 2, 3 levels, window 20: the restatement's bytes, and the shares of tests/test_recentre_cpu.py"""
    got = scene["fields"]["re-centred"]
    _same(got.disp_fw, scene["want"][0], "scene: disp_fw")
    _same(got.cost_fw, scene["want"][1], "scene: cost_fw")
    pan, rel = scene["pan"], scene["rel"]
    moved = (pan[0] + rel[0], pan[1] + rel[1])
    s = {k: shares(f.disp_fw[0].cpu().numpy(), pan, moved, *scene["masks"], 2) for k, f in scene["fields"].items()}
    print("pan %r, rel %r: %s" % (pan, rel, "   ".join("%s %.4f / %.4f" % (k, *v) for k, v in s.items())))
    assert s["3 levels"][1] <= 0.1 and s["re-centred"][0] >= 0.95 and s["re-centred"][1] >= 0.9


def test_property_a_on_the_device(scene):
    """every cell's key is <= the key of the hierarchical call's result, and smaller on the object"""
    rec, hier = scene["fields"]["re-centred"], scene["fields"]["3 levels"]
    k = key_of(rec.disp_fw.cpu().numpy(), rec.cost_fw.cpu().numpy(), 2)
    kh = key_of(hier.disp_fw.cpu().numpy(), hier.cost_fw.cpu().numpy(), 2)
    assert (k <= kh).all()
    obj = cells_of(scene["masks"][1], 2, 67, 120)
    assert (k[0][obj] < kh[0][obj]).all()


def test_property_b_on_the_device():
    """the scene of tests/test_recentre_cpu.py (a static background, an object within the flat reach), window == search: on
    the tiles whose origin -- taken from the device's own hierarchical field -- is (0, 0), the cells whose d_h lies within
    the window hold match_pairs' flat result at the finest stride"""
    from papteam_opticalflow_amd.tensors import match_pairs
    im1, im2, _, interior = object_scene(2, (14, -8), H=72, W=136, size=16, origin=(50, 30), background=(0, 0))
    t1, t2 = torch.from_numpy(im1[None]).cuda(), torch.from_numpy(im2[None]).cuda()
    kw = dict(layout="NHWC", both=False, stride=2, patch=2, search=10)
    flat = match_pairs(t1, t2, **kw)
    hier = match_pairs(t1, t2, levels=2, **kw)
    rec = match_pairs(t1, t2, levels=2, recentre=10, **kw)
    dh = hier.disp_fw[0].cpu().numpy().astype(np.int64) // 2
    org = tile_origins(dh)
    zero = np.repeat(np.repeat((org == 0).all(axis=0), 8, axis=0), 32, axis=1)[:36, :68]
    within = torch.from_numpy(zero & (np.abs(dh) <= 10).all(axis=0)).cuda()
    assert zero.mean() > 0.5 and int(within.sum()) > 0.5 * zero.sum()
    assert torch.equal(rec.disp_fw[0][:, within].view(torch.int64), flat.disp_fw[0][:, within].view(torch.int64))
    assert torch.equal(rec.cost_fw[0][within].view(torch.int64), flat.cost_fw[0][within].view(torch.int64))
    obj = torch.from_numpy(cells_of(interior, 2, 36, 68)).cuda()
    assert bool((within & obj).any()) and bool(((rec.disp_fw[0, 0] == 14) & (rec.disp_fw[0, 1] == -8))[obj].all())


def test_views_are_read_in_place():
    rng = np.random.default_rng(8)
    big = torch.from_numpy(texture(rng, 2 * 33 + 3, 2 * 70, 4)).cuda()[None].repeat(4, 1, 1, 1)
    big[1::2] = torch.roll(big[1::2], (4, -8), (1, 2))
    a = big[::2, 2:68:2, ::2, 1:]   # every other item, row and column, the channels cut: (2, 33, 70, 3)
    b = big[1::2, 2:68:2, ::2, 1:]
    assert not a.is_contiguous() and tuple(a.shape) == (2, 33, 70, 3)
    _check_pairs(a, b, "NHWC", "sliced NHWC", stride=1, levels=2, patch=3, search=4, refine=1, window=20, penalty=0)
    ap, bp = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)  # NCHW views of channels-last memory
    assert not ap.is_contiguous()
    _check_pairs(ap, bp, "NCHW", "permuted NCHW", stride=1, levels=2, patch=1, search=4, refine=3, window=1, penalty=5)


@pytest.mark.parametrize("both", [True, False])
def test_sequence(both):
    from papteam_opticalflow_amd.tensors import match_pairs, match_video
    rng = np.random.default_rng(9)
    t = texture(rng, 80, 140, 3)
    v = np.stack([t[6 + 4 * k:6 + 4 * k + 33, 8 + 9 * k:8 + 9 * k + 70] for k in range(4)])
    tv = torch.from_numpy(v).cuda()
    kw = dict(stride=1, levels=2, patch=3, search=5, refine=1)
    got = match_video(tv, both=both, layout="NHWC", recentre=20, **kw)
    fw = recentre_reference(v[:-1], v[1:], window=20, **kw)
    _same(got.disp_fw, fw[0], "sequence: disp_fw")
    _same(got.cost_fw, fw[1], "sequence: cost_fw")
    assert tuple(got.disp_fw.shape) == (3, 2, 33, 70)
    if both:
        bw = recentre_reference(v[1:], v[:-1], window=20, **kw)
        _same(got.disp_bw, bw[0], "sequence: disp_bw")
        _same(got.cost_bw, bw[1], "sequence: cost_bw")
    else:
        assert got.disp_bw is None
    pairs = match_pairs(tv[:-1], tv[1:], both=both, layout="NHWC", recentre=20, **kw)
    assert torch.equal(pairs.disp_fw, got.disp_fw) and torch.equal(pairs.cost_fw, got.cost_fw)
    mid = got.disp_fw[:, :, 8:-8, 12:-12]  # the texture moved by (-9, -4) per frame
    assert set(mid[:, 0].unique().tolist()) == {-9.0} and set(mid[:, 1].unique().tolist()) == {-4.0}


def test_two_runs_and_an_item_alone_or_in_a_batch():
    from papteam_opticalflow_amd.tensors import match_pairs
    a, b = _frames(3, 33, 70, 3, torch.uint8, 77, (13, -6), (-4, 2))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kw = dict(layout="NHWC", stride=1, levels=2, patch=3, search=6, recentre=20)
    first = match_pairs(ta, tb, **kw)
    again = match_pairs(ta, tb, **kw)
    for x, y, name in zip(first, again, first._fields):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), name
    for i in range(3):
        alone = match_pairs(ta[i:i + 1], tb[i:i + 1], **kw)
        for x, y, name in zip(alone, first, first._fields):
            assert torch.equal(x[0].view(torch.int64), y[i].view(torch.int64)), (i, name)


def test_none_and_levels_1_return_the_bytes_of_before():
    """recentre=None: the flat call with levels=1 and the hierarchical call with more, held to their restatements"""
    from papteam_opticalflow_amd.tensors import match_pairs
    a, b = _frames(2, 33, 70, 3, torch.uint8, 60, (5, -3), (-2, 1))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for kw, ref in ((dict(), match_reference), (dict(levels=1, refine=3), match_reference), (dict(levels=2), hmatch_reference)):
        got = match_pairs(ta, tb, layout="NHWC", stride=1, patch=3, search=6, recentre=None, **kw)
        ref_kw = dict(levels=2) if kw.get("levels") == 2 else {}
        for g, (x, y) in ((0, (a, b)), (1, (b, a))):
            want = ref(x, y, stride=1, patch=3, search=6, **ref_kw)
            _same((got.disp_fw, got.disp_bw)[g], want[0], "recentre=None %r: disp %d" % (kw, g))
            _same((got.cost_fw, got.cost_bw)[g], want[1], "recentre=None %r: cost %d" % (kw, g))


def test_flow_pairs_ld_with_match_recentre():
    """the first scene through flow_pairs_ld(match_levels=3, match_recentre=20): the bytes of match_pairs(levels=3,
    recentre=20) -> match_init -> flow_pairs_fb chained by hand; and the mean endpoint error on the object's interior (4 px
    inside it) beside the match_levels=3-only call's, which starts the solver about 37 px off there.
    Measured: 0.0008 px against 35.49 px."""
    from papteam_opticalflow_amd.tensors import flow_pairs_fb, flow_pairs_ld, match_init, match_pairs
    pan, rel, origin = SCENES[0]
    im1, im2, _, inside = pan_object_scene(4, pan, rel, origin)
    truth = np.zeros(im1.shape[:2] + (2,))
    truth[..., 0], truth[..., 1] = pan[0] + rel[0], pan[1] + rel[1]
    t1, t2 = torch.from_numpy(im1[None]).cuda(), torch.from_numpy(im2[None]).cuda()
    ld = flow_pairs_ld(t1, t2, 2, layout="NHWC", match_levels=3, match_recentre=20)
    init = match_init(*match_pairs(t1, t2, layout="NHWC", levels=3, recentre=20), im1.shape[:2])
    ref = flow_pairs_fb(t1, t2, 2, layout="NHWC", init_flow=init.init_fw, init_flow_bw=init.init_bw)
    for name in ("flow_fw", "flow_bw", "warpI2_fw", "warpI2_bw"):
        assert torch.equal(getattr(ld, name).view(torch.int64), getattr(ref, name).view(torch.int64)), name
    assert torch.equal(ld.occlusion, ref.occlusion)
    f = ld.flow_fw[0].cpu().numpy()
    g = flow_pairs_ld(t1, t2, 2, layout="NHWC", match_levels=3).flow_fw[0].cpu().numpy()
    e, e3 = epe(f[0], f[1], truth, inside), epe(g[0], g[1], truth, inside)
    print("object interior EPE: match_levels 3 + match_recentre 20: %.4f px; match_levels 3 alone: %.4f px" % (e, e3))
    assert e < 0.5 * e3
