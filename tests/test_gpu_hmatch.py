"""Hierarchical block matching on device tensors (papteam_opticalflow_amd/tensors.py: match_pairs / match_video with
levels > 1, flow_pairs_ld with match_levels -> papof_match_hier_tensor).  The device's displacements and costs must be the
BYTES of the numpy restatement (tests/_hmatch_ref.py): levels 2 .. 4, refine 1 .. 3, patch 1, 3 and 7, strides 1, 2 and 8,
1, 3 and 4 channels, uint8 / float32 / float64 frames with a NaN, NCHW, NHWC, sliced and permuted views, float32 outputs, a
penalty; odd grids at every level, a frame of one top-level cell, tiles that fit exactly; a two-layer frame whose boundary
tiles leave the staged path, against PAPOF_MATCH_STAGED=0; pairs and a sequence; two runs, levels=1 through the new entry
point, a side stream; and the (90, 30) pan that the flat search cannot reach, through flow_pairs_ld."""
import ctypes

import numpy as np
import pytest

from _hmatch_ref import exact_share, hmatch_reference, wide_pan_scene
from _match_ref import epe, texture

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


def _frames(n, H, W, C, dtype, seed, shift=(3, -2)):
    """(a, b): n textured frames (n, H, W, C) of `dtype` and the same texture moved by `shift` with a little noise; floats
    reach beyond 0 .. 1 and hold a NaN"""
    rng = np.random.default_rng(seed)
    pad = max(16, abs(shift[0]), abs(shift[1]))
    a, b = [], []
    for _ in range(n):
        t = texture(rng, H + 2 * pad, W + 2 * pad, C)
        a.append(t[pad:pad + H, pad:pad + W])
        b.append(t[pad - shift[1]:pad - shift[1] + H, pad - shift[0]:pad - shift[0] + W])
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
    from papteam_opticalflow_amd.tensors import match_pairs
    ta, tb = (a, b) if isinstance(a, torch.Tensor) else (_as_layout(a, layout), _as_layout(b, layout))
    na, nb = (t.cpu().numpy() if layout == "NHWC" else t.permute(0, 2, 3, 1).cpu().numpy() for t in (ta, tb))
    got = match_pairs(ta, tb, both=both, layout=layout, out_dtype=out_dtype, **kw)
    np_dtype = _NP[out_dtype or torch.float64]
    fw = hmatch_reference(na, nb, out_dtype=np_dtype, **kw)
    _same(got.disp_fw, fw[0], what + ": disp_fw")
    _same(got.cost_fw, fw[1], what + ": cost_fw")
    if both:
        bw = hmatch_reference(nb, na, out_dtype=np_dtype, **kw)
        _same(got.disp_bw, bw[0], what + ": disp_bw")
        _same(got.cost_bw, bw[1], what + ": cost_bw")
    else:
        assert got.disp_bw is None and got.cost_bw is None
    return got


# (levels, refine, patch, stride, C, dtype, layout, out_dtype, penalty, (H, W), shift): every value of levels, refine, patch,
# stride, C, dtype and layout that the issue names at least once, top strides 2 .. 32, shifts beyond one top-level cell
_SWEEP = [
    (2, 1, 1, 1, 1, torch.uint8, "NHWC", None, 0, (45, 77), (5, -3)),
    (3, 2, 3, 2, 3, torch.float32, "NCHW", None, 0, (45, 77), (13, -6)),
    (4, 3, 7, 2, 4, torch.float64, "NHWC", torch.float32, 0, (34, 51), (-22, 9)),
    (2, 2, 3, 8, 3, torch.uint8, "NCHW", torch.float32, 0, (70, 100), (24, -8)),
    (3, 1, 1, 8, 1, torch.float32, "NHWC", None, 0, (70, 133), (-40, 16)),
    (4, 1, 3, 1, 3, torch.float64, "NCHW", None, 0, (37, 75), (9, 4)),
    (3, 3, 1, 2, 4, torch.uint8, "NHWC", None, 3, (45, 77), (-11, 7)),
    (2, 3, 7, 2, 3, torch.uint8, "NCHW", None, 40, (39, 70), (6, 2)),
    (4, 2, 1, 2, 1, torch.uint8, "NHWC", None, 0, (45, 77), (30, -12)),
]


@pytest.mark.parametrize("levels,refine,patch,stride,C,dtype,layout,out_dtype,penalty,size,shift", _SWEEP)
def test_sweep(levels, refine, patch, stride, C, dtype, layout, out_dtype, penalty, size, shift):
    a, b = _frames(2, size[0], size[1], C, dtype, 7 * levels + refine + patch, shift=shift)
    got = _check_pairs(a, b, layout, "levels %d refine %d patch %d stride %d" % (levels, refine, patch, stride), both=levels == 3,
                       out_dtype=out_dtype, stride=stride, levels=levels, patch=patch, search=6, refine=refine, penalty=penalty)
    assert (got.disp_fw != 0).any()


def test_odd_grids_at_every_level():
    """39 x 79 at stride 2, levels 3: grids 19 x 39, 9 x 19 and 4 x 9 -- every clamped parent, more than one tile; a frame
    of exactly one top-level cell; frames whose level-0 tiles fit exactly"""
    a, b = _frames(1, 39, 79, 3, torch.uint8, 41, shift=(14, -6))
    for refine in (1, 2):
        _check_pairs(a, b, "NHWC", "39 x 79 refine %d" % refine, stride=2, levels=3, patch=3, search=4, refine=refine)
    a, b = _frames(1, 8, 8, 3, torch.uint8, 42, shift=(2, 0))
    _check_pairs(a, b, "NHWC", "one top-level cell", stride=2, levels=3, patch=2, search=3)
    a, b = _frames(1, 11, 9, 1, torch.uint8, 43, shift=(1, 1))
    _check_pairs(a, b, "NHWC", "one top-level cell and a remainder", stride=1, levels=4, patch=1, search=2, refine=3)
    a, b = _frames(1, 16, 64, 3, torch.uint8, 44, shift=(-10, 4))
    for levels in (2, 3):
        _check_pairs(a, b, "NHWC", "exact tiles, levels %d" % levels, stride=2, levels=levels, patch=3, search=5)


def _two_layers(H=96, W=256, seed=51):
    """the upper half moves by (+40, 0), the lower by (-40, 8)"""
    rng = np.random.default_rng(seed)
    pad = 48
    t = texture(rng, H + 2 * pad, W + 2 * pad, 3)
    im1 = t[pad:pad + H, pad:pad + W].copy()
    im2 = t[pad:pad + H, pad - 40:pad - 40 + W].copy()
    im2[H // 2:] = t[pad - 8 + H // 2:pad - 8 + H, pad + 40:pad + 40 + W]
    return im1[None], im2[None]


def test_two_layers_staged_and_global_paths(monkeypatch):
    """the tiles on the boundary see parents that differ by 80 px (20 and 40 cells at levels 1 and 0: beyond the staged
    window's spread) and read B through global addresses; the others stage it.  PAPOF_MATCH_STAGED=0 sends every tile down
    the global path: equal bytes, and both equal to the restatement."""
    from papteam_opticalflow_amd.tensors import match_pairs
    a, b = _two_layers()
    kw = dict(stride=2, levels=3, patch=3, search=8, refine=1)
    monkeypatch.delenv("PAPOF_MATCH_STAGED", raising=False)
    got = _check_pairs(a, b, "NHWC", "two layers", **kw)
    d = got.disp_fw[0].cpu().numpy()
    assert (d[:, 8:16, 30:90] == np.array([40.0, 0.0])[:, None, None]).mean() > 0.95
    assert (d[:, 34:42, 40:100] == np.array([-40.0, 8.0])[:, None, None]).mean() > 0.95
    monkeypatch.setenv("PAPOF_MATCH_STAGED", "0")
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    plain = match_pairs(ta, tb, layout="NHWC", **kw)
    for x, y, name in zip(plain, got, got._fields):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), name
    for r in (2, 3):  # the wider refinements under the switch too
        _check_pairs(a[:, :40, :90], b[:, :40, :90], "NHWC", "global path, refine %d" % r, stride=2, levels=2, patch=1, search=4,
                     refine=r)


def test_views_are_read_in_place():
    rng = np.random.default_rng(8)
    big = torch.from_numpy(texture(rng, 2 * 50 + 3, 2 * 90, 4)).cuda()[None].repeat(4, 1, 1, 1)
    big[1::2] = torch.roll(big[1::2], (6, -10), (1, 2))
    a = big[::2, 2:102:2, ::2, 1:]   # every other item, rows and columns, channels cut: (2, 50, 90, 3)
    b = big[1::2, 2:102:2, ::2, 1:]
    assert not a.is_contiguous()
    _check_pairs(a, b, "NHWC", "sliced NHWC", stride=2, levels=2, patch=3, search=4)
    ap, bp = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)  # NCHW views of channels-last memory
    assert not ap.is_contiguous()
    _check_pairs(ap, bp, "NCHW", "permuted NCHW", stride=1, levels=3, patch=2, search=4, refine=2)


@pytest.mark.parametrize("both", [True, False])
def test_sequence(both):
    from papteam_opticalflow_amd.tensors import match_pairs, match_video
    rng = np.random.default_rng(9)
    t = texture(rng, 120, 200, 3)
    v = np.stack([t[8 + 6 * k:8 + 6 * k + 57, 10 + 14 * k:10 + 14 * k + 91] for k in range(4)])
    tv = torch.from_numpy(v).cuda()
    kw = dict(stride=2, levels=3, patch=3, search=4, refine=1)
    got = match_video(tv, both=both, layout="NHWC", **kw)
    fw = hmatch_reference(v[:-1], v[1:], **kw)
    _same(got.disp_fw, fw[0], "sequence: disp_fw")
    _same(got.cost_fw, fw[1], "sequence: cost_fw")
    assert tuple(got.disp_fw.shape) == (3, 2, 28, 45)
    if both:
        bw = hmatch_reference(v[1:], v[:-1], **kw)
        _same(got.disp_bw, bw[0], "sequence: disp_bw")
        _same(got.cost_bw, bw[1], "sequence: cost_bw")
    else:
        assert got.disp_bw is None
    pairs = match_pairs(tv[:-1], tv[1:], both=both, layout="NHWC", **kw)
    assert torch.equal(pairs.disp_fw, got.disp_fw) and torch.equal(pairs.cost_fw, got.cost_fw)
    mid = got.disp_fw[:, :, 8:-8, 10:-10]  # the texture moved by (-14, -6) pixels per frame
    assert set(mid[:, 0].unique().tolist()) == {-14.0} and set(mid[:, 1].unique().tolist()) == {-6.0}


def test_levels_1_through_the_new_entry_point_is_match_pairs():
    """papof_match_hier_tensor with levels == 1, on papof_match_hier_workspace's bytes: match_pairs' bytes"""
    from papteam_opticalflow_amd import tensors
    a, b = _frames(2, 45, 77, 3, torch.uint8, 60)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = tensors.match_pairs(ta, tb, stride=2, patch=3, search=8, layout="NHWC")
    disp = torch.full((4, 2, 22, 38), -1.0, dtype=torch.float64, device="cuda")
    cost = torch.full((4, 22, 38), -1.0, dtype=torch.float64, device="cuda")
    d_in = [tensors._struct(t, *tensors.descriptor(t, "NHWC")[1:]) for t in (ta, tb)]
    d_disp = tensors._flow_struct(disp, tensors.capi.DTYPE_F64)
    d_cost = tensors._struct(cost, (cost.stride(0), cost.stride(1), cost.stride(2), 0), tensors.capi.DTYPE_F64)
    tensors._launch(ta.device, "papof_match_hier_tensor", 2, 0, ctypes.byref(d_in[0]), ctypes.byref(d_in[1]), 45, 77, 3, 2, 1, 3, 8,
                    2, 0, 1, ctypes.byref(d_disp), ctypes.byref(d_cost),
                    workspace=("papof_match_hier_workspace", (2, 0, 45, 77, 2, 1), "refused"))
    assert torch.equal(disp[:2].view(torch.int64), want.disp_fw.view(torch.int64))
    assert torch.equal(disp[2:].view(torch.int64), want.disp_bw.view(torch.int64))
    assert torch.equal(cost[:2].view(torch.int64), want.cost_fw.view(torch.int64))
    assert torch.equal(cost[2:].view(torch.int64), want.cost_bw.view(torch.int64))
    again = tensors.match_pairs(ta, tb, stride=2, patch=3, search=8, layout="NHWC", levels=1, refine=3)
    assert torch.equal(again.disp_fw.view(torch.int64), want.disp_fw.view(torch.int64))


def test_two_runs_and_a_side_stream():
    """the same bytes twice; inputs written on a side stream behind a long sleep and matched under that stream with no
    synchronisation: every kernel must follow the writes"""
    import time
    from papteam_opticalflow_amd.tensors import match_init, match_pairs
    a, b = _frames(2, 135, 240, 3, torch.uint8, 30, shift=(52, -24))
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    kw = dict(layout="NHWC", levels=3, search=8)
    first = match_pairs(ta, tb, **kw)
    again = match_pairs(ta, tb, **kw)
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    assert exact_share(first.disp_fw[0].cpu().numpy(), (52, -24), 2, (135, 240)) > 0.95
    want = [t.cpu().numpy() for t in first]
    want_init = [t.cpu().numpy() for t in match_init(*first, (135, 240))]
    da, db = torch.zeros_like(ta), torch.zeros_like(tb)
    side = torch.cuda.Stream(priority=-1)
    with torch.cuda.stream(side):  # the side stream's allocator blocks exist
        warm = match_init(*match_pairs(da, db, **kw), (135, 240))
    del warm
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the rate of the sleep kernel's clock
        t0 = time.perf_counter()
        torch.cuda._sleep(50_000_000)
        side.synchronize()
        per_cycle = (time.perf_counter() - t0) / 50_000_000
    with torch.cuda.stream(side):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(0.3 / per_cycle))  # ~0.3 s: far longer than the enqueueing of the calls
        da.copy_(ta)
        db.copy_(tb)
        got = match_pairs(da, db, **kw)
        init = match_init(*got, (135, 240))
        took = time.perf_counter() - t0
    side.synchronize()
    assert took < 0.25, "the calls waited for the stream: %.3f s" % took
    for g, w, name in zip(got, want, got._fields):
        _same(g, w, "side stream: " + name)
    for g, w, name in zip(init, want_init, init._fields):
        _same(g, w, "side stream: " + name)


def test_flow_pairs_ld_reaches_the_90_30_pan():
    """the (90, 30) pan of tests/test_hmatch_cpu.py: the flat matcher's reach is 40 px; with match_levels=3 flow_pairs_ld
    ends below 0.5 px on the pixels that stay in view, and is byte-equal to flow_pairs_fb started from match_init of
    match_pairs(levels=3)"""
    from papteam_opticalflow_amd.tensors import flow_pairs_fb, flow_pairs_ld, match_init, match_pairs
    im1, im2, truth, interior = wide_pan_scene(3, (90, 30))
    t1, t2 = torch.from_numpy(im1[None]).cuda(), torch.from_numpy(im2[None]).cuda()
    ld = flow_pairs_ld(t1, t2, 2, layout="NHWC", match_levels=3)
    f = ld.flow_fw[0].cpu().numpy()
    e = epe(f[0], f[1], truth, interior)
    flat = flow_pairs_ld(t1, t2, 2, layout="NHWC").flow_fw[0].cpu().numpy()
    print("pan (90, 30): flow_pairs_ld match_levels 3: interior EPE %.4f; match_levels 1: %.3f" % (
        e, epe(flat[0], flat[1], truth, interior)))
    assert e < 0.5
    init = match_init(*match_pairs(t1, t2, layout="NHWC", levels=3), im1.shape[:2])
    ref = flow_pairs_fb(t1, t2, 2, layout="NHWC", init_flow=init.init_fw, init_flow_bw=init.init_bw)
    for name in ("flow_fw", "flow_bw", "warpI2_fw", "warpI2_bw"):
        assert torch.equal(getattr(ld, name).view(torch.int64), getattr(ref, name).view(torch.int64)), name
    assert torch.equal(ld.occlusion, ref.occlusion)
