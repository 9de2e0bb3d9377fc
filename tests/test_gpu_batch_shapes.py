"""The batched launch chain at the shapes where its plan changes (tests/_batch_shapes.py: the table, and why each case is in
it).  Every case goes through Papof.flow_batch (host frames), through tensors.flow_video / flow_pairs and, where its class
says so, through flow_video_fb / flow_pairs_fb and init_flow=.  Three things are held, per pair:
  1. the BITS of the single call on the same handle on that pair (integer views: the sign of a zero counts) -- with an
     initial flow, of the same tensor call on that pair alone; backward pairs: the single call on the exchanged frames, and the
     mask is the check's rule (tests/test_fb_cpu.py: fb_reference) on the two single-call flows;
  2. the oracle itself within 1e-9 (the bound tests/test_gpu_fuzz_small.py holds the single call to), and its bytes where the
     single call gives them -- a defect that chain and single call share does not pass 1;
  3. the route: papof_batch_stats before and after says that the chain ran, with exactly the case's solver pairs, no pair outside
     it and no re-run -- or exactly the split, the single calls and the re-runs the case is there for.  Without it "the batch
     equals the single calls" passes when the chain silently never ran.
One handle (the module's own, tensors._handle) serves every route and the reference single calls."""
import time

import numpy as np
import pytest

import _batch_shapes as bs
from _libs import ORACLE_BOUND
from test_fb_cpu import fb_reference
from test_gpu_fb import _same_mask
from test_gpu_tensors import _same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_report = []  # one line per case: what papof_batch_stats added on each route
_started = []  # when the module's handle was made


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    _started.append(time.perf_counter())
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


_refs = {}  # single calls and oracle results, once per (video, schedule, frame pair): shared by the cases of one video


def _video_key(c):
    return (c.H, c.W, c.C, c.origin, c.dtype, c.levels, tuple(sorted(c.params.items())))


def _frame(c, i, channels=None):
    return bs.as_dtype(bs.frame_u8(c, i, channels), c.dtype)


def _single(gpu, c, a, b):
    """(vx, vy, warpI2) of the single call on distinct frames a, b of the case's video"""
    from papteam_opticalflow_amd import default_params
    key = ("single", _video_key(c), a, b)
    if key not in _refs:
        P = default_params(**c.params)
        fa, fb = _frame(c, a), _frame(c, b)
        if c.dtype == "u8":
            r = gpu.coarse2fine_flow_u8(fa, fb, c.levels, P)[:3]
        else:
            r = gpu.coarse2fine_flow(fa.astype(np.float64), fb.astype(np.float64), c.levels, P)[:3]
        _refs[key] = tuple(np.array(x) for x in r)
    return _refs[key]


def _oracle(oracle, c, a, b):
    key = ("oracle", _video_key(c), a, b)
    if key not in _refs:
        p = oracle.default_params()
        for k, v in c.params.items():
            setattr(p, k, v)
        fa, fb = (bs.frame_u8(c, i) / 255.0 if c.dtype == "u8" else _frame(c, i).astype(np.float64) for i in (a, b))
        _refs[key] = oracle.coarse2fine_flow(fa, fb, c.levels, p)[:3]
    return _refs[key]


def _triples(flow, warp, layout):
    """[(vx, vy, warpI2 HWC)] numpy arrays of a tensor call's outputs"""
    w = warp.permute(0, 2, 3, 1) if layout == "NCHW" else warp
    f, w = flow.cpu().numpy(), w.cpu().numpy()
    return [(f[i, 0], f[i, 1], w[i]) for i in range(f.shape[0])]


def _check(got, singles, oracles, what, out32=False):
    """assertions 1 and 2 on [(vx, vy, warpI2)] of one route"""
    assert len(got) == len(singles), (what, len(got), len(singles))
    worst = 0.0
    for i, (g3, s3) in enumerate(zip(got, singles)):
        for name, g, s in zip(("vx", "vy", "warpI2"), g3, s3):
            _same_bits(g, s.astype(np.float32) if out32 else s, "%s pair %d %s against the single call" % (what, i, name))
        if oracles is None or out32:  # (float32 outputs: the rounded single call, which is held to the oracle below)
            continue
        for name, g, s, o in zip(("vx", "vy", "warpI2"), g3, s3, oracles[i]):
            d = float(np.abs(g - o).max())
            worst = max(worst, d)
            assert d <= ORACLE_BOUND, "%s pair %d %s against the oracle: max-abs %.3e" % (what, i, name, d)
            if s.tobytes() == np.ascontiguousarray(o).tobytes():
                assert np.ascontiguousarray(g).tobytes() == s.tobytes(), "%s pair %d %s: the single call gives the oracle's bytes" % (what, i, name)
    return worst


def _delta(gpu, before):
    after = gpu.batch_stats()
    return {k: after[k] - before[k] for k in after}


def _check_route(c, got, fb, what):
    """assertion 3: exactly the chains, solver pairs, single calls and re-runs the restatement expects"""
    want = bs.expected_stats(c, fb)
    assert got == want, "%s: papof_batch_stats added %s, the case expects %s" % (what, got, want)
    per = 2 if fb else 1  # solver pairs per frame pair
    assert got["chain_pairs"] + per * got["singles"] == per * c.B, "every frame pair once: in a chain or as a single call"
    if c.chain:
        assert got["chains"] >= 1
        if c.cls != "duplicates":
            assert got["reruns"] == 0
        if c.cls not in ("remainders", "duplicates"):
            assert got["singles"] == 0 and got["chain_pairs"] == per * c.B
    else:
        assert got["chains"] == 0 and got["singles"] == c.B


@pytest.mark.parametrize("name", [c.name for c in bs.CASES])
def test_case(gpu, oracle, monkeypatch, name):
    from papteam_opticalflow_amd import capi, default_params
    from papteam_opticalflow_amd.tensors import flow_pairs, flow_pairs_fb, flow_video, flow_video_fb
    c = bs.BY_NAME[name]
    t0 = time.perf_counter()
    print("%s [%s]: %dx%dx%d L%d %s B=%d %s %s max=%s dup=%s bands=%d slots=%d" % (
        name, c.cls, c.H, c.W, c.C, c.levels, c.params, c.B, "sequence" if c.sequence else "pairs", c.dtype, c.batch_max, c.dup,
        bs.bands(c), bs.slots(c)), flush=True)
    assert gpu.lap_guard_stats()["guard_on"]
    if c.cls == "level 0 tiny / just not":  # the sides the table claims, by the library's own predicate
        sizes = bs.level_sizes(c.H, c.W, 0.75, c.levels)
        assert (capi.sor_tiny_shape(c.H, c.W) != (0, 0)) == (c.W == 96), (c.H, c.W, capi.sor_tiny_shape(c.H, c.W))
        assert all(capi.sor_tiny_shape(h, w) != (0, 0) for h, w in sizes[1:]), sizes
        assert (c.H * c.W <= bs.TINY_MAX_CELLS) == (c.W <= 128)
    P = default_params(**c.params)
    ids, pairs = bs.frame_ids(c), bs.pair_ids(c)
    singles = [_single(gpu, c, a, b) for a, b in pairs]
    oracles = [_oracle(oracle, c, a, b) for a, b in pairs]
    worst = _check(singles, singles, oracles, name + " single call")  # the single call itself against the oracle
    for p in c.dup:
        assert not singles[p][0].any() and not singles[p][1].any(), "a repeated frame: zero flow"
    if c.batch_max is not None:
        monkeypatch.setenv("PAPOF_BATCH_MAX", str(c.batch_max))
    routes = {}

    # ---- host frames through Papof.flow_batch
    before = gpu.batch_stats()
    out, _ = gpu.flow_batch([_frame(c, i) for i in ids], c.levels, P, sequence=c.sequence)
    routes["host"] = _delta(gpu, before)
    worst = max(worst, _check([tuple(np.array(x) for x in o) for o in out], singles, oracles, name + " flow_batch"))
    _check_route(c, routes["host"], False, name + " flow_batch")

    # ---- device tensors through flow_video / flow_pairs
    layout = "NCHW" if c.view == "nchw" else "NHWC"
    if c.view == "gray":  # a channel-sliced view of three-channel storage
        t = torch.from_numpy(np.stack([_frame(c, i, 3) for i in ids])).cuda()[..., 1:2]
        assert not t.is_contiguous()
    else:
        t = torch.from_numpy(np.stack([_frame(c, i) for i in ids])).cuda()
        if c.view == "nchw":  # an NCHW view of NHWC storage
            t = t.permute(0, 3, 1, 2)
            assert not t.is_contiguous()
    im1, im2 = (t[:-1], t[1:]) if c.sequence else (t[0::2], t[1::2])
    kw = dict(layout=layout, **c.params)
    if c.out32:
        kw["out_dtype"] = torch.float32
    init = init_bw = None
    want_fw, want_bw = singles, None
    if c.init:  # the same tensor call on every pair alone: a batch of one runs the single route with the init
        full = torch.from_numpy(bs.smooth_init(c.B, c.H, c.W, per_pair=c.init == "per pair")).cuda()
        full_bw = -0.5 * full.flip(3)
        init, init_bw = (full, full_bw) if c.init == "per pair" else (full[0], full_bw[0])
        assert init.dtype == torch.float32
        alone = lambda x, y, ini: _triples(*flow_pairs(x, y, c.levels, init_flow=ini, **kw)[:2], layout)[0]  # noqa: E731
        want_fw = [alone(im1[i:i + 1], im2[i:i + 1], full[i:i + 1]) for i in range(c.B)]
        want_bw = [alone(im2[i:i + 1], im1[i:i + 1], full_bw[i:i + 1]) for i in range(c.B)]
    before = gpu.batch_stats()
    flow, warp, _ = (flow_video(t, c.levels, init_flow=init, **kw) if c.sequence else
                     flow_pairs(im1, im2, c.levels, init_flow=init, **kw))
    routes["tensor"] = _delta(gpu, before)
    assert flow.dtype == (torch.float32 if c.out32 else torch.float64)
    worst = max(worst, _check(_triples(flow, warp, layout), want_fw, None if c.init else oracles, name + " tensors", c.out32))
    _check_route(c, routes["tensor"], False, name + " tensors")

    # ---- both directions
    if c.fb:
        if want_bw is None:
            want_bw = [_single(gpu, c, b, a) for a, b in pairs]
        before = gpu.batch_stats()
        res = (flow_video_fb(t, c.levels, init_flow=init, init_flow_bw=init_bw, **kw) if c.sequence else
               flow_pairs_fb(im1, im2, c.levels, init_flow=init, init_flow_bw=init_bw, **kw))
        routes["fb"] = _delta(gpu, before)
        worst = max(worst, _check(_triples(res.flow_fw, res.warpI2_fw, layout), want_fw, None if c.init else oracles,
                                  name + " fb forward", c.out32))
        _check(_triples(res.flow_bw, res.warpI2_bw, layout), want_bw, None, name + " fb backward", c.out32)
        fw = np.stack([np.stack(s[:2]) for s in want_fw])
        bw = np.stack([np.stack(s[:2]) for s in want_bw])
        _same_mask(res.occlusion, fb_reference(fw, bw), name + " occlusion")
        _check_route(c, routes["fb"], True, name + " fb")
    if c.batch_max is not None:
        monkeypatch.delenv("PAPOF_BATCH_MAX")
    line = "%-28s %-5s %s  oracle max-abs %.1e  %.2f s" % (
        name, "chain" if c.chain else "singles",
        "  ".join("%s +%d chains +%d pairs +%d singles +%d reruns" % (r, s["chains"], s["chain_pairs"], s["singles"], s["reruns"])
                  for r, s in routes.items()), worst, time.perf_counter() - t0)
    print(line, flush=True)
    _report.append(line)


def test_report_the_routes_and_the_wall_time(capsys):
    """the last test of the module: the route every case took and the module's wall time, printed past the capture"""
    wall = time.perf_counter() - _started[0]
    with capsys.disabled():
        print("\n" + "\n".join(_report))
        print("test_gpu_batch_shapes: %d cases in %.1f s wall" % (len(_report), wall))
    chain = [c.name for c in bs.CASES if c.chain]
    assert len(_report) <= len(bs.CASES) and len(chain) == len(bs.CASES) - 2
