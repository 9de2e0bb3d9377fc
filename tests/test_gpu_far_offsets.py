"""Every offset is 64-bit: the device-tensor kernels on operands whose element offsets exceed 2^32 bytes and 2^31 float32
elements.  The descriptors carry long long strides and the kernels mix them with int rows, columns, items and channels; one
int temporary in a product goes unnoticed as long as every tensor of the suite lives in a few megabytes.

Here the operands -- frames, masks, flows, matrices, weights, and the OUTPUTS that the wrappers allocate -- are as_strided
views of two arenas from torch.empty of which only the few kilobytes under the views are ever touched: a uint8 arena of
2^32 + 2^16 bytes and a float32 arena of 2^31 + 2^14 elements.  The item stride of a view puts its last item beyond the
arena's 2^32nd byte / 2^31st element (for two items: item 1); one variant carries the distance in the ROW stride instead.
The outputs are placed by handing tensors.py an allocator (its _torch().empty) that carves them from the arenas.

The result must be byte-identical to the same call on contiguous copies of the same values with ordinary outputs: the
kernel against itself at near offsets, which the rest of the suite pins to the restatements.  The property is only that
distance does not matter.  The float32 arena (8.6 GB) may skip, with the reason printed, when less than three times its
size is free; the uint8 part never skips."""
import ctypes

import numpy as np
import pytest

from _seam import flows, frames, holes, matrices, occlusion

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from papteam_opticalflow_amd import capi, tensors  # noqa: E402

FAR_U8 = 1 << 32    # bytes
FAR_F32 = 1 << 31   # elements
BLOCK = {torch.uint8: 4096, torch.float32: 1024}  # a view's items each fit one block; 16 blocks lie beyond the far mark


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()


class Arena:
    """as_strided views of one allocation, each in a block of its own"""

    def __init__(self, dtype, far):
        self.dtype, self.far, self.block = dtype, far, BLOCK[dtype]
        self.t = torch.empty((far + 16 * self.block,), dtype=dtype, device="cuda")
        self.next = 0

    def reset(self):
        self.next = 0

    def view(self, shape, rows_far=False):
        """a view of `shape` (items first, the rest contiguous) whose last item starts beyond the far mark -- or, with
        rows_far (shape (n, H, ...), H = 5), whose rows are 2^30 / 2^29 apart so that row 4 of every item lies beyond it"""
        shape = tuple(int(s) for s in shape)
        n, inner = shape[0], int(np.prod(shape[1:]))
        assert self.next < 16, "more views than blocks beyond the far mark"
        base = self.next * self.block
        self.next += 1
        strides = [1]
        for s in reversed(shape[2:]):
            strides.insert(0, strides[0] * s)
        if rows_far:
            assert shape[1] == 5 and n == 2
            row = int(np.prod(shape[2:]))
            assert 2 * row <= self.block // 2
            strides = [self.block // 2, self.far // 4] + strides[1:]
        else:
            assert n >= 2 and inner <= self.block, (shape, self.block)
            strides = [self.far // (n - 1) + (64 if n > 2 else 0)] + strides
        v = torch.as_strided(self.t, shape, strides, base)
        last = v[n - 1, -1] if rows_far else v[n - 1]
        assert (last.data_ptr() - self.t.data_ptr()) // self.t.element_size() >= self.far  # beyond the mark
        end = sum((s - 1) * st for s, st in zip(shape, strides)) + base
        assert end < self.t.numel()                                                           # and inside the arena
        return v

    def put(self, values, rows_far=False):
        """a far view that holds `values` (a numpy array or a tensor)"""
        t = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(values))
        src = t.view(torch.uint8) if t.dtype == torch.bool else t
        v = self.view(src.shape, rows_far)
        v.copy_(src.cuda())
        return v.view(torch.bool) if t.dtype == torch.bool else v


@pytest.fixture(scope="module")
def bytes_arena():
    a = Arena(torch.uint8, FAR_U8)
    yield a
    del a.t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def floats_arena():
    need = 4 * (FAR_F32 + 16 * BLOCK[torch.float32])
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * need:
        reason = "the float32 arena needs %.1f GB, and three times that free: %.1f GB are" % (need / 1e9, free / 1e9)
        print(reason)
        pytest.skip(reason)
    a = Arena(torch.float32, FAR_F32)
    yield a
    del a.t
    torch.cuda.empty_cache()


class _FarTorch:
    """torch, but empty() carves the uint8 and float32 tensors of three and more dimensions from the arenas: handed to
    tensors.py as its _torch(), it places the outputs that the wrappers allocate"""

    def __init__(self, arenas):
        self.arenas = arenas
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None, **kw):
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        if dtype in self.arenas and len(shape) >= 3 and shape[0] >= 2:
            v = self.arenas[dtype].view(shape)
            self.made.append(v)
            return v
        return torch.empty(shape, dtype=dtype, device=device, **kw)


def _far_outputs(monkeypatch, arenas):
    far = _FarTorch(arenas)
    monkeypatch.setattr(tensors, "_torch", lambda: far)

    def mask(n_pairs, H, W, dev):  # tensors._mask writes the strides of a contiguous tensor: here the view's own
        occ = far.empty((n_pairs, 2, H, W), dtype=torch.uint8, device=dev)
        return occ, tensors._struct(occ, (occ.stride(0), occ.stride(2), occ.stride(3), occ.stride(1)), capi.DTYPE_U8)
    monkeypatch.setattr(tensors, "_mask", mask)
    return far


def _flat(result):
    """the tensors of a call's result, in order"""
    if isinstance(result, torch.Tensor):
        return [result]
    return [t for t in result if isinstance(t, torch.Tensor)]


def _same(far, near, what):
    assert len(far) == len(near) and len(far) > 0
    for k, (f, n) in enumerate(zip(far, near)):
        assert f.shape == n.shape and f.dtype == n.dtype, (what, k, f.shape, n.shape, f.dtype, n.dtype)
        as_bytes = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t).contiguous().view(torch.uint8)  # noqa: E731
        assert torch.equal(as_bytes(f), as_bytes(n)), "%s: output %d differs between far and near operands" % (what, k)


def _run(monkeypatch, request, call, operands, floats_far, what, rows_far=(), outputs_far=True):
    """call(**operands on contiguous tensors, ordinary outputs) against call(**operands as far views, far outputs);
    outputs_far False: the call has no output of an arena's dtype"""
    arenas = {torch.uint8: request.getfixturevalue("bytes_arena")}
    if floats_far:
        arenas[torch.float32] = request.getfixturevalue("floats_arena")
    for a in arenas.values():
        a.reset()
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in operands.items()}
    near = _flat(call(**dev))
    torch.cuda.synchronize()
    moved = {}
    for k, t in dev.items():
        key = torch.uint8 if t.dtype == torch.bool else t.dtype
        moved[k] = arenas[key].put(t, rows_far=k in rows_far) if key in arenas and t.dim() >= 3 else t
        assert key not in arenas or t.dim() < 3 or moved[k].data_ptr() != t.data_ptr()
    proxy = _far_outputs(monkeypatch, arenas)
    far = _flat(call(**moved))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert proxy.made or not outputs_far, "no output was placed in an arena"
    _same(far, near, what)
    del proxy, far, near, moved, dev


H, W, C = 5, 66, 2
FLOATS = pytest.mark.parametrize("floats_far", [False, True], ids=["bytes far", "bytes and floats far"])


@FLOATS
@pytest.mark.parametrize("rows_far", [False, True], ids=["items far", "rows far"])
def test_interpolate(monkeypatch, request, floats_far, rows_far):
    """interp_pixel, sample_frame, sample_flow, sample_mask and store"""
    fw, bw = flows(2, H, W, 1)
    ops = dict(a=frames(2, H, W, C, 2), b=frames(2, H, W, C, 3), fw=fw, bw=bw, occ=occlusion(2, H, W, 4))

    def call(a, b, fw, bw, occ):
        return tensors.interpolate(a, b, fw, bw, [0.25, 0.5], occlusion=occ, layout="NHWC")
    _run(monkeypatch, request, call, ops, floats_far, "interpolate", rows_far=("a", "b") if rows_far else ())


@FLOATS
def test_temporal_filter(monkeypatch, request, floats_far):
    """hop chains through three frames and two pairs, the video and the support plane"""
    fw, bw = flows(2, H, W, 5)
    ops = dict(f=frames(3, H, W, C, 6), fw=fw, bw=bw)

    def call(f, fw, bw):
        return tensors.temporal_filter(f, fw, bw, radius=2, layout="NHWC")
    _run(monkeypatch, request, call, ops, floats_far, "temporal_filter")


@FLOATS
def test_flow_pairs_fb(monkeypatch, request, floats_far):
    """k_ingest_frames on far frames, k_emit_outputs on far flows and warps, k_fb_check on a far mask"""
    ops = dict(a=frames(2, 9, 12, 1, 7), b=frames(2, 9, 12, 1, 8))

    def call(a, b):
        r = tensors.flow_pairs_fb(a, b, 1, layout="NHWC", out_dtype=torch.float32)
        return [r.flow_fw, r.flow_bw, r.warpI2_fw, r.warpI2_bw, r.occlusion]
    _run(monkeypatch, request, call, ops, floats_far, "flow_pairs_fb")


def test_fill_holes(monkeypatch, request):
    ops = dict(x=frames(2, H, W, 1, 9), m=holes(2, H, W, 10))

    def call(x, m):
        return tensors.fill_holes(x, m, layout="NHWC", relax=1)
    _run(monkeypatch, request, call, ops, False, "fill_holes")


@FLOATS
def test_match_pairs(monkeypatch, request, floats_far):
    from _seam import _textures
    a, b = _textures(9, 34, 1, 11, [(1, 0), (-2, 1)])
    ops = dict(a=a, b=b)

    def call(a, b):
        m = tensors.match_pairs(a, b, stride=1, patch=1, search=3, layout="NHWC", out_dtype=torch.float32)
        return [m.disp_fw, m.disp_bw, m.cost_fw, m.cost_bw]
    _run(monkeypatch, request, call, ops, floats_far, "match_pairs", outputs_far=floats_far)  # the fields are float32


@FLOATS
def test_mosaic(monkeypatch, request, floats_far):
    from test_gpu_mosaic import _frame_masks, _mats
    rng = np.random.default_rng(12)
    T, h, w, Hc, Wc = 2, 9, 13, 5, 66
    M = _mats(rng, 2, 2, h, w, Hc, Wc).astype(np.float32)
    ops = dict(f=frames(T, h, w, C, 13), masks=_frame_masks(rng, T, h, w), M=M)
    src = np.array([[0, 1], [1, 0]])

    def call(f, masks, M):
        got = tensors.mosaic(f, src, M, (Hc, Wc), mode="median", masks=masks, layout="NHWC")
        return [got.out, got.count]
    _run(monkeypatch, request, call, ops, floats_far, "mosaic")


@FLOATS
def test_warp_affine(monkeypatch, request, floats_far):
    M = matrices(4, H, W, 14)[[0, 3]].astype(np.float32)  # both land in the image
    ops = dict(f=frames(2, H, W, C, 15), M=M)

    def call(f, M):
        return tensors.warp_affine(f, M, layout="NHWC")
    _run(monkeypatch, request, call, ops, floats_far, "warp_affine")


@FLOATS
def test_splat(monkeypatch, request, floats_far):
    fw, _ = flows(2, H, W, 16)
    w = (np.random.default_rng(17).random((2, H, W)) * 1.3).astype(np.float32)
    ops = dict(x=frames(2, H, W, 1, 18), fw=fw, w=w)

    def call(x, fw, w):
        s = tensors.splat(x, fw, [0.5], weight=w, fill=0.5, layout="NHWC")
        return [s.out, s.coverage]
    _run(monkeypatch, request, call, ops, floats_far, "splat")
