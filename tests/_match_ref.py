"""Dense block matching (include/papof.h: papof_match_tensor, papof_match_densify_tensor) restated in numpy integers -- the
rule that tests/test_match_cpu.py checks with known answers and tests/test_gpu_match.py compares the device's outputs with,
byte for byte -- and the synthetic large-displacement scenes both test files build.

    disp, cost = match_reference(A, B, stride=2, patch=3, search=20)      # A, B (n, H, W, C); disp (n, 2, h, w), cost (n, h, w)
    flow, hole = densify_reference(disp_fw, disp_bw, cost_fw, (H, W), stride)

Only the test suite and tools/match_probe.py import this module."""
import numpy as np

STRIDES = (1, 2, 4, 8)


def quantise(x):
    """frames of uint8 (as they are), float32 or float64 (rint(255 x) clamped to 0 .. 255, NaN -> 0) as uint8"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    assert x.dtype in (np.float32, np.float64), x.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(255.0 * x.astype(np.float64))
    return np.clip(np.where(np.isnan(q), 0.0, q), 0.0, 255.0).astype(np.uint8)


def decimate(q, stride):
    """q (n, H, W, C) uint8 -> (n, H // stride, W // stride, C) int64: (sum + stride^2 / 2) // stride^2 per channel"""
    n, H, W, C = q.shape
    h, w = H // stride, W // stride
    blocks = q[:, :h * stride, :w * stride].astype(np.int64).reshape(n, h, stride, w, stride, C)
    return (blocks.sum(axis=(2, 4)) + stride * stride // 2) // (stride * stride)


def _key(cost, dx, dy):
    """the lexicographic key (cost, dx^2 + dy^2, dy, dx) as one integer"""
    return (cost << 26) | ((dx * dx + dy * dy) << 14) | ((dy + 64) << 7) | (dx + 64)


def match_coarse(a, b, patch, search, penalty=0):
    """a, b (h, w, C) int64 coarse frames -> (d (2, h, w) int64 in coarse pixels (dx, dy), cost (h, w) int64)"""
    h, w, _ = a.shape
    P = patch
    ys, xs = np.arange(-P, h + P), np.arange(-P, w + P)
    ap = a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    yy, xx = np.mgrid[0:h, 0:w]
    best = np.full((h, w), np.iinfo(np.int64).max)
    for dy in range(-search, search + 1):
        rows = np.clip(ys + dy, 0, h - 1)
        row_ok = (yy + dy >= 0) & (yy + dy < h)
        if not row_ok.any():
            continue
        for dx in range(-search, search + 1):
            ok = row_ok & (xx + dx >= 0) & (xx + dx < w)
            if not ok.any():
                continue
            D = np.abs(ap - b[rows][:, np.clip(xs + dx, 0, w - 1)]).sum(axis=2)
            S = np.zeros((h + 2 * P + 1, w + 2 * P + 1), np.int64)
            S[1:, 1:] = D.cumsum(0).cumsum(1)
            n = 2 * P + 1
            cost = S[n:, n:] - S[:-n, n:] - S[n:, :-n] + S[:-n, :-n] + penalty * (abs(dx) + abs(dy))
            best = np.where(ok, np.minimum(best, _key(cost, dx, dy)), best)
    d = np.stack([(best & 127) - 64, ((best >> 7) & 127) - 64])
    return d, best >> 26


def match_reference(A, B, stride=2, patch=3, search=20, penalty=0, out_dtype=np.float64):
    """A, B (n, H, W, C) uint8 / float32 / float64 -> (disp (n, 2, h, w) = stride * d, cost (n, h, w)) of out_dtype"""
    a, b = decimate(quantise(A), stride), decimate(quantise(B), stride)
    got = [match_coarse(a[i], b[i], patch, search, penalty) for i in range(a.shape[0])]
    return (np.stack([stride * d for d, _ in got]).astype(out_dtype), np.stack([c for _, c in got]).astype(out_dtype))


def densify_reference(disp, disp_rev, cost, size, stride, tol=1, max_cost=None):
    """disp, disp_rev (n, 2, h, w), cost (n, h, w) or None, size (H, W) -> (flow (n, 2, H, W) float64, hole (n, H, W) uint8)"""
    H, W = size
    disp, rev = np.asarray(disp, np.float64), np.asarray(disp_rev, np.float64)
    n, _, h, w = disp.shape
    assert (h, w) == (H // stride, W // stride)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = disp[:, 0] / float(stride), disp[:, 1] / float(stride)
        qx, qy = xx + dx, yy + dy
        ok = (np.rint(dx) == dx) & (np.rint(dy) == dy) & (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
        ix, iy = np.where(ok, qx, 0).astype(np.int64), np.where(ok, qy, 0).astype(np.int64)
        item = np.arange(n)[:, None, None]
        ok &= (np.abs(dx + rev[item, 0, iy, ix] / float(stride)) <= tol) & (np.abs(dy + rev[item, 1, iy, ix] / float(stride)) <= tol)
        if max_cost is not None and max_cost >= 0:
            ok &= np.asarray(cost, np.float64) <= max_cost
    cy, cx = np.minimum(np.arange(H) // stride, h - 1), np.minimum(np.arange(W) // stride, w - 1)
    full = ok[:, cy][:, :, cx]
    flow = np.where(full[:, None], disp[:, :, cy][:, :, :, cx], 0.0)
    return flow, (~full).astype(np.uint8)


# ---- the scenes of the large-displacement tests: band-limited random RGB texture quantised to uint8, a textured object on
# a background that moves by (1, 0)
def texture(rng, H, W, C=3, sigma=1.5):
    """(H, W, C) uint8: white noise low-passed by a Gaussian in the Fourier domain (periodic), stretched to 0 .. 255"""
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    g = np.exp(-2.0 * (np.pi * sigma) ** 2 * (fx * fx + fy * fy))
    out = np.empty((H, W, C))
    for c in range(C):
        t = np.fft.ifft2(np.fft.fft2(rng.standard_normal((H, W))) * g).real
        out[..., c] = (t - t.min()) / (t.max() - t.min())
    return np.rint(255.0 * out).astype(np.uint8)


def object_scene(seed, motion, H=135, W=240, size=24, origin=(100, 60), background=(1, 0)):
    """(im1, im2 (H, W, 3) uint8, truth (H, W, 2) of im1's pixels, interior (H, W) bool: the object less a 3 px margin).
    The background is one large texture shifted by `background`; the size x size object, a texture of its own with its top
    left corner at `origin` (x, y) in im1, moves by `motion` (dx, dy)."""
    rng = np.random.default_rng(seed)
    pad = 64
    bg = texture(rng, H + 2 * pad, W + 2 * pad)
    obj = texture(rng, size, size)
    bx, by = background
    im1 = bg[pad:pad + H, pad:pad + W].copy()
    im2 = bg[pad - by:pad - by + H, pad - bx:pad - bx + W].copy()
    ox, oy = origin
    mx, my = motion
    im1[oy:oy + size, ox:ox + size] = obj
    im2[oy + my:oy + my + size, ox + mx:ox + mx + size] = obj
    truth = np.zeros((H, W, 2))
    truth[..., 0], truth[..., 1] = bx, by
    truth[oy:oy + size, ox:ox + size] = (mx, my)
    interior = np.zeros((H, W), bool)
    interior[oy + 3:oy + size - 3, ox + 3:ox + size - 3] = True
    return im1, im2, truth, interior


def pan_scene(seed, motion, H=135, W=240):
    """(im1, im2, truth, interior): the whole frame moves by `motion`; interior = the pixels that stay in view, less 3 px"""
    rng = np.random.default_rng(seed)
    pad = 64
    bg = texture(rng, H + 2 * pad, W + 2 * pad)
    mx, my = motion
    im1 = bg[pad:pad + H, pad:pad + W].copy()
    im2 = bg[pad - my:pad - my + H, pad - mx:pad - mx + W].copy()
    truth = np.zeros((H, W, 2))
    truth[..., 0], truth[..., 1] = mx, my
    yy, xx = np.mgrid[0:H, 0:W]
    interior = (xx + mx >= 3) & (xx + mx < W - 3) & (yy + my >= 3) & (yy + my < H - 3)
    return im1, im2, truth, interior


def epe(vx, vy, truth, where):
    return float(np.hypot(vx - truth[..., 0], vy - truth[..., 1])[where].mean())
