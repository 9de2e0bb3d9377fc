"""The coarse-to-fine call started from an initial flow, restated on the CPU oracle's per-stage functions (include/papof.h:
papof_flow_batch_tensor_init states the rule).  Without an initial flow this is orc_coarse2fine_flow, stage by stage:
tests/test_init_flow_cpu.py pins that bit for bit, so that the composition itself is known to be the reference's.

    vx, vy, warpI2 = coarse2fine_init(orc, im1, im2, levels, init=None)   # HWC float64 frames; init (H, W, 2) or None

Only the test suite imports this module."""
import ctypes

import numpy as np

from _libs import _D, _c, _p, OracleLib  # noqa: F401  (OracleLib: the caller's handle)

BILINEAR, BICUBIC = 0, 1
LAPLACIAN, GMIXTURE = 0, 1


def clamped_ratio(ratio):
    """the ratio the pyramid and the up-sampling use (src/GaussianPyramid.cpp:82-83)"""
    return 0.75 if ratio > 0.98 or ratio < 0.4 else ratio


def init_scale(levels, ratio=0.75):
    """s = 1.0 multiplied by ratio L - 1 times in fp64"""
    s, r = 1.0, clamped_ratio(ratio)
    for _ in range(levels - 1):
        s *= r
    return s


def coarsest_init(orc, init, levels, ratio=0.75):
    """(u, v) at level L - 1 from an (H, W, 2) initial flow: init itself for L == 1, else the coarsest level of the frames'
    pyramid applied to init as a two-channel image, times s"""
    init = _c(init)
    if levels == 1:
        return init[..., 0].copy(), init[..., 1].copy()
    top = orc.pyramid(init, ratio, levels)[levels - 1]
    s = init_scale(levels, ratio)
    return np.ascontiguousarray(top[..., 0] * s), np.ascontiguousarray(top[..., 1] * s)


def coarse2fine_init(orc, im1, im2, levels, init=None, interpolation=BILINEAR, noise_model=LAPLACIAN, alpha=0.012,
                     ratio=0.75, n_outer=7, n_outer_per_level=1, n_inner=1, n_sor=30, n_sor_per_level=3, omega=1.8):
    """(vx, vy, warpI2) of the call on HWC float64 frames, from `init` (H, W, 2) or zero flow (init None)"""
    L = orc.L
    im1, im2 = _c(im1), _c(im2)
    h, w, c = im1.shape
    r = clamped_ratio(ratio)
    p1, p2 = orc.pyramid(im1, ratio, levels), orc.pyramid(im2, ratio, levels)
    fc = L.orc_im2feature(None, 1, 1, c, None)
    lappara = np.full(max(c + 2, fc), 0.02)  # carried from level to level (src/OpticalFlow.cpp:773-775)
    gm = None
    if noise_model == GMIXTURE:
        gm = np.zeros(5 * max(c + 2, fc))
        L.orc_gm_reset.argtypes = [_D, ctypes.c_int]
        L.orc_gm_reset(_p(gm), fc)
    L.orc_smoothflow_sor_ex.argtypes = [_D, _D, _D, _D, _D, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, _D, _D,
                                        ctypes.c_int, _D]
    phase = np.zeros(4)
    u = v = None
    for k in range(levels - 1, -1, -1):
        lh, lw = p1[k].shape[:2]
        f1, f2 = orc.im2feature(p1[k]), orc.im2feature(p2[k])
        if k == levels - 1:
            if init is None:  # :801-806
                u, v = np.zeros((lh, lw)), np.zeros((lh, lw))
                warp = f2.copy()
            else:  # the rule: the coarsest level entered as every finer one
                u, v = coarsest_init(orc, init, levels, ratio)
                warp = orc.warpFL(f1, f2, u, v) if interpolation == BILINEAR else orc.bicubic_warp_noclamp(f1, f2, u, v)
        else:  # :809-816
            inv = 1 / r
            u = np.ascontiguousarray(orc.resize_wh(u[..., None], lw, lh)[..., 0] * inv)
            v = np.ascontiguousarray(orc.resize_wh(v[..., None], lw, lh)[..., 0] * inv)
            warp = orc.warpFL(f1, f2, u, v) if interpolation == BILINEAR else orc.bicubic_warp_noclamp(f1, f2, u, v)
        warp = np.ascontiguousarray(warp)
        L.orc_smoothflow_sor_ex(_p(f1), _p(f2), _p(warp), _p(u), _p(v), lh, lw, fc, alpha, n_outer + k * n_outer_per_level,
                                n_inner, n_sor + k * n_sor_per_level, omega, 0, _p(lappara), _p(phase), interpolation,
                                _p(gm) if gm is not None else None)
    return u, v, orc.bicubic_warp(im1, im2, u, v)  # :841-842
