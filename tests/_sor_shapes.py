"""Planes that pin every instance of the one-workgroup exact-order solver (csrc/sor.hip: k_sor_tiny<C, NW>) at the edges of
its shape heuristic (tiny_shape): (cells per tile C, (height, width), waves of the launch, what the plane is there for).
tests/test_sor_tiny_shapes.py holds the table against the library's own answer (papof_sor_tiny_shape) on the CPU, so a change
of the heuristic fails there instead of silently moving what tests/test_gpu_sor_kernels.py covers."""

TINY_SHAPES = [
    (1, (1, 1), 1, "smallest"),
    (1, (1, 2), 1, "one lane, two tiles"),
    (1, (1, 2048), 16, "full workgroup"),
    (1, (1024, 1), 16, "full workgroup"),
    (1, (32, 63), 16, "odd segment count"),
    (1, (60, 33), 16, "odd segment count"),
    (2, (2, 2048), 16, "full workgroup"),
    (2, (1, 3192), 13, "LDS at the cap"),
    (2, (798, 3), 13, "LDS at the cap, ragged tile"),
    (2, (798, 4), 13, "LDS at the cap"),
    (2, (63, 64), 16, ""),
    (2, (22, 131), 12, "ragged tile"),
    (3, (2, 2304), 12, "full workgroup"),
    (3, (531, 5), 9, "ragged tile"),
    (3, (48, 85), 12, "ragged tile, odd segment count"),
    (3, (21, 193), 11, "ragged tile"),
    (5, (4, 1280), 8, "full workgroup"),
    (5, (238, 19), 8, "LDS at the cap, ragged tile"),
    (5, (17, 283), 8, "ragged tile"),
    (6, (4, 1536), 8, "full workgroup"),
    (6, (198, 23), 7, "LDS at the cap, ragged tile"),
    (6, (56, 101), 8, "ragged tile"),
    (6, (20, 292), 8, "ragged tile"),
]

# just past each limit of the heuristic: too many lanes for the widest tile, one row / column more than the LDS holds
NOT_TINY = [(1, 3193), (799, 3), (4, 1537), (199, 22), (90, 91)]

TINY_MAX_CELLS = 8192  # csrc/common.h: kTinyMaxCells
