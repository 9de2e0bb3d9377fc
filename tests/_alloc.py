"""Guarded, poisoned allocations for the device-tensor calls (tests/test_gpu_alloc_guard.py, tests/test_alloc_guard_cpu.py).

papteam_opticalflow_amd/tensors.py takes every output, and through _launch every workspace, from torch.empty: memory that holds
what the caching allocator handed out before -- zeros in a fresh test process, the leftovers of other tensors in a user's.  A
kernel that relies on what its memory held (an output element that a branch never writes, a workspace cleared too short, a tap
of weight 0 on an iterate nobody wrote) is right on zeros and wrong on anything else; a kernel that writes one element past
what it was given lands in a neighbour's tensor inside the allocator's block and never faults.

Guarded is a stand-in for tensors._torch() in the manner of _FarTorch (tests/test_gpu_far_offsets.py): everything is torch's,
but empty() serves a tensor from the middle of a fresh uint8 buffer of GUARD + nbytes + GUARD bytes whose EVERY byte holds a
pattern first.  GUARD is a multiple of 512 bytes, so the data pointer keeps the alignment that PyTorch gives and the aligned
dword and 8-byte instances of the kernels are still chosen.  put() places a call's inputs the same way.  Every buffer stays
alive until check(): the workspace too, which _launch drops right behind the call.

check() -- after the call and a synchronize -- asserts that every guard byte of every buffer still holds the pattern and that
every input still has the bytes it was given, and names the buffer (shape, dtype, role) and the offset of the first byte that
differs, relative to the tensor.

The patterns:
  A  0x7FF8DEAD7FF8DEAD repeated: a quiet NaN as float64, two NaNs as float32, no byte that is 0 or 1
  B  the byte 0x01: small finite floats, True, 1 -- what NaN propagation would mask (a comparison that is false for NaN)"""
import contextlib

import numpy as np

GUARD = 64 * 1024
assert GUARD % 512 == 0
PATTERNS = {"A": bytes.fromhex("ADDEF87FADDEF87F"),  # 0x7FF8DEAD7FF8DEAD, little-endian
            "B": b"\x01"}


def _torch():
    import torch
    return torch


def pattern_bytes(pattern, n):
    """the first n bytes of a buffer filled with the pattern, as a numpy uint8 array"""
    p = np.frombuffer(PATTERNS[pattern], np.uint8)
    return np.tile(p, -(-max(n, 1) // p.size))[:n].copy()


def as_bytes(t):
    """a tensor's values as a flat uint8 tensor (bool through uint8); the tensor may be a view"""
    torch = _torch()
    t = t.contiguous()
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.reshape(-1).view(torch.uint8) if t.numel() else torch.empty((0,), dtype=torch.uint8, device=t.device)


def to_tensor(a):
    """the tensor of a numpy array (or a tensor as it is); torch has no arithmetic on uint16 but carries its bytes"""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.uint8)).view(torch.uint16).reshape(a.shape)
    return torch.from_numpy(a)


def same_bytes(got, want, what):
    """a tensor against the expected values (a numpy array or a tensor), byte for byte: the sign of a zero counts, bool is
    compared as uint8; names the first element that differs"""
    torch = _torch()
    want = to_tensor(want)
    if want.dtype == torch.bool:
        want = want.view(torch.uint8)
    if got.dtype == torch.bool:
        got = got.view(torch.uint8)
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape),
                                                                              got.dtype, want.dtype)
    g, w = as_bytes(got).cpu(), as_bytes(want).cpu()
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero().reshape(-1)
    size = got.element_size()
    first = int(bad[0]) // size
    where = np.unravel_index(first, tuple(got.shape)) if got.dim() else ()
    n = int(torch.unique(bad // size).numel())
    raise AssertionError("%s: %d of %d elements differ, the first at %s: got bytes %s, expected %s"
                         % (what, n, got.numel(), tuple(int(i) for i in where),
                            bytes(g[first * size:(first + 1) * size].tolist()).hex(),
                            bytes(w[first * size:(first + 1) * size].tolist()).hex()))


class _Buffer:
    def __init__(self, raw, tensor, nbytes, role, given):
        self.raw, self.tensor, self.nbytes, self.role = raw, tensor, nbytes, role
        self.given = given  # an input: the whole buffer as it was handed to the call

    def name(self):
        return "%s %s %s" % (self.role, tuple(self.tensor.shape), str(self.tensor.dtype).replace("torch.", ""))


class Guarded:
    """torch, but empty() and put() serve tensors between two guard bands of a buffer filled with the pattern"""

    def __init__(self, pattern, device="cuda", guard=GUARD):
        assert guard % 512 == 0 and pattern in PATTERNS
        self.pattern, self.device, self.guard = pattern, device, guard
        self.buffers = []   # every buffer served, alive until free()
        self.served = 0     # calls of empty()
        self.launched = []  # the entry points of launching()
        self._role = "output"

    def __getattr__(self, name):
        return getattr(_torch(), name)

    def _filled(self, n, device):
        torch = _torch()
        p = torch.from_numpy(np.frombuffer(PATTERNS[self.pattern], np.uint8).copy())
        raw = torch.empty((n,), dtype=torch.uint8, device=device)
        raw.copy_(p.repeat(-(-n // p.numel()))[:n])
        return raw

    def _serve(self, shape, dtype, device, role, values=None):
        torch = _torch()
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        size = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * size
        raw = self._filled(2 * self.guard + nbytes, device)
        mid = raw[self.guard:self.guard + nbytes]
        if dtype == torch.bool:
            t = mid.view(torch.bool).reshape(shape)
        else:
            t = (mid.view(dtype) if nbytes else torch.empty((0,), dtype=dtype, device=raw.device)).reshape(shape)
        assert t.is_contiguous() and (not nbytes or t.data_ptr() == raw.data_ptr() + self.guard)
        given = None
        if values is not None:
            mid.copy_(as_bytes(values))
            given = raw.clone()
        self.buffers.append(_Buffer(raw, t, nbytes, role, given))
        return t

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = shape[0]
        self.served += 1
        return self._serve(shape, dtype or _torch().get_default_dtype(), device if device is not None else self.device,
                           self._role)

    def put(self, values):
        """a guarded tensor that holds `values` (a numpy array or a tensor): an input of the call"""
        t = to_tensor(values)
        return self._serve(t.shape, t.dtype, self.device, "input", t)

    @contextlib.contextmanager
    def launching(self, name):
        """around tensors._launch: records the entry point, and what is allocated inside is its workspace"""
        self.launched.append(name)
        self._role, before = "workspace of " + name, self._role
        try:
            yield
        finally:
            self._role = before

    def check(self):
        """every guard byte of every buffer holds the pattern, and every input the bytes it was given"""
        torch = _torch()
        for b in self.buffers:
            g, n = self.guard, b.nbytes
            want = b.given if b.given is not None else self._filled(b.raw.numel(), b.raw.device)
            parts = [(0, g), (g + n, 2 * g + n)] if b.given is None else [(0, 2 * g + n)]
            for lo, hi in parts:
                if torch.equal(b.raw[lo:hi], want[lo:hi]):
                    continue
                at = lo + int((b.raw[lo:hi] != want[lo:hi]).nonzero()[0])
                side = "before" if at < g else "behind" if at >= g + n else "inside"
                raise AssertionError("%s (pattern %s): byte %d relative to the tensor, %s it (%d bytes), was changed: 0x%02x, "
                                     "was 0x%02x" % (b.name(), self.pattern, at - g, side, n, int(b.raw[at]), int(want[at])))

    def free(self):
        self.buffers = []


def install(monkeypatch, tensors, guarded):
    """tensors.py allocates from `guarded`, and its _launch records the entry points and marks the workspaces"""
    launch = tensors._launch

    def recording(dev, name, *args, **kw):
        with guarded.launching(name):
            return launch(dev, name, *args, **kw)
    monkeypatch.setattr(tensors, "_torch", lambda: guarded)
    monkeypatch.setattr(tensors, "_launch", recording)
