"""Every device-tensor call on poisoned, guarded outputs and workspaces (tests/_alloc.py has the why and the harness,
tests/_alloc_cases.py the table; tests/test_alloc_guard_cpu.py checks both without a GPU).

Each row runs twice in its test, once per pattern: its inputs are placed between guard bands, tensors.py allocates its
outputs and -- through _launch -- its workspaces from buffers whose every byte holds the pattern, and after the call and a
synchronize
  * every guard byte of every buffer still holds the pattern, and every input the bytes it was given;
  * the outputs are the BYTES of the numpy restatement -- or lie within the bound that the call's own test pins;
  * the entry points that the row names were launched, and every output that the call returned lies in a buffer that the
    stand-in served (but the one that a wrapper derives with torch, which the row names): a wrapper that allocates by
    another route fails;
  * and then the outputs under pattern A and under pattern B have the same bytes as each other.
A kernel that relies on what its memory held fails the second or the last, one that writes outside what it was given the
first.  The handle's own arena is not poisoned here: tests/test_gpu_handle_state.py owns that."""
import time

import pytest

import _alloc
import _alloc_cases
from _alloc import PATTERNS, Guarded, as_bytes, same_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    """the module's handle on device 0 (tensors._handle), given back when the module ends"""
    from papteam_opticalflow_amd import tensors
    yield tensors._handle(0)[0]
    for g, _ in tensors._handles.values():
        g.close()
    tensors._handles.clear()
    torch.cuda.empty_cache()


def _served(g, t):
    """the tensor's memory lies in a buffer that the stand-in served for an output"""
    at = t.untyped_storage().data_ptr()
    return any(b.role == "output" and b.raw.data_ptr() <= at < b.raw.data_ptr() + b.raw.numel() for b in g.buffers)


def _run(monkeypatch, row, b, pattern):
    """the row's call under one pattern, every check but A against B: the outputs' bytes on the host"""
    from papteam_opticalflow_amd import tensors
    t0 = time.perf_counter()
    g = Guarded(pattern)
    d = {k: g.put(a) for k, a in b.inputs.items()}
    _alloc.install(monkeypatch, tensors, g)
    try:
        got = b.run(d)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    what = "%s, pattern %s" % (row.name, pattern)
    g.check()
    missing = [e for e in row.entries if e not in g.launched]
    assert not missing, "%s: launched %s, not %s" % (what, g.launched, missing)
    assert got and all(isinstance(t, torch.Tensor) for t in got), what
    elsewhere = [k for k, t in enumerate(got) if k not in b.derived and not _served(g, t)]
    assert g.served >= 1 and not elsewhere, "%s: outputs %s were not allocated through tensors._torch().empty" % (what, elsewhere)
    if b.check is not None:
        b.check(got, what)
    else:
        assert len(got) == len(b.want), (what, len(got), len(b.want))
        for k, (t, w) in enumerate(zip(got, b.want)):
            same_bytes(t, w, "%s output %d" % (what, k))
    roles = [x.role for x in g.buffers]
    print("%-28s %s  %s  outputs %d workspaces %d  %.3f s" % (
        row.name, pattern, " ".join(g.launched), roles.count("output"), sum(r.startswith("workspace") for r in roles),
        time.perf_counter() - t0), flush=True)
    mine = [as_bytes(t).cpu() for t in got]
    del d, got
    g.free()
    return mine


@pytest.mark.parametrize("name", [r.name for r in _alloc_cases.ROWS])
def test_row(monkeypatch, name):
    row = _alloc_cases.BY_NAME[name]
    b = _alloc_cases.built(name)  # the reference: once per row, shared by both patterns
    a, z = (_run(monkeypatch, row, b, pattern) for pattern in sorted(PATTERNS))
    for k, (x, y) in enumerate(zip(a, z)):  # bitwise reproducible, whatever the memory held
        assert torch.equal(x, y), "%s output %d: %d bytes differ between pattern A and pattern B" % (name, k, int((x != y).sum()))
