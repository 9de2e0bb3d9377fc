"""The guarded, poisoned allocations (tests/_alloc.py) catch what they claim -- on CPU tensors, with fake calls in Python --
and the table of tests/test_gpu_alloc_guard.py (tests/_alloc_cases.py) names every device-tensor entry point and can fail."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _alloc  # noqa: E402
import _alloc_cases  # noqa: E402
from _alloc import GUARD, PATTERNS, Guarded, pattern_bytes, same_bytes  # noqa: E402

from papteam_opticalflow_amd import capi  # noqa: E402

BOTH = pytest.mark.parametrize("pattern", sorted(PATTERNS))


def _fake_call(g, x, skip=None, stray=None, ws_stray=None, spoil_input=False):
    """out = 2 x through g.empty, with a workspace as tensors._launch takes it: allocated inside the launch and dropped
    right behind it.  skip: an output element left unwritten; stray: a byte offset relative to the output that is written
    too; ws_stray: one relative to the workspace; spoil_input: the call writes into x"""
    out = g.empty(tuple(x.shape), dtype=torch.float32, device="cpu")
    with g.launching("fake_entry"):
        ws = g.empty((40,), dtype=torch.uint8, device="cpu")
        ws.fill_(7)
        if ws_stray is not None:
            g.buffers[-1].raw[GUARD + ws_stray] = 0x33
        del ws
    flat, src = out.reshape(-1), x.reshape(-1)
    for i in range(flat.numel()):
        if i != skip:
            flat[i] = 2 * src[i]
    if stray is not None:
        g.buffers[1].raw[GUARD + stray] = 0x33
    if spoil_input:
        raw = x.reshape(-1).view(torch.uint8)
        raw[12] = raw[12] ^ 0xff
    return out


def _values():
    return np.arange(1, 31, dtype=np.float32).reshape(2, 3, 5)


@BOTH
def test_a_clean_call_passes(pattern):
    g = Guarded(pattern, device="cpu")
    x = g.put(_values())
    out = _fake_call(g, x)
    g.check()
    same_bytes(out, 2 * _values(), "clean")
    assert g.served == 2 and g.launched == ["fake_entry"]
    assert [b.role for b in g.buffers] == ["input", "output", "workspace of fake_entry"]  # the workspace is still alive
    assert all(b.tensor.data_ptr() % 512 == b.raw.data_ptr() % 512 for b in g.buffers)  # PyTorch's alignment is kept
    g.free()
    assert not g.buffers


@BOTH
def test_the_whole_buffer_holds_the_pattern_first(pattern):
    g = Guarded(pattern, device="cpu")
    for dtype, shape in ((torch.float64, (3, 5)), (torch.float32, (7,)), (torch.uint8, (2, 3, 5)), (torch.bool, (4, 3)),
                         (torch.uint16, (3, 3)), (torch.int32, (2, 2)), (torch.int64, (3,)), (torch.float32, (0, 4))):
        t = g.empty(shape, dtype=dtype, device="cpu")
        b = g.buffers[-1]
        assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
        assert b.raw.numel() == 2 * GUARD + b.nbytes and b.nbytes == t.numel() * t.element_size()
        assert np.array_equal(b.raw.numpy(), pattern_bytes(pattern, b.raw.numel()))
        assert np.array_equal(_alloc.as_bytes(t).numpy(), pattern_bytes(pattern, b.nbytes))
    g.check()
    if pattern == "A":  # a quiet NaN as float64, two NaNs as float32, no byte that is 0 or 1
        assert torch.isnan(g.buffers[0].tensor).all() and torch.isnan(g.buffers[1].tensor).all()
        assert not set(PATTERNS["A"]) & {0, 1}
        assert np.frombuffer(PATTERNS["A"], np.uint64)[0] == 0x7FF8DEAD7FF8DEAD
    else:
        assert g.buffers[3].tensor.all() and (g.buffers[5].tensor == 0x01010101).all()
        assert torch.isfinite(g.buffers[0].tensor).all()


@BOTH
def test_an_unwritten_output_element_fails(pattern):
    g = Guarded(pattern, device="cpu")
    out = _fake_call(g, g.put(_values()), skip=17)
    g.check()  # nothing was written outside: only the values tell
    with pytest.raises(AssertionError, match=r"1 of 30 elements differ, the first at \(1, 0, 2\)"):
        same_bytes(out, 2 * _values(), "unwritten")


@BOTH
def test_a_byte_written_outside_an_output_is_named(pattern):
    """the first and the last byte of the band in front of the output and of the one behind it"""
    for stray, side in ((-1, "before"), (-GUARD, "before"), (120, "behind"), (120 + GUARD - 1, "behind")):
        g = Guarded(pattern, device="cpu")
        out = _fake_call(g, g.put(_values()), stray=stray)
        same_bytes(out, 2 * _values(), "the values are right")
        with pytest.raises(AssertionError) as e:
            g.check()
        text = str(e.value)
        assert "output (2, 3, 5) float32" in text and "byte %d relative to the tensor, %s it (120 bytes)" % (stray, side) in text
        assert "pattern %s" % pattern in text


@BOTH
def test_a_byte_written_behind_a_workspace_is_named(pattern):
    g = Guarded(pattern, device="cpu")
    _fake_call(g, g.put(_values()), ws_stray=40)
    with pytest.raises(AssertionError) as e:
        g.check()
    assert "workspace of fake_entry (40,) uint8" in str(e.value) and "byte 40 relative to the tensor, behind it" in str(e.value)


@BOTH
def test_a_modified_input_is_named(pattern):
    g = Guarded(pattern, device="cpu")
    _fake_call(g, g.put(_values()), spoil_input=True)
    with pytest.raises(AssertionError, match=r"input \(2, 3, 5\) float32 .*byte 12 relative to the tensor, inside it"):
        g.check()
    g = Guarded(pattern, device="cpu")  # and a byte in front of an input
    x = g.put(_values())
    g.buffers[0].raw[GUARD - 2] = 0x33
    with pytest.raises(AssertionError, match=r"input \(2, 3, 5\) float32 .*byte -2 relative to the tensor, before it"):
        g.check()
    assert x.shape == (2, 3, 5)


def test_same_bytes_counts_the_sign_of_a_zero_and_bool_as_uint8():
    same_bytes(torch.tensor([0.0, 1.0]), np.array([0.0, 1.0], np.float32), "equal")
    with pytest.raises(AssertionError, match="got bytes 00000080, expected 00000000"):
        same_bytes(torch.tensor([-0.0, 1.0]), np.array([0.0, 1.0], np.float32), "the sign of a zero")
    same_bytes(torch.tensor([True, False]), np.array([1, 0], np.uint8), "bool as uint8")
    with pytest.raises(AssertionError):
        same_bytes(torch.tensor([1.0]), np.array([1.0]), "another dtype")
    words = np.array([[1, 0xfffe]], np.uint16)
    same_bytes(_alloc.to_tensor(words), words, "uint16")


def test_install_routes_the_allocations_and_records_the_launches(monkeypatch):
    """tensors._torch() is the stand-in, and what _launch allocates inside is named a workspace of its entry point"""
    from papteam_opticalflow_amd import tensors
    g = Guarded("B", device="cpu")
    seen = []

    def fake_launch(dev, name, *args, workspace=None, timers=None):
        seen.append(name)
        tensors._torch().empty((8,), dtype=torch.uint8, device=dev)
    monkeypatch.setattr(tensors, "_launch", fake_launch)
    _alloc.install(monkeypatch, tensors, g)
    assert tensors._torch() is g and tensors._torch().float32 is torch.float32
    tensors._launch("cpu", "papof_fake_tensor")
    out, _ = tensors._new_frames(2, 3, 4, 1, "NHWC", torch.float32, "cpu")
    assert seen == g.launched == ["papof_fake_tensor"] and g.served == 2
    assert [b.role for b in g.buffers] == ["workspace of papof_fake_tensor", "output"] and out is g.buffers[1].tensor
    g.check()


# ---- the table

def test_the_table_names_every_device_tensor_entry_point():
    """no exemption list: an entry point that no row launches is a finding, and a new papof_*_tensor export needs a row"""
    rows = _alloc_cases.ROWS
    want = {s for s in capi.SYMBOLS if "_tensor" in s}
    got = set().union(*(r.entries for r in rows))
    assert got == want, "without a row: %s; not exported: %s" % (sorted(want - got), sorted(got - want))
    assert len({r.name for r in rows}) == len(rows)
    from papteam_opticalflow_amd import tensors
    for r in rows:
        assert r.entries and callable(getattr(tensors, r.fn)) and r.dead, r.name


def test_each_rows_reference_can_fail():
    """every row has an output, and no expected output equals either pattern's bytes: an output that the call never wrote
    cannot pass.  The inputs are what the row says: numpy arrays with items.  (One test for the table, not one per row: the
    GPU test is the one that runs per row.)"""
    for row in _alloc_cases.ROWS:
        name = row.name
        b = _alloc_cases.built(name)
        assert b.inputs and all(isinstance(a, np.ndarray) and a.size for a in b.inputs.values()), name
        assert b.want is not None and len(b.want) >= 1, name
        for k, w in enumerate(b.want):
            w = np.ascontiguousarray(w)
            assert w.size, (name, k)
            raw = w.view(np.uint8).reshape(-1)
            for pattern in PATTERNS:
                assert not np.array_equal(raw, pattern_bytes(pattern, raw.size)), (name, k, pattern)


def test_each_bound_passes_the_restatement_and_fails_an_unwritten_output():
    """the rows that are held within a bound and not to the bytes (the fits, the bundle sums, the flow calls): the row's
    check passes the restatement's own outputs, and fails when any one output is what the memory held, under either pattern
    -- pattern B's small finite floats and ones included"""
    bound = [r.name for r in _alloc_cases.ROWS if _alloc_cases.built(r.name).check is not None]
    assert {"global_motion", "global_homography", "bundle_sums", "flow_video B=3", "flow_video_fb init B=1"} <= set(bound)
    assert len(bound) == 11
    for name in bound:
        b = _alloc_cases.built(name)
        right = [_alloc.to_tensor(w) for w in b.want]
        b.check(right, name)
        for k in range(len(right)):
            for pattern in sorted(PATTERNS):
                g = Guarded(pattern, device="cpu")
                got = list(right)
                got[k] = g.empty(tuple(right[k].shape), dtype=right[k].dtype, device="cpu")
                with pytest.raises(AssertionError):
                    b.check(got, "%s with output %d unwritten, pattern %s" % (name, k, pattern))
