"""The two claims about the numpy restatements on which the oracle of tests/test_gpu_split_launches.py rests
(tests/_seam.py: temporal_bank), checked against the full restatement on a periodic video of 4 periods, for every temporal
case of the table: a periodic video gives a periodic interior, and a window of the video reproduces the full result away
from the window's ends.  Also the table itself: the counts cross their cuts, and the first item of a second launch is not
item 0 in any operand."""
import numpy as np
import pytest

import _seam
from _seam import CASES, index, temporal_bank

TEMPORAL = [c for c in CASES if c.oracle == "temporal"]


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = (a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(1)
    assert not bad.any(), "%s: frames %s differ" % (what, np.nonzero(bad)[0].tolist())


@pytest.mark.parametrize("case", TEMPORAL, ids=[c.name for c in TEMPORAL])
def test_the_oracle_is_the_full_restatement(case):
    b = case.build()
    n, r, period = 4 * b.period, b.reach, b.period
    full = b.ref(0, n)
    assert all(f.shape[0] == n for f in full)
    # a periodic video gives a periodic interior
    for k, f in enumerate(full):
        _same(f[r + 1:n - r - 1 - period], f[r + 1 + period:n - r - 1], "%s output %d, one period on" % (case.name, k))
    # a window reproduces the full result away from its ends: one that starts inside the video, at an odd frame
    s, L = period + 1, 2 * r + 2 + 3
    for k, (w, f) in enumerate(zip(b.ref(s, L), full)):
        _same(w[r + 1:L - r - 1], f[s + r + 1:s + L - r - 1], "%s output %d, window" % (case.name, k))
    # so the oracle's bank, gathered, is the full restatement: ends and interior
    bank, idx = temporal_bank(b.ref, n, r, period)
    assert idx.shape == (n,) and len(bank) == len(full)
    for k, (w, f) in enumerate(zip(bank, full)):
        _same(w[idx], f, "%s output %d, the oracle" % (case.name, k))
    # the output is not constant over the frames: the comparison can fail
    assert any((np.ascontiguousarray(f[r + 1]).tobytes() != np.ascontiguousarray(f[r + 2]).tobytes()) for f in full)


def test_the_oracle_at_the_count_the_gpu_test_uses():
    """the index of the bank at N = 65537: the ends, the interior, and every row of the bank used"""
    n, r, period = _seam.N_TILES, 2, _seam.P
    calls = []

    def ref(start, count):
        calls.append((start, count))
        return [start + np.arange(count)]  # the frame numbers themselves
    bank, idx = temporal_bank(ref, n, r, period)
    assert calls == [(0, 6), (0, 3 * period), (n - 6, 6)]
    got = bank[0][idx]
    t = np.arange(n)
    assert (got[:r + 1] == t[:r + 1]).all() and (got[-(r + 1):] == t[-(r + 1):]).all()
    mid = got[r + 1:n - r - 1]
    assert (mid % period == t[r + 1:n - r - 1] % period).all() and (mid >= period).all() and (mid < 2 * period).all()
    assert sorted(set(idx.tolist())) == list(range(len(bank[0])))


def test_the_table():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c.count > c.cut and c.count - c.cut >= 2, c.name
        assert c.oracle in ("periodic", "temporal", "full") and c.via in ("wrapper", "C entry")
    assert _seam.TILES_CUT % _seam.P != 0 and _seam.FB_CUT % _seam.P_FB != 0
    assert (index(10, 7, 5) == [5, 6, 0, 1, 2, 3, 4, 5, 6, 0]).all()


@pytest.mark.parametrize("case", [c for c in CASES if c.oracle != "full"], ids=[c.name for c in CASES if c.oracle != "full"])
def test_the_first_item_of_a_second_launch_is_not_item_0(case):
    b = case.build()
    for name, (a, kind) in b.inputs.items():
        if kind == "full":  # shared by the items (a mosaic's frames)
            continue
        a = np.ascontiguousarray(a)
        rows = a.view(np.uint8).reshape(a.shape[0], -1)
        assert a.shape[0] in (_seam.P, _seam.P_FB), (case.name, name)
        for i in range(1, a.shape[0]):
            assert (rows[i] != rows[0]).any(), (case.name, name, i)
