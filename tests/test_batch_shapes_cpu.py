"""The case table of tests/_batch_shapes.py against its own restatement of the batched chain's decisions, on the CPU: every
class has a case, every case lies on the side of the decision its class claims, only the two cases meant to run as single
calls expect them, and every case is one the library accepts.  tests/test_gpu_batch_shapes.py compares the chain with the
single calls: a case that the chain silently does not take would pass there without testing anything -- this is the
condition that keeps it from doing so, and papof_batch_stats is its witness on the GPU."""
import numpy as np
import pytest

import _batch_shapes as bs


def test_every_class_has_a_case():
    got = {c.cls for c in bs.CASES}
    assert got == set(bs.CLASSES), sorted(set(bs.CLASSES) ^ got)
    few = {(c.H, c.W) for c in bs.CASES if c.cls == "few pixels"}
    assert few == {(1, 9), (9, 1), (2, 2), (3, 4)}
    assert {c.B for c in bs.CASES if c.cls == "few pixels"} == {2, 3} and {c.C for c in bs.CASES if c.cls == "few pixels"} == {1, 3}
    assert sum(c.cls == "seeded small draw" for c in bs.CASES) == 12 and sum(c.cls == "tile borders" for c in bs.CASES) == 6
    rem = {(c.batch_max, c.B) for c in bs.CASES if c.cls == "remainders"}
    assert rem == {(m, n) for m in (2, 3, 5) for n in (3, 4, 5, 7)}
    assert {c.dtype for c in bs.CASES if c.cls == "dtypes and views"} == {"u8", "f32", "f64"}
    assert {c.view for c in bs.CASES if c.cls == "dtypes and views"} == {None, "nchw", "gray"}
    assert any(c.out32 for c in bs.CASES) and any(c.init == "broadcast" for c in bs.CASES)


@pytest.mark.parametrize("name", [c.name for c in bs.CASES])
def test_the_restatement_puts_the_case_on_the_side_its_class_claims(name):
    c = bs.BY_NAME[name]
    assert bs.expects_chain(c) == c.chain, (name, bs.bands(c), bs.slots(c))
    if c.nb is not None:
        assert bs.bands(c) == c.nb, (name, bs.bands(c))
    if not c.chain:
        assert name.endswith(bs.MAY_RUN_SINGLY), name + ": only the first-single and the 1040-slot cases may run as single calls"
    # admissible: the parameters pass check_params, every level has a pixel
    P = bs.params_of(c)
    assert bs.params_ok(P, c.levels) and bs.default_branches(P)
    sizes = bs.level_sizes(c.H, c.W, P["ratio"], c.levels)
    assert len(sizes) == c.levels and all(h >= 1 and w >= 1 for h, w in sizes), sizes
    assert c.B >= 2 and c.C in (1, 3) and all(0 <= p < c.B for p in c.dup)
    # the frames the GPU test will use
    ids = bs.frame_ids(c)
    assert len(ids) == (c.B + 1 if c.sequence else 2 * c.B)
    pairs = bs.pair_ids(c)
    assert [a == b for a, b in pairs] == [p in c.dup for p in range(c.B)]
    f = bs.frame_u8(c, max(ids))
    assert f.shape == (c.H, c.W, c.C) and f.dtype == np.uint8


def test_the_limits_sit_where_the_table_says():
    by = bs.BY_NAME
    assert bs.bands(by["901x24, last batched"]) == 15 and bs.bands(by["902x24, first single"]) == 16
    assert bs.slots(by["slot limit, 1024"]) == 1024 and bs.slots(by["slot limit, 1040"]) == 1040
    assert bs.bands(by["slot limit, 1040"]) < 16  # ... and nothing but the slots keeps it out of the chain
    assert [c.levels for c in bs.CASES if c.cls == "deep pyramid"] == [32, 33, 40]
    assert 32 <= bs.NZ_LEVELS < 33
    deep = bs.level_sizes(48, 64, 0.95, 40)
    assert deep[27] == (int(48 * 0.95 ** 27), int(64 * 0.95 ** 27)) and min(min(s) for s in deep) >= 1
    # level 0 of the two k_sor_tiny cases on either side of the widest instance; 64 x 128 and 64 x 129 on either side of
    # kTinyMaxCells, level 0 the band kernel's, the coarser levels k_sor_tiny's
    assert bs.tiny_shape(64, 96) != (0, 0) and bs.tiny_shape(64, 97) == (0, 0)
    assert 64 * 128 == bs.TINY_MAX_CELLS and bs.tiny_shape(64, 128) == (0, 0) and bs.tiny_shape(64, 129) == (0, 0)
    assert all(bs.tiny_shape(h, w) != (0, 0) for h, w in bs.level_sizes(64, 129, 0.75, 3)[1:])
    assert bs.tiny_shape(33, 70) != (0, 0) and bs.tiny_shape(34, 70) != (0, 0)
    assert bs.tiny_shape(33, 260) == (0, 0) and bs.tiny_shape(34, 260) == (0, 0)


def test_the_restated_tiny_shape_is_the_librarys():
    """papof_sor_tiny_shape is host code: no device is touched"""
    from papteam_opticalflow_amd import capi
    seen = set()
    for c in bs.CASES:
        seen.update(bs.level_sizes(c.H, c.W, bs.params_of(c)["ratio"], c.levels))
    seen.update((h, w) for h in (1, 31, 63, 64, 65, 90) for w in (1, 64, 95, 96, 97, 128, 129, 200))
    for h, w in sorted(seen):
        assert bs.tiny_shape(h, w) == capi.sor_tiny_shape(h, w), (h, w)


def test_the_split_of_a_collection_into_sub_batches():
    assert bs.split(3, 2, False) == [2, 1] and bs.split(7, 3, False) == [3, 2, 2] and bs.split(7, 5, False) == [5, 2]
    assert bs.split(4, 3, False) == [2, 2] and bs.split(5, 2, False) == [2, 2, 1] and bs.split(7, None, False) == [7]
    assert bs.split(3, 2, True) == [1, 1, 1] and bs.split(3, 3, True) == [1, 1, 1] and bs.split(5, 5, True) == [2, 2, 1]
    by = bs.BY_NAME
    assert bs.expected_stats(by["37x53 max 2 pairs 3"]) == dict(chains=1, chain_pairs=2, singles=1, reruns=0)
    assert bs.expected_stats(by["37x53 max 2 pairs 3"], fb=True) == dict(chains=3, chain_pairs=6, singles=0, reruns=0)
    assert bs.expected_stats(by["37x53 max 5 pairs 7"], fb=True) == dict(chains=4, chain_pairs=14, singles=0, reruns=0)
    assert bs.expected_stats(by["902x24, first single"]) == dict(chains=0, chain_pairs=0, singles=2, reruns=0)
    assert bs.expected_stats(by["101x173 repeated middle"]) == dict(chains=1, chain_pairs=3, singles=0, reruns=1)
    # the repeated pair as the one-pair remainder: a single call from the start, forward-only; a chain of its own and a re-run
    # with the backward pairs
    assert bs.expected_stats(by["101x173 repeated remainder"]) == dict(chains=1, chain_pairs=2, singles=1, reruns=0)
    assert bs.expected_stats(by["101x173 repeated remainder"], fb=True) == dict(chains=3, chain_pairs=6, singles=0, reruns=1)
    # 37 x 53: every level has at most 4096 pixels, the chain looks at all of them and proves the repeated pair's guard open
    assert bs.repeated_pair_is_rerun(by["101x173 repeated first"]) and not bs.repeated_pair_is_rerun(by["37x53 repeated first"])
    assert bs.expected_stats(by["37x53 repeated middle"], fb=True) == dict(chains=1, chain_pairs=6, singles=0, reruns=0)


def test_flow_batch_refuses_mixed_dtypes():
    """Papof.flow_batch took the dtype from frames[0] alone: a uint8 frame behind a float64 one went in as 0..255.  The check
    stands before the handle or the library is touched."""
    from papteam_opticalflow_amd import capi
    f64, u8 = np.zeros((8, 9, 3)), np.zeros((8, 9, 3), np.uint8)
    for frames in ([f64, u8], [u8, f64], [f64, f64, u8], [f64.astype(np.float32), u8], [f64.astype(np.int32)] * 2):
        with pytest.raises(ValueError, match="all uint8 or all floating"):
            capi.Papof.flow_batch(None, frames, 2)
    assert capi.batch_frames_are_u8([u8, u8]) is True and capi.batch_frames_are_u8(np.stack([u8, u8])) is True
    assert capi.batch_frames_are_u8([f64, f64.astype(np.float32)]) is False and capi.batch_frames_are_u8(np.stack([f64, f64])) is False
