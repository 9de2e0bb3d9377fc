import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


# Streams whose kernels WAIT FOR EACH OTHER on the device with no host-side launch order -- the ranks of a group on the RCCL stand-in of
# tests/fake_rccl that share ONE device, and the strips of one solve (PAPOF_STRIPS) -- need a hardware queue each: two streams
# that share a hardware queue run their kernels one after the other, and a kernel in front of the one it waits for would never
# end (on a multi-GPU node every rank has a device to itself).  (The local transport's exact-order band split does not: its
# ranks' solver kernels are enqueued in producer order from the host, tiles.hip: turn_wait.)  The suite does not raise the HIP
# runtime's limit on hardware queues per process; a test that needs more than the limit allows is skipped, with the count in
# the reason -- the multi-rank protocols are rehearsed over gloo on the CPU as well.
HIP_DEFAULT_HW_QUEUES = 4  # the HIP runtime's default limit when the environment does not set one


def hw_queue_limit():
    """hardware queues the HIP runtime of this process may open"""
    v = os.environ.get("GPU_MAX_HW_QUEUES")
    return int(v) if v else HIP_DEFAULT_HW_QUEUES


def require_hw_queues(need, what):
    """skip unless the process may open `need` hardware queues: one for every stream of `what`, whose kernels wait for each
    other on the device"""
    if hw_queue_limit() < need:
        pytest.skip("%s wait for each other on the device: they need %d hardware queues, the HIP runtime of this process "
                    "may open %d" % (what, need, hw_queue_limit()))


def require_queues_for_ranks(nranks):
    """skip unless `nranks` ranks on one device (two streams each, plus the runtime's null stream) get a queue per stream"""
    if nranks > 1:
        require_hw_queues(2 * nranks + 1, "%d ranks on one device" % nranks)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: > 15 s of CPU work; enabled by PAPOF_SLOW=1")


@pytest.hookimpl(hookwrapper=True)
def pytest_runtest_makereport(item, call):
    """keeps each phase's report on the test item (rep_setup / rep_call / rep_teardown) for fixtures' teardown"""
    outcome = yield
    rep = outcome.get_result()
    setattr(item, "rep_" + rep.when, rep)


@pytest.fixture(scope="session")
def oracle():
    from _libs import OracleLib
    return OracleLib()


FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


@pytest.fixture(params=["local", "rccl"])
def tile_group(request, monkeypatch):
    """The class that builds a multi-rank tile group inside this process, once per TRANSPORT of csrc/tiles.hip:
    `local`  LocalTileGroup: device copies behind hipStreamSynchronize + two host barriers of all ranks per exchange;
    `rccl`   RcclTileGroup: the RCCL transport itself (papof_tiles_create, ncclSend / ncclRecv groups on the rank's stream, no host
             synchronisation, barrier() a no-op) bound to tests/fake_rccl -- a stand-in with RCCL's stream-ordered semantics whose
             ranks may share the one device of this box.  Afterwards the stand-in must have carried messages and seen no error
             (a receive or send that gave up, byte counts that disagree)."""
    import ctypes
    from papteam_opticalflow_amd import capi
    if request.param == "local":
        yield capi.LocalTileGroup
        return
    assert os.path.exists(FAKE_RCCL), "tests/fake_rccl/libfake_rccl.so is not built (__graft_entry__.build())"
    # The ranks' group kernels wait for each other on the device, so every rank's stream needs a hardware queue of its own (see the
    # top of this file): give back the streams that earlier tests left pooled -- flow_collection()'s handles, the default handle
    import gc
    import papteam_opticalflow_amd as pkg
    for pool in pkg._collection_handles.values():
        for hnd in pool:
            hnd.close()
        pool.clear()
    if pkg._default is not None:
        pkg._default.close()
        pkg._default = None
    gc.collect()
    monkeypatch.setenv("PAPOF_RCCL_LIB", FAKE_RCCL)
    monkeypatch.setenv("PAPOF_TILES_TIMEOUT_S", os.environ.get("PAPOF_TILES_TIMEOUT_S", "40"))
    fake = ctypes.CDLL(FAKE_RCCL)
    fake.fake_rccl_error_count.restype = ctypes.c_uint
    fake.fake_rccl_reset_errors()
    before = (ctypes.c_long * 3)()
    fake.fake_rccl_stats(before)
    capi.RcclTileGroup.standin = fake
    yield capi.RcclTileGroup
    after = (ctypes.c_long * 3)()
    fake.fake_rccl_stats(after)
    kinds = (ctypes.c_uint * 4)()
    fake.fake_rccl_error_kinds(kinds)
    fake.fake_rccl_reset_errors()
    rep = getattr(request.node, "rep_call", None)
    if rep is not None and rep.skipped:  # the group was never built (require_queues_for_ranks)
        return
    assert kinds[0] == 0 or getattr(request.node, "_standin_errors_expected", False), ("the RCCL stand-in saw %d errors: %d sends and %d receives gave up, %d messages whose two ends disagree "
                           "about the byte count" % tuple(kinds))
    if not getattr(request.node, "_standin_may_be_idle", False):
        assert after[1] > before[1] and after[2] > before[2], "no message went through the RCCL stand-in"
    print("RCCL stand-in: %d group kernels, %d sends, %d receives" % tuple(after[i] - before[i] for i in range(3)))
