"""Build-time check of k_flow_system's generated gfx950 code (no GPU needed): what its occupancy and its gathers rest on.
  * every instantiation allocates at most 168 VGPRs (three workgroups of four waves per CU);
  * the non-batched instantiations use no scratch;
  * the channel loop of the 5-plane skewed instantiation (the headline's) loads each footprint row of the bilinear taps as ONE
    16-byte load -- two rows for each of the three slots of pixels -- and holds no 8-byte load beyond frame 1's values of
    the pixels that leave the image (3), the guard's witness (1) and the smoothed frame 1 (2): no 8-byte gather of frame 2.
Read from the assembly the build saved beside the object (csrc/.build, exactly the shipped code); compiled here when that
is missing or older than the source."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "papteam_opticalflow_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_census  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{demangled short name: isa_census entry} of the k_flow_system instantiations"""
    src = os.path.join(CSRC, "kernels.hip")
    asm = os.path.join(CSRC, ".build", "kernels", "kernels-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm) or os.path.getmtime(asm) < os.path.getmtime(src):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        asm = str(tmp_path_factory.mktemp("fs") / "kernels.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "--offload-device-only", "-S", "-o", asm, src],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    ks = isa_census.kernels(asm)
    out = {}
    for n in ks:
        if "k_flow_system" in n:  # <PLANES, SKEW, BATCH, W1> in the mangled name
            m = re.search(r"13k_flow_systemILi(\d+)ELb([01])ELb([01])ELb([01])EE", n)
            assert m, n
            out[(int(m.group(1)), m.group(2) == "1", m.group(3) == "1", m.group(4) == "1")] = ks[n]
    return out


def test_every_instantiation_is_there_and_fits_three_workgroups_per_cu(kernels):
    want = {(p, s, b, w1) for p in (3, 5) for s in (False, True) for b in (False, True) for w1 in (False, True)}
    assert set(kernels) == want, sorted(set(kernels) ^ want)
    for key, k in sorted(kernels.items()):
        print(key, "VGPRs", k["vgpr"], "scratch", k["scratch"])
        assert k["vgpr"] <= 168, (key, k["vgpr"])


def test_the_single_pair_instantiations_have_no_scratch(kernels):
    for key, k in sorted(kernels.items()):
        if not key[2]:
            assert k["scratch"] == 0 and k.get("spills", 0) == 0, (key, k["scratch"], k.get("spills"))


def _channel_loop(body):
    """the instructions of the smallest loop (label ... backward branch to it) that holds three barriers: P1 | P2 | P3 | P4"""
    text = body["text"]
    label_at = {}
    for i, ln in enumerate(text):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    best = None
    for i, ln in enumerate(text):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and label_at.get(m.group(1), i) < i:
            span = text[label_at[m.group(1)]:i + 1]
            if sum(1 for s in span if s.strip().startswith("s_barrier")) == 3 and (best is None or len(span) < len(best)):
                best = span
    assert best is not None, "no loop with three barriers"
    return [s.strip().split()[0] for s in best if s.startswith("\t") and not s.strip().startswith((";", "."))]


def test_the_channel_loop_loads_each_footprint_row_once(kernels):
    ops = _channel_loop(kernels[(5, True, False, False)])
    x4 = [o for o in ops if o.endswith("load_dwordx4")]
    x2 = [o for o in ops if o.endswith("load_dwordx2") and not o.startswith(("s_", "ds_"))]
    other = [o for o in ops if "load" in o and o.startswith(("global_", "flat_", "buffer_")) and o not in x4 + x2]
    print("channel loop: %d instructions, 16-byte loads %d, 8-byte loads %d, others %s" % (len(ops), len(x4), len(x2), other))
    assert len(x4) == 6, x4  # three slots of pixels x two footprint rows
    assert len(x2) <= 6 and not other, (x2, other)  # frame 1's value per slot, the witness, the smoothed frame 1 (2)
