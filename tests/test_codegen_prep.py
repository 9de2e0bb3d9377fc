"""Build-time check of the preparation's newest kernels in the generated gfx950 code (no GPU needed):
  * k_smooth_resize<1 .. 4> (csrc/kernels.hip, one pyramid level per launch) are all there, have no private segment and spill
    nothing, keep their registers low enough for four workgroups of four waves per CU at the widest half-width, and hold only
    the 256 bytes of the tile's source positions as fixed LDS (the staged footprint is sized per launch);
  * k_bicubic_grad and k_bicubic_grad3 (the final warp) have no private segment either, the three-channel one within the 96
    registers of five waves per SIMD, and take no derivative plane: five global buffers and the phase stamp among their kernel
    arguments where k_bicubic<false> has three more (gx, gy, gxy), and 16 eight-byte loads per channel, all from frame 2.
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
def asm(tmp_path_factory):
    src = os.path.join(CSRC, "kernels.hip")
    asm = os.path.join(CSRC, ".build", "kernels", "kernels-hip-amdgcn-amd-amdhsa-gfx950.s")
    if not os.path.exists(asm) or os.path.getmtime(asm) < os.path.getmtime(src):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        asm = str(tmp_path_factory.mktemp("prep") / "kernels.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "--offload-device-only", "-S", "-o", asm, src],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    return asm


@pytest.fixture(scope="module")
def every(asm):
    return isa_census.kernels(asm)


@pytest.fixture(scope="module")
def kernels(every):
    """{half-width F: isa_census entry} of the k_smooth_resize<F> instantiations"""
    out = {}
    for n, k in every.items():
        m = re.search(r"15k_smooth_resizeILi(\d+)EE", n)
        if m:
            out[int(m.group(1))] = k
    return out


def test_every_half_width_is_there(kernels):
    assert sorted(kernels) == [1, 2, 3, 4]


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_no_private_segment_and_four_workgroups_per_cu(kernels, f):
    k = kernels[f]
    print("k_smooth_resize<%d>: VGPRs %d SGPRs %d scratch %d spills %d fixed LDS %d" %
          (f, k["vgpr"], k["sgpr"], k["scratch"], k.get("spills", 0), k["lds"]))
    assert k["scratch"] == 0 and k.get("spills", 0) == 0, (k["scratch"], k.get("spills"))
    assert k["vgpr"] <= 128, k["vgpr"]  # 512 registers per SIMD lane / 128 = 4 waves per SIMD: four workgroups per CU
    assert k["lds"] == 2 * 16 * 8, k["lds"]  # pos[2][kSrT]


def test_three_barriers_and_no_division_beside_the_positions(kernels):
    """the source positions are divided once per tile column and once per tile row and shared through LDS: two fp64
    reciprocals in the kernel's text (resize_pos along x and along y), three barriers (positions | staged cells | h pass)"""
    for f, k in sorted(kernels.items()):
        ops = [s.split()[0] for s in k["body"]]
        assert ops.count("s_barrier") == 3, (f, ops.count("s_barrier"))
        assert sum(o.startswith("v_rcp_f64") for o in ops) == 2, (f, [o for o in ops if o.startswith("v_rcp")])


def _one(every, pattern):
    names = [n for n in every if re.search(pattern, n)]
    assert len(names) == 1, (pattern, names)
    return names[0]


def _global_buffers(asm, symbol):
    """how many of the kernel arguments of `symbol` are global buffers, from its metadata entry"""
    text = open(asm).read()
    entries = re.split(r"\n  - \.agpr_count:", text[text.index("amdhsa.kernels:"):])
    mine = [e for e in entries if re.search(r"\n    \.name:\s+%s\n" % re.escape(symbol), e)]
    assert len(mine) == 1, symbol
    return re.findall(r"\.value_kind:\s+(\w+)", mine[0]).count("global_buffer")


GRAD, GRAD3, PLANES = r"14k_bicubic_gradE", r"15k_bicubic_grad3E", r"9k_bicubicILb0EE"


@pytest.mark.parametrize("pattern,vgprs", [(GRAD, 128), (GRAD3, 96)])
def test_the_final_warp_has_no_private_segment(every, pattern, vgprs):
    k = every[_one(every, pattern)]
    print(pattern, "VGPRs", k["vgpr"], "scratch", k["scratch"], "spills", k.get("spills", 0))
    assert k["scratch"] == 0 and k.get("spills", 0) == 0, (k["scratch"], k.get("spills"))
    assert k["vgpr"] <= vgprs, k["vgpr"]


def test_the_final_warp_takes_no_derivative_plane(asm, every):
    n_planes = _global_buffers(asm, _one(every, PLANES))
    for pattern in (GRAD, GRAD3):
        n = _global_buffers(asm, _one(every, pattern))
        print("global-buffer arguments: %s %d, k_bicubic<false> %d" % (pattern, n, n_planes))
        assert n == 6  # im1, im2, vx, vy, out, stamp
        assert n_planes == n + 3  # ... and gx, gy, gxy


def test_sixteen_loads_per_channel(every):
    def loads(pattern):
        ops = [s.split()[0] for s in every[_one(every, pattern)]["body"]]
        got = [o for o in ops if o.startswith(("global_load", "flat_load", "buffer_load"))]
        assert all(o.endswith("dwordx2") for o in got), got
        return len(got)
    # beside the channels' loads: vx, vy, and frame 1's value in the loop of the pixels that leave the image
    print("loads in the text:", loads(PLANES), loads(GRAD), loads(GRAD3))
    assert loads(GRAD) == loads(PLANES) == 2 + 1 + 16
    assert loads(GRAD3) == 2 + 1 + 3 * 16  # the three channels unrolled
