"""BASELINE.json configs[0] (plumbing): the reference's caller (Code/Serial/OpticalFlowCalculation.py) reaches this
repository's drop-in `pyflow` module by module name alone, with frames it decodes itself.

The caller's side is restated here on the committed frames (tests/golden/frames), in a fresh process whose PYTHONPATH
holds only the drop-in's directory: PIL -> np.array -> astype(float) / 255., then the positional call
`pyflow.coarse2fine_flow(im1, im2, pyramidLevels)` (OpticalFlowCalculation.py:65-73) and what the caller does with the
result (`u[..., None]` concatenation, the 'Total C++ Execution' timer).  Without a device the call must fail THERE with
the loud no-device error -- which proves the binding: same module name, same positional signature, float64 HWC arrays
from PIL.  The full contract of the result is checked on the GPU by
tests/test_gpu_parity.py::test_pyflow_dropin_entry_point.
"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = os.path.join(ROOT, "tests", "golden", "frames", "240")

DRIVER = r'''
import os, sys
import numpy as np
from PIL import Image
import pyflow
frames = sys.argv[1]
im1 = np.array(Image.open(os.path.join(frames, "frame_00001.jpg")))
im2 = np.array(Image.open(os.path.join(frames, "frame_00002.jpg")))
im1 = im1.astype(float) / 255.
im2 = im2.astype(float) / 255.
print("MODULE", os.path.basename(os.path.dirname(os.path.abspath(pyflow.__file__))))
try:
    timingDictionary, u, v, im2W = pyflow.coarse2fine_flow(im1, im2, 2)
    flow = np.concatenate((u[..., None], v[..., None]), axis=2)
    print("RESULT ok", flow.shape, im2W.shape, float(timingDictionary["Total C++ Execution"]) > 0)
except RuntimeError as e:
    print("RESULT RuntimeError", e)
'''


def test_reference_style_caller_reaches_our_pyflow(tmp_path):
    import __graft_entry__
    lib = os.path.join(ROOT, "papteam_opticalflow_amd", "csrc", "libpapof.so")
    if not os.path.exists(lib):
        __graft_entry__.build()
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1",
               PYTHONPATH=os.path.join(ROOT, "papteam_opticalflow_amd", "dropin"))
    out = subprocess.run([sys.executable, "-c", DRIVER, FRAMES], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    text = out.stdout + out.stderr
    assert "MODULE dropin" in text, text[-3000:]
    have_gpu = ctypes.CDLL(lib).papof_device_count() > 0
    if have_gpu:
        assert "RESULT ok (135, 240, 2) (135, 240, 3) True" in text, text[-3000:]
    else:
        assert "RESULT RuntimeError" in text and "no usable gfx950 device" in text, text[-3000:]
