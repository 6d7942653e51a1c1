"""Interpreter twin of tests/test_gpu_render.py::test_training_gradients_aligned_at_general_sample_counts: the package's host
layer on CPU tensors against the CPU SIMT interpreter build of the kernels (tests.emu.host_on_emu), the same case body
(tests/render_step_case.py) and the same bounds -- one render_rays training step at 40 + 33 samples per ray (rays that
straddle the 128-sample blocks, an odd sample total) against the gate- and sample-aligned CPU oracle.  What the
interpreter cannot show -- unaligned vector accesses, buffer-store windows, real wave shuffles -- is the GPU test's."""
import json

import pytest

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("mode,options", [("fp32", {}), ("resident", {}), ("fp32", dict(shared_net=True, attached=True))],
                         ids=["fp32", "resident", "fp32_shared_net_attached"])
def test_training_gradients_aligned_at_40_plus_33_samples(mode, options):
    """(one resident case only: the resident kernels are the slow ones on the interpreter)"""
    from scnerf_amd.functional import host_linspace
    from tests import render_step_case as C
    from tests.emu.host_on_emu import emulated_device
    with emulated_device(mode):
        R = C.modules()
        saved = R["ops"].wgrad_arithmetic()
        R["ops"].wgrad_arithmetic("fp32" if mode == "fp32" else "half")
        try:
            entry = C.aligned_gradients_case(R, 4, "xavier", mode, host_linspace, sc=40, sf=33, device="cpu", **options)
        finally:
            R["ops"].wgrad_arithmetic(saved)
            # (the parity report is the GPU's: the interpreter's figures go to the test's output only)
            C.REPORT.pop(C.report_key(4, "xavier", mode, False, 40, 33, **options), None)
    print("\n4x(40+33) %s %s: %s" % (mode, options, json.dumps(entry)))
