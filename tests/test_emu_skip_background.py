"""Interpreter twin of tests/test_gpu_skip_background.py: ops.inference_skip_background -- the two kernels behind it and
the NeRF++ node with the switch on --, the package's host layer on CPU tensors against the CPU SIMT interpreter build of
the kernels, the same case bodies (tests/skip_background_case.py) and the same equalities.  The node cases run 24 rays x
(16 + 12) samples on the fused fp32 kernels, which the interpreter runs fastest; the mixed case also in the resident
arithmetic.  The switch's own checks, the host layer's refusal of CPU tensors and the fp64 bound need no kernel."""
import numpy as np
import pytest

from tests import nerfpp_reference as NR
from tests import skip_background_case as C


class EmuRoute:
    """how the kernel cases hold buffers and call the C ABI on the interpreter (tests/test_emu_nerfpp.py's, plus status())"""
    @staticmethod
    def inp(a):
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def out(shape, dtype=np.float32):
        buf = np.full((shape[0] + 2,) + tuple(shape[1:]), NR.INT_GUARD if dtype == np.int32 else np.nan, dtype)
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        from tests.emu import harness as H
        H.call(name, *args, None)

    @staticmethod
    def status(name, *args):
        from tests.emu import harness as H
        return H.lib_call_status(name, *args, None)

    @staticmethod
    def host(buf):
        return buf


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = O.inference_skip_background()
    O.inference_skip_background("off")
    yield O
    O.inference_skip_background("off" if before is None else before)


SIZE_IDS = ["sf%d_sb%d" % s for s in NR.COMP_SIZES]


def test_the_switch_validates_its_argument(ops, monkeypatch):
    C.switch_validation(ops, monkeypatch)


def test_cpu_tensors_are_rejected_by_the_host_layer(ops):
    C.cpu_tensors_are_rejected(ops)


@pytest.mark.parametrize("size", NR.COMP_SIZES, ids=SIZE_IDS)
def test_the_bound_holds_on_the_fp64_oracle(size):
    C.bound_in_fp64(size)


@pytest.mark.emu
@pytest.mark.parametrize("size", NR.COMP_SIZES, ids=SIZE_IDS)
def test_fg_lambda_is_the_compositing_kernels_bg_lambda(size):
    C.fg_lambda_case(EmuRoute, size)


@pytest.mark.emu
@pytest.mark.parametrize("pattern", C.SKIP_PATTERNS)
@pytest.mark.parametrize("size", NR.COMP_SIZES, ids=SIZE_IDS)
def test_composite_fwd_skip_equals_composite_fwd_on_zeroed_rows(size, pattern):
    C.composite_skip_case(EmuRoute, size, pattern)


@pytest.mark.emu
def test_bad_arguments_are_status_codes():
    C.argument_checks(EmuRoute)


@pytest.mark.emu
@pytest.mark.parametrize("mode", ["fp32", "resident"])
def test_live_rays_as_switch_off_skipped_rays_without_background(ops, mode):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device(mode):
        C.mixed_case(ops, "cpu", mode)


@pytest.mark.emu
def test_with_the_scale_guard_on_live_rays_are_the_switch_off_call_on_them(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("resident"):
        C.guarded_case(ops, "cpu", "fallback")


@pytest.mark.emu
def test_nothing_skipped_and_everything_skipped(ops, monkeypatch):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.nothing_skipped_case(ops, "cpu", "fp32")
        C.everything_skipped_case(ops, "cpu", "fp32", monkeypatch)


@pytest.mark.emu
def test_a_call_that_tracks_gradients_does_not_notice(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.tracking_call_case(ops, "cpu", "fp32")


@pytest.mark.emu
def test_render_single_image_level_by_level(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.render_single_image_case(ops, "cpu", "fp32", "cpu")
