"""ops.inference_skip_background on the GPU (pytest -m gpu): the two kernels behind it (scnerf_npp_fg_lambda,
scnerf_npp_composite_fwd_skip) launched stand-alone through the C ABI, and the NeRF++ node and render_single_image with the
switch on, in the fp32, resident and one-product arithmetics.  The case bodies are tests/skip_background_case.py's, shared
with the interpreter twin tests/test_emu_skip_background.py; every comparison but the error bound is for equality of bits."""
import numpy as np
import pytest
import torch

from tests import nerfpp_reference as NR
from tests import skip_background_case as C

pytestmark = pytest.mark.gpu
MODES = ["fp32", "resident", "fast"]


class GpuRoute:
    """how the kernel cases hold buffers and call the C ABI on the device (tests/test_gpu_nerfpp_kernels.py's, plus status())"""
    @staticmethod
    def inp(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def out(shape, dtype=np.float32):
        buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[1:-1]

    @staticmethod
    def status(name, *args):
        from scnerf_amd import _capi
        return getattr(_capi.load(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], _capi.current_stream())

    @staticmethod
    def call(name, *args):
        from scnerf_amd import _capi
        _capi.check(GpuRoute.status(name, *args), name)

    @staticmethod
    def host(buf):
        return buf.cpu().numpy()


@pytest.fixture
def ops():
    assert torch.cuda.is_available()
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
def test_fg_lambda_is_the_compositing_kernels_bg_lambda(ops, size):
    C.fg_lambda_case(GpuRoute, size)


@pytest.mark.parametrize("pattern", C.SKIP_PATTERNS)
@pytest.mark.parametrize("size", NR.COMP_SIZES, ids=SIZE_IDS)
def test_composite_fwd_skip_equals_composite_fwd_on_zeroed_rows(ops, size, pattern):
    C.composite_skip_case(GpuRoute, size, pattern)


def test_bad_arguments_are_status_codes(ops):
    C.argument_checks(GpuRoute)


@pytest.mark.parametrize("mode", MODES)
def test_live_rays_as_switch_off_skipped_rays_without_background(ops, mode):
    C.mixed_case(ops, "cuda", mode)


@pytest.mark.parametrize("guard", ["fallback", "report"])
def test_with_the_scale_guard_on_live_rays_are_the_switch_off_call_on_them(ops, guard):
    C.guarded_case(ops, "cuda", guard)


@pytest.mark.parametrize("mode", MODES)
def test_nothing_skipped(ops, mode):
    C.nothing_skipped_case(ops, "cuda", mode)


@pytest.mark.parametrize("mode", MODES)
def test_everything_skipped_launches_no_background(ops, mode, monkeypatch):
    C.everything_skipped_case(ops, "cuda", mode, monkeypatch)


@pytest.mark.parametrize("mode", ["fp32", "resident"])
def test_a_call_that_tracks_gradients_does_not_notice(ops, mode):
    C.tracking_call_case(ops, "cuda", mode)


@pytest.mark.parametrize("mode", MODES)
def test_render_single_image_level_by_level(ops, mode):
    C.render_single_image_case(ops, "cuda", mode, 0)
