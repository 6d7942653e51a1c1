"""Interpreter twin of tests/test_gpu_npp_occupancy.py: ops.inference_occupancy_nerfpp (csrc/npp_occupancy.hip,
scnerf_amd/occupancy.py, nerfplusplus/ddp_model.py) under the CPU SIMT interpreter -- the kernels through the C ABI on numpy
buffers against the transcriptions of tests/npp_occupancy_reference.py, the NeRF++ node (the package's host layer on CPU
tensors, 24 rays x (16 + 12) samples, fused fp32 kernels; with the scale guard in the resident arithmetic) against the oracle
of tests/npp_occupancy_cases.py.  Everything for equality of bits.  The switch's own checks need no kernel; of the baking the
interpreter runs one pass of 64 cells."""
import numpy as np
import pytest

from tests import npp_occupancy_cases as C
from tests.emu import harness as H


class EmuRoute:
    """how the kernel cases hold buffers and call the C ABI on the interpreter"""
    @staticmethod
    def inp(a):
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def out(shape, dtype=np.float32):
        buf = np.full((shape[0] + 2,) + tuple(shape[1:]), C.SENTINEL if dtype == np.int32 else np.nan, dtype)
        return buf, buf[1:-1]

    @staticmethod
    def pinned_word():
        return np.full(1, C.SENTINEL, np.int32)

    @staticmethod
    def shifted(a):
        return a.reshape(-1)[1:]

    @staticmethod
    def size(name, n):
        return getattr(H.lib(), name)(n)

    @staticmethod
    def call(name, *args):
        H.call(name, *args, None)

    @staticmethod
    def status(name, *args):
        return H.lib_call_status(name, *args, None)

    @staticmethod
    def host(buf):
        return buf

    @staticmethod
    def sync():
        pass


@pytest.fixture(autouse=True)
def _blocks_on_the_calling_thread(monkeypatch):
    """(tests/test_emu_occupancy.py: many small launches, one worker, the fiber stacks reused)"""
    monkeypatch.setenv("SIMT_EMU_THREADS", "1")


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    O.inference_occupancy_nerfpp("off")
    O.inference_occupancy("off")
    O.inference_skip_background("off")
    yield O
    O.inference_occupancy_nerfpp("off")
    O.inference_occupancy("off")
    O.inference_skip_background("off")


def test_the_switch_the_spaces_and_the_state_dict(ops):
    C.validation(ops)


@pytest.mark.emu
@pytest.mark.parametrize("kind", C.GRIDS)
@pytest.mark.parametrize("P", C.SIZES)
def test_compaction_and_expansion_equal_the_transcription(P, kind):
    C.check_compact4_and_expand(EmuRoute, P, kind)


@pytest.mark.emu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_inverted_probe_points_equal_the_transcription(k):
    C.check_probe_points_inverted(EmuRoute, k)


@pytest.mark.emu
def test_bad_arguments_are_status_codes():
    C.argument_checks(EmuRoute)


@pytest.mark.emu
def test_both_grids_mixed_equal_the_oracle(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.mixed_case(ops, "cpu", "fp32")


@pytest.mark.emu
@pytest.mark.parametrize("which", ["fg", "bg"])
def test_one_grid_alone_mixed_all_set_none_set(ops, which, monkeypatch):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.one_grid_case(ops, "cpu", "fp32", which, monkeypatch)


@pytest.mark.emu
def test_nothing_live_launches_no_network(ops, monkeypatch):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.nothing_live_case(ops, "cpu", "fp32", monkeypatch)


@pytest.mark.emu
def test_with_skip_background_equals_the_composition_by_hand(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.with_skip_background_case(ops, "cpu", "fp32", extremes=False)


@pytest.mark.emu
def test_with_the_scale_guard_on(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("resident"):
        C.mixed_case(ops, "cpu", "resident", guard="fallback")


@pytest.mark.emu
def test_calls_with_gradients_and_the_euclidean_switch_do_not_notice(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.tracking_call_case(ops, "cpu", "fp32")
        C.euclidean_switch_is_ignored_case(ops, "cpu", "fp32")


@pytest.mark.emu
def test_stale_and_foreign_networks_and_one_baking_pass(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.one_baking_pass_case(ops, "cpu")
        C.stale_and_foreign_case(ops, "cpu")


@pytest.mark.emu
def test_render_single_image_level_by_level(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.render_single_image_case(ops, "cpu", "fp32", "cpu")
