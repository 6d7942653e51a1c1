"""The projected-ray-distance kernels (csrc/prd_loss.hip: scnerf_prd_loss_fwd in both modes, scnerf_prd_loss_bwd,
scnerf_prd_filter) launched stand-alone through the C ABI on the CPU SIMT interpreter, against float64: the cases,
references, bounds and guard rows of tests/prd_reference.py, which tests/test_gpu_prd_kernels.py runs again on the GPU."""
import numpy as np
import pytest

from tests import prd_reference as PR
from tests.emu import harness as H

pytestmark = pytest.mark.emu


class EmuRoute:
    """how tests/prd_reference.py's run functions hold buffers and call the C ABI on the interpreter"""
    @staticmethod
    def inp(a):
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def out(shape, dtype=np.float32):
        buf = np.full((shape[0] + 2,) + tuple(shape[1:]), PR.GUARD_BYTE if dtype == np.uint8 else np.nan, dtype)
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        H.call(name, *args, None)

    @staticmethod
    def host(buf):
        return buf


def launched(case):
    """the case's launches, once per session"""
    return PR._cached(("emu", PR.CR._key(case)), lambda: PR.run(EmuRoute, PR.references(case)[0], case))


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    PR.report()


@pytest.mark.parametrize("case", PR.CASES_BOTH, ids=PR.case_id)
def test_prd_vs_fp64(case):
    """counts on both sides of the wave and block edges, both thresholds, both axis conventions, an incoming gradient far
    from 1, the planted rows: counts and verdicts exactly, masked rows exactly zero, loss (both modes) and gradients
    under the bound"""
    PR.check(case, launched(case))


@pytest.mark.parametrize("thr", [5.0, 1.0])
def test_nerfpp_axes_on_the_mirrored_scene_give_the_twin(thr):
    case = PR.prd_case(65, thr=thr, neg=0)
    PR.check_twin(case, launched(case), launched(PR.twin(case)))


def test_gradients_are_linear_in_the_incoming_gradient():
    case = PR.prd_case(65, g=-0.37)
    PR.check_linear(case, launched(case), launched(PR.prd_case(65)))


def test_one_direction_empty():
    """no match valid in direction 0: the loss is NaN as the reference's, direction 1 still gets its gradients"""
    PR.check(PR.EMPTY0, launched(PR.EMPTY0))


def test_nonfinite_errors_count_as_the_threshold_in_eval_mode():
    PR.run_and_check_nonfinite_eval(EmuRoute)


def test_empty_batch():
    PR.run_and_check_empty(EmuRoute)


def test_per_match_outputs_repeat_bit_for_bit():
    PR.run_twice_and_compare(EmuRoute, PR.prd_case(257))


@pytest.mark.parametrize("case", PR.CASES_BOTH + PR.CASES_GPU + [PR.EMPTY0], ids=PR.case_id)
def test_margin_of_the_borderline_rule_covers_the_fp32_oracle(case):
    """DELTA >= 8 x the fp32 oracle's worst relative error in L near the threshold, on every case of either route (the
    references assert that no case has a borderline match at m <= 257 and none more than 1 %)"""
    d = PR.measured_delta(PR.inputs(case), case)
    print("prd %s measured delta %.3g" % (PR.case_id(case), d))
    assert d <= PR.DELTA
