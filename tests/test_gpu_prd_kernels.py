"""GPU twin of tests/test_emu_prd_kernels.py (pytest -m gpu): the projected-ray-distance kernels of csrc/prd_loss.hip
launched stand-alone through the C ABI on the cases, float64 references, bounds and guards of tests/prd_reference.py -- the
hardware's side of what the interpreter shows: dead lanes in the wave reductions, global float atomics from up to 17
blocks, an empty grid, contracted arithmetic.  Plus the public wrappers with NeRF++'s axes."""
import types

import numpy as np
import pytest
import torch

from tests import prd_reference as PR

pytestmark = pytest.mark.gpu


def _ptr(t):
    """a tensor's address; of an empty view, the address it would start at (torch reports NULL for every empty tensor)"""
    if t.numel():
        return t.data_ptr()
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


class GpuRoute:
    """how tests/prd_reference.py's run functions hold buffers and call the C ABI on the device"""
    @staticmethod
    def inp(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.size:
            return torch.from_numpy(a).cuda()
        return torch.zeros((1,) + a.shape[1:], dtype=torch.from_numpy(a).dtype, device="cuda")[:0]    # empty, with an address

    @staticmethod
    def out(shape, dtype=np.float32):
        full = (shape[0] + 2,) + tuple(shape[1:])
        if dtype == np.uint8:
            buf = torch.full(full, PR.GUARD_BYTE, dtype=torch.uint8, device="cuda")
        else:
            buf = torch.full(full, float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        from scnerf_amd import _capi
        st = getattr(_capi.load(), name)(*[_ptr(a) if torch.is_tensor(a) else a for a in args], _capi.current_stream())
        _capi.check(st, name)

    @staticmethod
    def host(buf):
        return buf.cpu().numpy()


def launched(case):
    """the case's launches, once per session"""
    return PR._cached(("gpu", PR.CR._key(case)), lambda: PR.run(GpuRoute, PR.references(case)[0], case))


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available()
    yield
    PR.report()


@pytest.mark.parametrize("case", PR.CASES_BOTH + PR.CASES_GPU, ids=PR.case_id)
def test_prd_vs_fp64(case):
    """tests/test_emu_prd_kernels.py::test_prd_vs_fp64 on the GPU, plus an exact block, its neighbours, 4 and 17 blocks"""
    PR.check(case, launched(case))


@pytest.mark.parametrize("m", [65, 257])
@pytest.mark.parametrize("thr", [5.0, 1.0])
def test_nerfpp_axes_on_the_mirrored_scene_give_the_twin(thr, m):
    case = PR.prd_case(m, thr=thr, neg=0)
    PR.check_twin(case, launched(case), launched(PR.twin(case)))


@pytest.mark.parametrize("m", [65, 257])
def test_gradients_are_linear_in_the_incoming_gradient(m):
    case = PR.prd_case(m, g=-0.37)
    PR.check_linear(case, launched(case), launched(PR.prd_case(m)))


def test_one_direction_empty():
    PR.check(PR.EMPTY0, launched(PR.EMPTY0))


def test_nonfinite_errors_count_as_the_threshold_in_eval_mode():
    PR.run_and_check_nonfinite_eval(GpuRoute)


def test_empty_batch():
    """the device refuses a launch of zero blocks, which the interpreter does not see"""
    PR.run_and_check_empty(GpuRoute)


@pytest.mark.parametrize("m", [257, 4097])
def test_per_match_outputs_repeat_bit_for_bit(m):
    PR.run_twice_and_compare(GpuRoute, PR.prd_case(m))


def test_public_wrappers_with_nerfpp_axes():
    """proj_ray_dist_loss_single and filter_matches_with_gt with method="NeRF++" on the mirrored scene: the loss, n_match and
    keep-mask of method="NeRF" on the scene itself, and the gradient of K under the bound (the sign of K[0][0] and its undo)"""
    from scnerf_amd import prd_evaluation, ray_dist_loss
    case = PR.prd_case(65, neg=0)
    got = {}
    for c, method in ((case, "NeRF++"), (PR.twin(case), "NeRF")):
        inp, o64, o32, _, _ = PR.references(c)
        assert (inp["kps0"][:, 0] < PR.W_IMG).all() and (inp["kps1"][:, 0] < PR.W_IMG).all()      # (the wrapper asserts it)
        T = {k: torch.from_numpy(inp[k]).cuda() for k in PR.INPUTS}
        Kmat = T["K"].requires_grad_(True)
        args = types.SimpleNamespace(proj_ray_dist_threshold=c["thr"])
        rays0, rays1 = (T["rays0_o"], T["rays0_d"]), (T["rays1_o"], T["rays1_d"])
        loss, nm = ray_dist_loss.proj_ray_dist_loss_single(T["kps0"], T["kps1"], 0, 1, rays0, rays1, "train", "cuda", PR.H_IMG,
                                                           PR.W_IMG, args, intrinsic=Kmat, extrinsic=T["E2"], method=method)
        loss.backward()
        keep = prd_evaluation.filter_matches_with_gt(T["kps0"], T["kps1"], PR.W_IMG, PR.H_IMG, T["K"].detach(), T["E2"], rays0,
                                                     rays1, args, method, "cuda")
        got[method] = dict(loss=loss.detach().cpu().numpy().reshape(1), g_K=Kmat.grad.cpu().numpy(), n_match=nm,
                           keep=keep.cpu().numpy())
        PR.bound_check("prd", "wrapper-" + method, got[method], o64, o32, ("loss", "g_K"))
        assert nm == launched(c)["n_match"][0]
        # the filter's own constants: eps = 1e-6, one squared pixel
        flt = PR.classify(inp, dict(c, thr=1.0), PR.FILTER_EPS)
        assert not flt["bl"].any()
        np.testing.assert_array_equal(got[method]["keep"], flt["chir"] & flt["ok0"] & flt["ok1"])
    a, b = got["NeRF++"], got["NeRF"]
    assert a["n_match"] == b["n_match"] and a["n_match"] > 20
    np.testing.assert_array_equal(a["keep"], b["keep"])
    assert a["keep"].sum() > 20 and not a["keep"].all()
    PR.check_twin(case, dict(launched(case), loss=a["loss"]), dict(launched(PR.twin(case)), loss=b["loss"]))
