"""GPU twin of the fp64 cases of tests/test_emu_nerfpp.py (pytest -m gpu): the per-ray kernels of csrc/nerfpp.hip launched
stand-alone through the C ABI on the cases, references, bounds and guard rows of tests/nerfpp_reference.py -- the hardware's
side of what the interpreter shows: wave shuffles in a partial pass, LDS atomics, the device's expf / asinf / sinf / cosf,
dead waves behind the workgroup barrier.  Plus, per autograd wrapper of scnerf_amd.nerfplusplus.ddp_train_nerf, that the
public surface is that same launch."""
import numpy as np
import pytest
import torch

from tests import nerfpp_reference as NR

pytestmark = pytest.mark.gpu


class GpuRoute:
    """how tests/nerfpp_reference.py's run_* functions hold buffers and call the C ABI on the device"""
    @staticmethod
    def inp(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    @staticmethod
    def out(shape, dtype=np.float32):
        if dtype == np.int32:
            buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), NR.INT_GUARD, dtype=torch.int32, device="cuda")
        else:
            buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        from scnerf_amd import _capi
        st = getattr(_capi.load(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], _capi.current_stream())
        _capi.check(st, name)

    @staticmethod
    def host(buf):
        return buf.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available()


@pytest.mark.parametrize("case", NR.COMP_CASES, ids=lambda c: "sf%d_sb%d_%s" % (c[0], c[1], "all" if c[2] else "rgb"))
def test_composite_any_sample_count_vs_fp64(case):
    """tests/test_emu_nerfpp.py::test_composite_any_sample_count_vs_fp64 on the GPU: same inputs, reference and bound"""
    inp, _, _ = NR.composite_references(case)
    NR.check_composite(case, NR.run_composite(GpuRoute, inp, case[2]))


@pytest.mark.parametrize("size", NR.GEO_SIZES, ids=lambda s: "sf%d_sb%d" % s)
def test_geometry_grazing_and_near_centre_rays_vs_fp64(size):
    inp, _, _ = NR.geometry_references(size)
    NR.check_geometry(size, NR.run_geometry(GpuRoute, inp))


def test_points_outside_forward_without_foreground():
    inp, _, _ = NR.geometry_references(NR.GEO_SIZES[0])
    NR.check_points_outside(NR.GEO_SIZES[0], NR.run_points_outside(GpuRoute, inp))


@pytest.mark.parametrize("case", NR.SAMPLER_CASES, ids=lambda c: "m%d_ns%d" % c)
def test_sampler_any_bin_count(case):
    """forward bit for bit against the fp32 oracle, which runs on the CPU beside it; g_bins under the bound"""
    inp = NR.sampler_references(case)[0]
    NR.check_sampler(case, NR.run_sampler(GpuRoute, inp))


@pytest.mark.parametrize("s", NR.JITTER_S)
def test_jitter_any_sample_count(s):
    NR.check_jitter(s, NR.run_jitter(GpuRoute, NR.jitter_references(s)[0]))


# ---- the autograd wrappers are the same launches: same bits, forward and backward -------------------------------------------
def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def same_bits(t, direct, what):
    np.testing.assert_array_equal(bits(t), np.ascontiguousarray(direct, np.float32).view(np.int32), err_msg=what)


def test_intersect_sphere_wrapper_is_the_same_launch():
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    inp, _, _ = NR.geometry_references(NR.GEO_SIZES[1])
    direct = NR.run_geometry(GpuRoute, inp)
    o, d = GpuRoute.inp(inp["ray_o"]).requires_grad_(True), GpuRoute.inp(inp["ray_d"]).requires_grad_(True)
    far = TR.intersect_sphere(o, d)
    (far * GpuRoute.inp(inp["g_far"])).sum().backward()
    same_bits(far, direct["far"], "far")
    same_bits(o.grad, direct["gi_o"], "g_o")
    same_bits(d.grad, direct["gi_d"], "g_d")


def test_perturb_samples_wrapper_is_the_same_launch():
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    inp, _ = NR.jitter_references(65)
    direct = NR.run_jitter(GpuRoute, inp)
    z = GpuRoute.inp(inp["z"]).requires_grad_(True)
    out = TR.perturb_samples(z, _t_rand=GpuRoute.inp(inp["t"]))
    (out * GpuRoute.inp(inp["g"])).sum().backward()
    same_bits(out, direct["out"], "perturbed")
    same_bits(z.grad, direct["g_z"], "g_z")


def test_sample_pdf_wrapper_is_the_same_launch():
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    case = (62, 65)
    inp = NR.sampler_references(case)[0]
    direct = NR.run_sampler(GpuRoute, inp)
    b = GpuRoute.inp(inp["bins"]).requires_grad_(True)
    s = TR.sample_pdf(b, GpuRoute.inp(inp["weights"]), inp["u"].shape[1], _u=GpuRoute.inp(inp["u"]))
    (s * GpuRoute.inp(inp["g"])).sum().backward()
    same_bits(s, direct["samples"], "samples")
    same_bits(b.grad, direct["g_bins"], "g_bins")
