"""GPU twin of tests/test_emu_camera_kernels.py (pytest -m gpu): the camera kernels of csrc/camera_rays.hip launched
stand-alone through the C ABI on the cases, float64 references, bounds and guard rows of tests/camera_reference.py -- the
hardware's side of what the interpreter shows: dead lanes in the wave reductions, the LDS pre-reduction and its 48 KB
request, global float atomics, an empty grid.  Plus, per public wrapper, that the public surface is that same launch."""
import types

import numpy as np
import pytest
import torch

from tests import camera_reference as CR

pytestmark = pytest.mark.gpu


def _ptr(t):
    """a tensor's address; of an empty view, the address it would start at (torch reports NULL for every empty tensor)"""
    if t.numel():
        return t.data_ptr()
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


class GpuRoute:
    """how tests/camera_reference.py's run_* functions hold buffers and call the C ABI on the device"""
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
        buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        from scnerf_amd import _capi
        st = getattr(_capi.load(), name)(*[_ptr(a) if torch.is_tensor(a) else a for a in args], _capi.current_stream())
        _capi.check(st, name)

    @staticmethod
    def host(buf):
        return buf.cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def device():
    assert torch.cuda.is_available()
    yield
    CR.report()


@pytest.mark.parametrize("case", CR.RAYS_CASES, ids=CR.case_id)
def test_camera_rays_vs_fp64(case):
    """tests/test_emu_camera_kernels.py::test_camera_rays_vs_fp64 on the GPU: same inputs, reference and bound"""
    inp, _, _ = CR.rays_references(case)
    CR.check_rays(case, CR.run_rays(GpuRoute, inp, case))


@pytest.mark.parametrize("case", CR.NPP_CASES, ids=CR.case_id)
def test_npp_camera_rays_vs_fp64(case):
    inp, _, _ = CR.npp_references(case)
    CR.check_npp(case, CR.run_npp(GpuRoute, inp, case))


@pytest.mark.parametrize("case", CR.MATRICES_CASES, ids=CR.case_id)
def test_camera_matrices_vs_fp64(case):
    inp, _, _ = CR.matrices_references(case)
    CR.check_matrices(case, CR.run_matrices(GpuRoute, inp, case))


@pytest.mark.parametrize("case", CR.NDC_CASES, ids=CR.case_id)
def test_ndc_vs_fp64(case):
    inp, _, _ = CR.ndc_references(case)
    CR.check_ndc(case, CR.run_ndc(GpuRoute, inp, case))


@pytest.mark.parametrize("case", CR.PACK_CASES, ids=CR.case_id)
def test_pack_rays_vs_fp64(case):
    inp, _, _ = CR.pack_references(case)
    CR.check_pack(case, CR.run_pack(GpuRoute, inp, case))


@pytest.mark.parametrize("shape", CR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_grid_vs_fp64(shape):
    inp, _, _ = CR.upsample_references(shape)
    CR.check_upsample(shape, CR.run_upsample(GpuRoute, inp, shape))


@pytest.mark.parametrize("case", CR.PINHOLE_CASES, ids=CR.case_id)
def test_pinhole_rays_vs_fp64(case):
    inp, _, _ = CR.pinhole_references(case)
    CR.check_pinhole(case, CR.run_pinhole(GpuRoute, inp, case))


def test_empty_batches_return_zero_with_zeroed_gradients():
    """the device refuses a launch of zero blocks, which the interpreter does not see"""
    CR.run_and_check_empty(GpuRoute)


def test_per_ray_outputs_repeat_bit_for_bit():
    for case, refs, run in ((CR.rays_case(n=257), CR.rays_references, CR.run_rays),
                            (CR.rays_case(pose="perray"), CR.rays_references, CR.run_rays),
                            (CR.npp_case(n=257), CR.npp_references, CR.run_npp),
                            (CR.ndc_case(n=257), CR.ndc_references, CR.run_ndc),
                            (CR.pack_case(n=257), CR.pack_references, CR.run_pack)):
        inp = refs(case)[0]
        a, b = run(GpuRoute, inp, case), run(GpuRoute, inp, case)
        names = ("rays_o", "rays_d", "ndc_o", "ndc_d", "g_rays_o", "g_rays_d", "pack_o", "pack_d", "pack_v")
        CR.same_bits(a, b, names + (("d_extrinsic",) if case.get("pose") == "perray" else ()))


# ---- the public wrappers are the same launches: per-ray outputs bit for bit, accumulated gradients under the bound -----------
def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def camera_model(inp, mult, C, shape=CR.SHAPES[0], scale_o=CR.SCALE_O):
    """the package's learnable camera model holding the tensors of a case of tests/camera_reference.py"""
    from scnerf_amd.camera_dict import camera_dict
    gh, gw, Hh, Ww = shape
    assert (Hh // 10, Ww // 10) == (gh, gw)
    key = "pinhole_rot_noise_10k_rayo_rayd"
    args = types.SimpleNamespace(camera_model=key, grid_size=10, ray_o_noise_scale=scale_o, ray_d_noise_scale=CR.SCALE_D,
                                 extrinsics_noise_scale=CR.EXTR_SCALE, intrinsics_noise_scale=CR.INTR_SCALE[mult],
                                 multiplicative_noise=bool(mult))
    cm = camera_dict[key](torch.eye(4), [np.eye(4, dtype=np.float32)] * C, args, Hh, Ww)
    with torch.no_grad():
        for name, k in (("intrinsics_initial", "intr_init"), ("intrinsics_noise", "intr_noise"),
                        ("extrinsics_initial", "extr_init"), ("extrinsics_noise", "extr_noise"),
                        ("ray_o_noise", "grid_o"), ("ray_d_noise", "grid_d")):
            if k in inp:
                getattr(cm, name).copy_(torch.from_numpy(inp[k]))
    return cm.cuda()


def test_get_rays_kps_use_camera_with_per_ray_poses_is_the_same_launch():
    from scnerf_amd import get_rays
    case = CR.rays_case(pose="perray", kps="interior")
    inp, o64, o32 = CR.rays_references(case)
    direct = CR.run_rays(GpuRoute, inp, case)
    gh, gw, Hh, Ww = case["shape"]
    cm = camera_model(inp, case["mult"], case["C"])
    E = cuda(inp["E"]).requires_grad_(True)
    ro, rd = get_rays.get_rays_kps_use_camera(Hh, Ww, cm, cuda(inp["kps"]), extrinsic=E)
    ((ro * cuda(inp["g_o"])).sum() + (rd * cuda(inp["g_d"])).sum()).backward()
    assert E.grad.shape == (case["n"], 4, 4) and cm.extrinsics_noise.grad is None
    got = dict(rays_o=host(ro), rays_d=host(rd), d_extrinsic=host(E.grad))
    CR.same_bits(got, direct, tuple(got))
    acc = dict(d_intr_noise=host(cm.intrinsics_noise.grad), d_grid_o=host(cm.ray_o_noise.grad), d_grid_d=host(cm.ray_d_noise.grad))
    CR.bound_check("rays", "wrapper-" + CR.case_id(case), acc, o64, o32, tuple(acc))


def test_pack_ray_batch_is_the_same_launch():
    from scnerf_amd import camera_functional as CF
    case = CR.pack_case(n=257)
    inp, o64, o32 = CR.pack_references(case)
    direct = CR.run_pack(GpuRoute, inp, case)
    o, d, f = (cuda(inp[k]).requires_grad_(True) for k in ("o", "d", "f2"))
    cam = types.SimpleNamespace(focal_xy=lambda: f)              # the only thing pack_ray_batch asks of a camera model
    Hh, Ww = CR.NDC_HW
    batch = CF.pack_ray_batch(Hh, Ww, o, d, CR.PACK_NEAR_FAR[0], CR.PACK_NEAR_FAR[1], True, True, camera_model=cam)
    (batch * cuda(inp["g_batch"])).sum().backward()
    b = host(batch)
    got = dict(pack_o=b[:, 0:3], pack_d=b[:, 3:6], pack_nf=b[:, 6:8], pack_v=b[:, 8:11], g_rays_o=host(o.grad), g_rays_d=host(d.grad))
    CR.same_bits(got, direct, tuple(got))
    CR.bound_check("ndc", "wrapper-pack", dict(g_focal_xy=host(f.grad)), o64, o32, ("g_focal_xy",))


def test_ndc_rays_camera_is_the_same_launch():
    from scnerf_amd import render
    case = CR.ndc_case(n=257)
    rcase = CR.rays_case(mult=1)
    cm = camera_model(CR.rays_references(rcase)[0], 1, rcase["C"])
    init = cm.intrinsics_initial.detach().double().cpu().numpy()[:2]
    with torch.no_grad():
        Km = cm.get_intrinsic()
    inp = dict(CR.ndc_references(case)[0], f2=host(torch.stack([Km[0, 0], Km[1, 1]])))
    direct = CR.run_ndc(GpuRoute, inp, case)
    o, d = cuda(inp["o"]).requires_grad_(True), cuda(inp["d"]).requires_grad_(True)
    Hh, Ww = CR.NDC_HW
    no, nd = render.ndc_rays_camera(Hh, Ww, cm, CR.NDC_NEAR, o, d)
    ((no * cuda(inp["g_no"])).sum() + (nd * cuda(inp["g_nd"])).sum()).backward()
    got = dict(ndc_o=host(no), ndc_d=host(nd), g_rays_o=host(o.grad), g_rays_d=host(d.grad))
    CR.same_bits(got, direct, tuple(got))
    # d fx / d intrinsics_noise = scale * initial (multiplicative residual): the focal gradient, under the bound
    chain = CR.INTR_SCALE[1] * init
    o64, o32 = CR.ndc_oracle(inp, case, torch.float64), CR.ndc_oracle(inp, case, torch.float32)
    g = host(cm.intrinsics_noise.grad).astype(np.float64)
    assert not g[2:].any()
    CR.bound_check("ndc", "wrapper-ndc", dict(g_focal_xy=g[:2] / chain), o64, o32, ("g_focal_xy",))


def test_get_ray_o_noise_is_the_same_launch():
    shape = CR.SHAPES[0]
    inp, o64, o32 = CR.upsample_references(shape)
    direct = CR.run_upsample(GpuRoute, inp, shape)
    cm = camera_model(dict(grid_o=inp["grid"]), 0, 5, shape, scale_o=CR.UPSAMPLE_SCALE)
    out = cm.get_ray_o_noise()
    (out * cuda(inp["g_out"])).sum().backward()
    CR.same_bits(dict(out=host(out)), direct, ("out",))
    CR.bound_check("upsample", "wrapper", dict(d_grid=host(cm.ray_o_noise.grad)), o64, o32, ("d_grid",))


@pytest.mark.parametrize("used", ["K", "E"])
def test_camera_matrix_getters_with_one_of_the_two_used(used):
    """get_intrinsic() alone / get_extrinsic() alone: the launch with the other upstream gradient NULL, whose parameter
    gradient is exactly zero"""
    case = CR.matrices_case(null="g_E" if used == "K" else "g_K")
    inp, _, _ = CR.matrices_references(case)
    direct = CR.run_matrices(GpuRoute, inp, case)
    cm = camera_model(inp, case["mult"], case["C"])
    if used == "K":
        m = cm.get_intrinsic()
        (m * cuda(inp["g_K"])).sum().backward()
    else:
        m = cm.get_extrinsic()
        (m * cuda(inp["g_E"])).sum().backward()
    CR.same_bits({used: host(m)}, direct, (used,))
    for name, k in (("intrinsics_noise", "d_intr_noise"), ("extrinsics_noise", "d_extr_noise")):
        CR.same_bits({k: host(getattr(cm, name).grad)}, direct, (k,))
    assert cm.intrinsics_noise.grad.any() == (used == "K") and cm.extrinsics_noise.grad.any() == (used == "E")
