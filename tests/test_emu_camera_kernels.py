"""The camera kernels (csrc/camera_rays.hip: all 14 C entry points) launched stand-alone through the C ABI on the CPU SIMT
interpreter, against float64: the cases, references, bounds and guard rows of tests/camera_reference.py, which
tests/test_gpu_camera_kernels.py runs again on the GPU."""
import numpy as np
import pytest
import torch

from oracle import nerfpp_oracle as NO
from oracle import scnerf_oracle as O
from tests import camera_reference as CR
from tests.emu import harness as H

pytestmark = pytest.mark.emu


class EmuRoute:
    """how tests/camera_reference.py's run_* functions hold buffers and call the C ABI on the interpreter"""
    @staticmethod
    def inp(a):
        return None if a is None else np.ascontiguousarray(a)

    @staticmethod
    def out(shape, dtype=np.float32):
        buf = np.full((shape[0] + 2,) + tuple(shape[1:]), np.nan, dtype)
        return buf, buf[1:-1]

    @staticmethod
    def call(name, *args):
        H.call(name, *args, None)

    @staticmethod
    def host(buf):
        return buf


@pytest.fixture(autouse=True)
def _blocks_on_the_calling_thread(monkeypatch):
    """The interpreter runs the blocks of a launch on threads of its own and keeps every thread's fiber stacks mapped for
    the life of the process; on the calling thread (one worker) the stacks are reused from launch to launch, and this
    file's several hundred small launches leave a test worker's memory where it was."""
    monkeypatch.setenv("SIMT_EMU_THREADS", "1")


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    CR.report()


@pytest.mark.parametrize("case", CR.RAYS_CASES, ids=CR.case_id)
def test_camera_rays_vs_fp64(case):
    """scnerf_camera_rays_fwd / _bwd: any ray count, every pose source (per-ray index, single index, shared matrix, per-ray
    matrices, more cameras than the LDS pre-reduction holds), key points on the edges and outside, five grid / image shapes,
    absent and aliased grids, both residual modes, ill-conditioned Gram-Schmidt input, absent upstream gradients"""
    inp, _, _ = CR.rays_references(case)
    CR.check_rays(case, CR.run_rays(EmuRoute, inp, case))


@pytest.mark.parametrize("case", CR.NPP_CASES, ids=CR.case_id)
def test_npp_camera_rays_vs_fp64(case):
    """scnerf_npp_camera_rays_fwd / _bwd: pixel 0, the last pixel and the pixel at the principal point; with and without
    distortion (and its gradient), learnable pose and explicit matrix"""
    inp, _, _ = CR.npp_references(case)
    CR.check_npp(case, CR.run_npp(EmuRoute, inp, case))


@pytest.mark.parametrize("case", CR.MATRICES_CASES, ids=CR.case_id)
def test_camera_matrices_vs_fp64(case):
    inp, _, _ = CR.matrices_references(case)
    CR.check_matrices(case, CR.run_matrices(EmuRoute, inp, case))


@pytest.mark.parametrize("case", CR.NDC_CASES, ids=CR.case_id)
def test_ndc_vs_fp64(case):
    inp, _, _ = CR.ndc_references(case)
    CR.check_ndc(case, CR.run_ndc(EmuRoute, inp, case))


@pytest.mark.parametrize("case", CR.PACK_CASES, ids=CR.case_id)
def test_pack_rays_vs_fp64(case):
    inp, _, _ = CR.pack_references(case)
    CR.check_pack(case, CR.run_pack(EmuRoute, inp, case))


@pytest.mark.parametrize("shape", CR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_grid_vs_fp64(shape):
    inp, _, _ = CR.upsample_references(shape)
    CR.check_upsample(shape, CR.run_upsample(EmuRoute, inp, shape))


@pytest.mark.parametrize("case", CR.PINHOLE_CASES, ids=CR.case_id)
def test_pinhole_rays_vs_fp64(case):
    inp, _, _ = CR.pinhole_references(case)
    CR.check_pinhole(case, CR.run_pinhole(EmuRoute, inp, case))


def test_empty_batches_return_zero_with_zeroed_gradients():
    CR.run_and_check_empty(EmuRoute)


def test_per_ray_outputs_repeat_bit_for_bit():
    """two identical launches: what one thread writes per ray does not depend on the order of anything"""
    for case, refs, run in ((CR.rays_case(n=257), CR.rays_references, CR.run_rays),
                            (CR.rays_case(pose="perray"), CR.rays_references, CR.run_rays),
                            (CR.npp_case(n=257), CR.npp_references, CR.run_npp),
                            (CR.ndc_case(n=257), CR.ndc_references, CR.run_ndc),
                            (CR.pack_case(n=257), CR.pack_references, CR.run_pack)):
        inp = refs(case)[0]
        a, b = run(EmuRoute, inp, case), run(EmuRoute, inp, case)
        names = ("rays_o", "rays_d", "ndc_o", "ndc_d", "g_rays_o", "g_rays_d", "pack_o", "pack_d", "pack_v")
        CR.same_bits(a, b, names + (("d_extrinsic",) if case.get("pose") == "perray" else ()))


def test_the_extended_references_are_the_oracles():
    """ref_rays is oracle.scnerf_oracle.camera_rays where that applies (per-ray index, key points inside), bit for bit in
    both precisions; ref_npp_rays is oracle.nerfpp_oracle.camera_rays_pixel_centre in float32"""
    case = CR.DEFAULT_RAYS
    inp = CR.rays_inputs(case)
    gh, gw, Hh, Ww = case["shape"]
    for dtype in (torch.float32, torch.float64):
        cam, leaves = CR.oracle_cam(inp, 0, dtype, ("grid_o", "grid_d"))
        cam.update(ray_o_noise=leaves["grid_o"], ray_d_noise=leaves["grid_d"])
        kps, idx = torch.from_numpy(inp["kps"]).to(dtype), torch.from_numpy(inp["idx"])
        with torch.no_grad():
            for a, b in zip(CR.ref_rays(cam, Hh, Ww, kps, idx=idx), O.camera_rays(cam, Hh, Ww, kps, idx)):
                assert torch.equal(a, b)
    case = CR.npp_case()
    inp = CR.npp_inputs(case)
    cam, leaves = CR.oracle_cam(inp, 0, torch.float32, ("grid_o", "grid_d"))
    cam.update(ray_o_noise=leaves["grid_o"], ray_d_noise=leaves["grid_d"])
    sel, dist = torch.from_numpy(inp["select"]), torch.from_numpy(inp["dist"])
    with torch.no_grad():
        got = CR.ref_npp_rays(cam, Hh, Ww, sel, dist, idx=int(inp["single"]))
        want = NO.camera_rays_pixel_centre(O.camera_K(cam), O.camera_E(cam)[int(inp["single"])], sel, Hh, Ww, dist,
                                           O.upsample_noise_grid(cam["ray_o_noise"], Hh, Ww, CR.SCALE_O),
                                           O.upsample_noise_grid(cam["ray_d_noise"], Hh, Ww, CR.SCALE_D))
    for a, b in zip(got, want[:2]):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-5, atol=1e-6)


def test_camera_wrapper_accepts_an_empty_batch_of_per_ray_poses():
    """get_rays_kps_use_camera on [0, 2] key points and [0, 4, 4] poses: empty rays, and a backward that leaves a zero
    gradient in every camera tensor and a [0, 4, 4] gradient in the poses"""
    import types
    from scnerf_amd import get_rays, synthetic as synth
    from scnerf_amd.camera_dict import camera_dict
    from tests.emu.host_on_emu import emulated_device
    Hh, Ww = 48, 64
    spec = synth.camera_spec(Hh, Ww, n_cams=3, seed=4, multiplicative=True)
    args = types.SimpleNamespace(camera_model="pinhole_rot_noise_10k_rayo_rayd", grid_size=10,
                                 ray_o_noise_scale=spec["ray_o_noise_scale"], ray_d_noise_scale=spec["ray_d_noise_scale"],
                                 extrinsics_noise_scale=spec["extrinsics_noise_scale"],
                                 intrinsics_noise_scale=spec["intrinsics_noise_scale"], multiplicative_noise=True)
    with emulated_device():
        cm = camera_dict["pinhole_rot_noise_10k_rayo_rayd"](spec["K_init"], list(spec["poses"].numpy()), args, Hh, Ww)
        E = torch.zeros(0, 4, 4, requires_grad=True)
        ro, rd = get_rays.get_rays_kps_use_camera(Hh, Ww, cm, torch.zeros(0, 2), extrinsic=E)
        assert ro.shape == (0, 3) and rd.shape == (0, 3)
        (ro.sum() + rd.sum()).backward()
        assert E.grad is not None and E.grad.shape == (0, 4, 4)
        for p in (cm.intrinsics_noise, cm.ray_o_noise, cm.ray_d_noise):
            assert p.grad is not None and not p.grad.any()
        ro, rd = get_rays.get_rays_kps_use_camera(Hh, Ww, cm, torch.zeros(0, 2), idx_in_camera_param=torch.zeros(0).long())
        (ro.sum() + rd.sum()).backward()
        assert not cm.extrinsics_noise.grad.any()
