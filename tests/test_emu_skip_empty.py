"""Interpreter twin of tests/test_gpu_skip_empty.py: ops.inference_skip_empty on the render path, the package's host layer
on CPU tensors against the CPU SIMT interpreter build of the kernels, 24 rays x (16 + 24) samples, the same case bodies
(tests/skip_empty_case.py) and the same equalities.  The switch's own checks need no kernel."""
import pytest

from scnerf_amd import synthetic as synth
from tests import skip_empty_case as C

N, SC, SF = 24, 16, 24


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = O.inference_skip_empty()
    O.inference_skip_empty("off")
    yield O
    O.inference_skip_empty("off" if before is None else before)


def test_the_switch_validates_its_argument(ops, monkeypatch):
    C.switch_validation(ops, monkeypatch)


@pytest.mark.emu
def test_live_rays_as_switch_off_on_them_skipped_rays_as_the_coarse_stage(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        nets = C.networks("cpu")
        rays = synth.ray_batch(N, seed=1)
        tau, live = C.mixed_case(ops, rays, nets, SC, SF)
        C.all_twelve_outputs_case(ops, rays, nets, SC, SF, tau, live)


@pytest.mark.emu
def test_injected_draws_follow_their_rays(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        C.mixed_case(ops, synth.ray_batch(N, seed=2), C.networks("cpu"), SC, SF, randoms=synth.render_randoms(N, SC, SF, seed=3))


@pytest.mark.emu
def test_nothing_skipped_and_everything_skipped(ops):
    from tests.emu.host_on_emu import emulated_device
    with emulated_device("fp32"):
        rays = synth.ray_batch(N, seed=1)
        C.nothing_skipped_case(ops, rays, "cpu", SC, SF)
        C.everything_skipped_case(ops, rays, "cpu", SC, SF)


@pytest.mark.emu
def test_a_call_that_tracks_gradients_does_not_notice(ops):
    from scnerf_amd import render as R
    from tests.emu.host_on_emu import emulated_device

    def forward(nets, rays):
        ret = R.render_rays(rays, nets[0], C.query(), SC, retraw=True, perturb=0.0, N_importance=SF, network_fine=nets[1])
        return {k: v.detach().clone() for k, v in ret.items()}

    with emulated_device("fp32"):
        nets = C.networks("cpu")
        rays = synth.ray_batch(4, seed=1).requires_grad_(True)
        a = forward(nets, rays)
        ops.skip_empty_stats(reset=True)
        ops.inference_skip_empty(float(a["acc0"].median()))
        b = forward(nets, rays)
        assert ops.skip_empty_stats() == {"rays": 0, "skipped": 0}          # the compaction never ran
        for k in a:
            C.same_bits(a[k], b[k], k)
