"""ops.inference_skip_empty on the MI355X: a forward-only render_rays call skips the fine pass of the rays whose coarse acc0
is at most tau.  300 and 1000 rays x (64 + 128) samples of synthetic.ray_batch through the standard networks, tau = the
median of the switch-off call's acc0 (tests/skip_empty_case.py: the coarse network's density bias is -0.25 there, because at
the default 0.5 that median is 1.0).  Live rays equal a switch-off call on the live rays alone and skipped rays equal the
coarse stage, bit for bit -- in the default arithmetic, under inference_arithmetic("fast"), under mlp_arithmetic("fp32")
and with the scale guard in "fallback" --; nothing skipped equals switch off; everything skipped launches no fine stage; a
training step does not notice the switch; render_path inherits it chunk by chunk.  Interpreter twin:
tests/test_emu_skip_empty.py."""
import numpy as np
import pytest
import torch

from scnerf_amd import synthetic as synth
from tests import skip_empty_case as C

pytestmark = pytest.mark.gpu
SC, SF = 64, 128


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = (O.inference_arithmetic(), O.mlp_arithmetic(), O.resident_guard(), O.fused_fine_stage(), O.inference_skip_empty())
    O.mlp_arithmetic("resident")
    O.inference_arithmetic("same")
    O.resident_guard("off")
    O.inference_skip_empty("off")
    yield O
    O.inference_arithmetic(before[0])
    O.mlp_arithmetic(before[1])
    O.resident_guard(before[2])
    O.fused_fine_stage(before[3])
    O.inference_skip_empty("off" if before[4] is None else before[4])


_shared = {}


def _nets():
    """(read only: one pair for the module)"""
    if "nets" not in _shared:
        _shared["nets"] = C.networks("cuda")
    return _shared["nets"]


@pytest.mark.parametrize("n", [300, 1000])
def test_live_rays_as_switch_off_on_them_skipped_rays_as_the_coarse_stage(ops, n):
    rays = synth.ray_batch(n, seed=1).cuda()
    tau, live = C.mixed_case(ops, rays, _nets(), SC, SF)
    C.all_twelve_outputs_case(ops, rays, _nets(), SC, SF, tau, live)


def test_injected_draws_follow_their_rays(ops):
    n = 300
    randoms = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=3).items()}
    C.mixed_case(ops, synth.ray_batch(n, seed=2).cuda(), _nets(), SC, SF, randoms=randoms)


@pytest.mark.parametrize("mode", ["fast", "fp32", "guard_fallback", "fused_fine_stage"])
def test_in_every_arithmetic_and_guard_mode(ops, mode):
    """each against the switch-off calls in the same mode; under SCNERF_FUSED_FINE_STAGE the switch-on fine stage is the
    three launches, whose numbers are the fused stage's"""
    if mode == "fast":
        ops.inference_arithmetic("fast")
    elif mode == "fp32":
        ops.mlp_arithmetic("fp32")
    elif mode == "guard_fallback":
        ops.resident_guard("fallback")
    else:
        ops.fused_fine_stage(True)
    C.mixed_case(ops, synth.ray_batch(300, seed=1).cuda(), _nets(), SC, SF, what=mode + ": ")


@pytest.mark.parametrize("n", [300, 1000])
def test_nothing_skipped_equals_switch_off(ops, n):
    C.nothing_skipped_case(ops, synth.ray_batch(n, seed=1).cuda(), "cuda", SC, SF)


def test_everything_skipped_returns_the_coarse_stage(ops):
    C.everything_skipped_case(ops, synth.ray_batch(300, seed=1).cuda(), "cuda", SC, SF)


def _training_step(nets, n=300):
    from scnerf_amd import render
    for net in nets:
        for q in net.parameters():
            q.grad = None
    rays = synth.ray_batch(n, seed=5).cuda().requires_grad_(True)
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=6).items()}
    ret = render.render_rays(rays, nets[0], C.query(), SC, retraw=True, perturb=1.0, N_importance=SF, network_fine=nets[1],
                             raw_noise_std=1.0, _randoms=rnd)
    loss = (ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["disp_map"].sum() + ret["acc0"].sum()
    loss.backward()
    grads = [q.grad.detach().clone() for net in nets for q in net.parameters()]
    return {k: v.detach().clone() for k, v in ret.items()}, rays.grad.clone(), grads


def test_a_training_step_does_not_notice_the_switch(ops):
    nets = C.networks("cuda")
    a = _training_step(nets)
    ops.skip_empty_stats(reset=True)
    ops.inference_skip_empty(float(a[0]["acc0"].median()))
    b = _training_step(nets)
    assert ops.skip_empty_stats() == {"rays": 0, "skipped": 0}          # the compaction never ran
    for k in a[0]:
        C.same_bits(a[0][k], b[0][k], k)
    C.same_bits(a[1], b[1], "d rays")
    assert len(a[2]) == len(b[2]) == 48 and all(float(g.abs().max()) > 0 for g in a[2])
    for i, (ga, gb) in enumerate(zip(a[2], b[2])):
        C.same_bits(ga, gb, "gradient of parameter %d" % i)


def test_render_path_inherits_the_switch(ops):
    """two 32 x 32 poses in chunks of 512 rays: four compactions, four counts.  Pixel by pixel the image is render_path's
    with the switch off where acc0 > tau and the (saturated) coarse render elsewhere."""
    from scnerf_amd import render as R
    H = W = 32
    nets = _nets()
    kw = dict(network_query_fn=C.query(), perturb=0.0, N_importance=SF, network_fine=nets[1], N_samples=SC, network_fn=nets[0],
              use_viewdirs=True, white_bkgd=False, raw_noise_std=0.0, near=0., far=1., ndc=True)
    poses = synth.camera_spec(H, W, n_cams=5, seed=4)["poses"][:2]
    K = torch.tensor([[40.0, 0, W / 2, 0], [0, 40.0, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    common = dict(gt_intrinsic=K.cuda(), gt_extrinsic=poses.cuda())
    rgb_off, disp_off = R.render_path(poses, (H, W, None), 512, kw, "test", **common)
    with torch.no_grad():
        coarse = [R.render(H=H, W=W, chunk=512, mode="test", image_idx=i, noisy_focal=None, **common, **kw)[3] for i in (0, 1)]
    acc0 = np.stack([c["acc0"].cpu().numpy().reshape(H, W) for c in coarse])
    rgb0 = np.stack([c["rgb0"].cpu().numpy().reshape(H, W, 3) for c in coarse])
    disp0 = np.stack([c["disp0"].cpu().numpy().reshape(H, W) for c in coarse])
    tau = float(np.float32(np.median(acc0)))
    assert 0.0 <= tau < 1.0
    live = ~(acc0 <= np.float32(tau))
    assert 0.25 * live.size <= live.sum() <= 0.75 * live.size, (live.sum(), tau)
    ops.skip_empty_stats(reset=True)
    ops.inference_skip_empty(tau)
    rgb_on, disp_on = R.render_path(poses, (H, W, None), 512, kw, "test", **common)
    ops.inference_skip_empty("off")
    assert ops.skip_empty_stats(reset=True) == {"rays": 2 * H * W, "skipped": int((~live).sum())}
    np.testing.assert_array_equal(rgb_on, np.where(live[..., None], rgb_off, rgb0))
    np.testing.assert_array_equal(disp_on, np.where(live, disp_off, disp0))


def test_the_switch_validates_its_argument(ops, monkeypatch):
    C.switch_validation(ops, monkeypatch)
