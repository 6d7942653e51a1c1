"""The scale guard of the resident arithmetic (ops.resident_guard, csrc/resident_guard.h) on the MI355X.  On a network whose
scale bound is too loose (tests/hostile_weights.py) every block trips at layer 3; the fallback guard runs the tripped
blocks again on the exact-fp32 kernels, so a render_rays step gives what mlp_arithmetic("fp32") gives.  On the suite's networks nothing trips and the guard changes no output."""
import pytest
import torch

from scnerf_amd import synthetic as synth
from tests import hostile_weights, trained_weights

pytestmark = pytest.mark.gpu

SC, SF = 64, 128
KEYS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "raw")


@pytest.fixture
def modes():
    from scnerf_amd import ops
    before = (ops.resident_guard(), ops.mlp_arithmetic())
    if before[1] != "resident":
        pytest.skip("the guard checks the resident arithmetic")
    yield ops
    ops.resident_guard(before[0])
    ops.mlp_arithmetic(before[1])


def _nets(params):
    from scnerf_amd import run_nerf_helpers as H
    out = []
    for p in params:
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(p)
        out.append(net.cuda())
    return out


def _query():
    from scnerf_amd import create_nerf, run_nerf_helpers as H
    return create_nerf.FusedNetworkQuery(H.get_embedder(10, 0)[0], H.get_embedder(4, 0)[0])


def _step(nets, n, seed=5):
    """one render_rays training step -> (outputs, [d rays, flat gradient of each network])"""
    from scnerf_amd import render
    rays = synth.ray_batch(n, seed=seed).cuda().requires_grad_(True)
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=seed + 1).items()}
    ret = render.render_rays(rays, nets[0], _query(), SC, retraw=True, perturb=1.0, N_importance=SF, network_fine=nets[1],
                             raw_noise_std=1.0, _randoms=rnd)
    loss = (ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["disp_map"].sum() + ret["acc0"].sum()
    params = [list(net.parameters()) for net in nets]
    got = torch.autograd.grad(loss, [rays] + params[0] + params[1])
    n0 = len(params[0])
    flat = [torch.cat([g.reshape(-1) for g in got[1:1 + n0]]), torch.cat([g.reshape(-1) for g in got[1 + n0:]])]
    return {k: ret[k].detach() for k in KEYS}, [got[0].detach()] + flat


def _render(nets, n, seed=9):
    """a render_path chunk: forward only"""
    from scnerf_amd import render
    rays = synth.ray_batch(n, seed=seed).cuda()
    with torch.no_grad():
        ret = render.render_rays(rays, nets[0], _query(), SC, retraw=True, perturb=0.0, N_importance=SF, network_fine=nets[1])
    return {k: ret[k] for k in KEYS}


def _same(a, b, grads=True):
    oa, ob = (a[0], b[0]) if grads else (a, b)
    for k in KEYS:
        assert torch.equal(oa[k], ob[k]), k
    if grads:
        for i, (x, y) in enumerate(zip(a[1], b[1])):
            assert torch.equal(x, y), i


def test_hostile_step_under_the_fallback_guard_is_the_fp32_step(modes):
    ops = modes
    nets = _nets([hostile_weights.weights(0), hostile_weights.weights(1)])
    ops.mlp_arithmetic("fp32")
    ref = _step(nets, 512)
    ops.mlp_arithmetic("resident")
    ops.resident_guard("off")
    off = _step(nets, 512)
    assert not torch.equal(off[0]["raw"], ref[0]["raw"])          # the loss the guard exists for
    ops.resident_guard("fallback")
    got = _step(nets, 512)
    for k in KEYS:
        assert torch.equal(got[0][k], ref[0][k]), k
    assert torch.equal(got[1][0], ref[1][0]), "d rays"
    for net, a, b in zip(("coarse", "fine"), got[1][1:], ref[1][1:]):
        rel = float((a - b).abs().max() / b.abs().max())
        print(net, "flat gradient, max difference / max |entry|:", rel)
        assert rel < 1e-3, (net, rel)
    m = ops.resident_margins()
    for name in ("coarse", "fine", "coarse_bwd", "fine_bwd"):
        assert m[name]["reran_blocks"] == m[name]["blocks"], (name, m[name])
    ops.resident_guard("report")
    again = _step(nets, 512)
    _same(got, again)
    m = ops.resident_margins()
    for name in ("coarse", "fine"):
        assert m[name]["layer_3"]["min_log2"] <= -6, (name, m[name]["layer_3"])
    ops.resident_guard("strict")
    with pytest.raises(ops.ResidentRangeError, match="layer_3"):
        _step(nets, 512)


@pytest.mark.parametrize("kind", ["xavier", "trained"])
def test_suite_networks_trip_nothing_at_the_headline_size(kind, modes):
    ops = modes
    if kind == "trained" and not trained_weights.have_trained():
        pytest.skip("no trained weights")
    params = ([synth.network_params(seed=0), synth.network_params(seed=1)] if kind == "xavier"
              else [trained_weights.weights("trained", which="coarse"), trained_weights.weights("trained", which="fine")])
    nets = _nets(params)
    ops.resident_guard("off")
    off, r_off = _step(nets, 4096), _render(nets, 4096)
    ops.resident_guard("report")
    on, r_on = _step(nets, 4096), _render(nets, 4096)
    _same(off, on)
    _same(r_off, r_on, grads=False)
    m = ops.resident_margins()
    for name in ("coarse", "fine", "coarse_bwd", "fine_bwd"):
        assert m[name]["reran_blocks"] == 0, (name, m[name])
        assert all(v["under"] == 0 and v["over"] == 0 for k, v in m[name].items() if isinstance(v, dict)), (name, m[name])
        print(kind, name, {k: v["min_log2"] for k, v in m[name].items() if isinstance(v, dict)})
    ops.resident_guard("fallback")
    _same(off, _step(nets, 4096))
    ops.resident_guard("strict")
    _step(nets, 4096)                                  # does not raise
    _render(nets, 4096)


def test_network_query_under_the_fallback_guard_is_the_fp32_query(modes):
    ops = modes
    net = _nets([hostile_weights.weights(0)])[0]
    g = torch.Generator().manual_seed(1)
    pts = (torch.rand(64, 64, 3, generator=g) * 2 - 1).cuda()
    vd = torch.nn.functional.normalize(torch.randn(64, 3, generator=g), dim=-1).cuda()
    ops.mlp_arithmetic("fp32")
    ref = _query()(pts, vd, net).detach()
    ops.mlp_arithmetic("resident")
    ops.resident_guard("fallback")
    got = _query()(pts, vd, net).detach()
    assert torch.equal(got, ref)
    m = ops.resident_margins()["query"]
    assert m["reran_blocks"] == m["blocks"], m
