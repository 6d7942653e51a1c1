"""ops.inference_arithmetic("fast") on the MI355X: forward-only network passes on one fp16 product per product
(scnerf_mlp_fwd_h3_fast, scnerf_coarse_stage_fwd_h3_fast; csrc/mlp_fwd_h3_kernel.h, PRODUCTS == 1).  The accuracy statement
lives at the network and coarse-stage level, against the fp64 yardstick of tests/fast_arithmetic_model.py; everything around
the network (samplers, compositing) is the same device code on the same numbers, so the host-level checks are bit for bit.
A call that tracks gradients, and every call under mlp_arithmetic("fp32"), must not notice the switch."""
import types

import numpy as np
import pytest
import torch

from scnerf_amd import synthetic as synth
from tests import fast_arithmetic_model as FM
from tests import trained_weights as TW
from tests.emu_mlp_util import npp_to_nerf_names

pytestmark = pytest.mark.gpu

SC, SF = 64, 128


@pytest.fixture
def ops():
    from scnerf_amd import ops as O
    before = (O.inference_arithmetic(), O.mlp_arithmetic(), O.resident_guard(), O.fused_fine_stage())
    O.mlp_arithmetic("resident")
    O.inference_arithmetic("same")
    O.resident_guard("off")
    yield O
    O.inference_arithmetic(before[0])
    O.mlp_arithmetic(before[1])
    O.resident_guard(before[2])
    O.fused_fine_stage(before[3])


def _params(pd, kind):
    if kind.startswith("trained"):
        return TW.weights("trained", which=kind.split("/")[1])
    if pd == 3:
        return synth.network_params(seed=0)
    return {k: v.clone() for k, v in npp_to_nerf_names(synth.nerfpp_params(777), "bg_net.").items()}


_cases = {}


def _case(ops, pd, kind, n_rays, spr):
    """one (network, inputs) case: packed weights on the device, inputs, the fp64 yardstick and the default arithmetic's
    output -- computed once, shared by the view-direction layouts, never written to"""
    key = (pd, kind, n_rays, spr)
    if key not in _cases:
        from scnerf_amd import mlp_layout as ML
        p = _params(pd, kind)
        flat = torch.cat([p[name].reshape(-1) for name, _ in ML.layout(pd).param_shapes]).float().cuda()
        wf, rw = ops.pack_weights(flat, "fwd", pd=pd), ops.pack_resident(flat, pd)
        g = torch.Generator().manual_seed(3)
        pts = torch.rand(n_rays * spr, pd, generator=g) * 3 - 1.5
        vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
        raw_res = ops.mlp_fwd(pts.cuda(), vd.cuda(), spr, wf, pd=pd, planes=rw).cpu().numpy()
        _cases[key] = (wf, rw, pts, vd, FM.Yardstick(p, pts.numpy(), vd.numpy(), spr), raw_res)
    return _cases[key]


@pytest.mark.parametrize("vd_stride", [3, 11])
@pytest.mark.parametrize("n_rays,spr", [(3, 70), (33, 64)])
@pytest.mark.parametrize("pd,kind", [(3, "xavier"), (3, "trained/coarse"), (3, "trained/fine"), (4, "xavier")])
def test_one_product_forward_through_the_c_abi(ops, pd, kind, n_rays, spr, vd_stride):
    """3 x 70: a partial wave tile in a second block, samples per ray that divide nothing; 33 x 64: seventeen blocks, the
    last one half empty.  The output buffer is poisoned: every row below n_samples finite, every padding row untouched."""
    from scnerf_amd import _capi
    wf, rw, pts, vd, yard, raw_res = _case(ops, pd, kind, n_rays, spr)
    P = n_rays * spr
    rows = (P + 127) // 128 * 128 + 128
    raw = torch.full((rows, 4), float("nan"), device="cuda")
    if vd_stride == 3:
        v = vd.cuda()
    else:
        batch = torch.full((n_rays, 11), float("nan"))
        batch[:, 8:11] = vd
        v = batch.cuda()[:, 8:11]
    pts_d = pts.cuda()
    st = _capi.load().scnerf_mlp_fwd_h3_fast(pd, pts_d.data_ptr(), v.data_ptr(), vd_stride, spr, wf.data_ptr(), rw.fwd.data_ptr(),
                                             rw.scales.data_ptr(), raw.data_ptr(), P, None, 0, 0, _capi.current_stream())
    assert st == 0
    got = raw.cpu().numpy()
    assert np.isfinite(got[:P]).all() and np.isnan(got[P:]).all()
    FM.check(yard, got[:P], raw_res, "pd %d %s %d x %d stride %d:" % (pd, kind, n_rays, spr, vd_stride))


def _nets(params):
    from scnerf_amd import run_nerf_helpers as H
    out = []
    for p in params:
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(p)
        out.append(net.cuda())
    return out


def _trained_nets():
    return _nets([TW.weights("trained", which="coarse"), TW.weights("trained", which="fine")])


def _query():
    from scnerf_amd import create_nerf, run_nerf_helpers as H
    return create_nerf.FusedNetworkQuery(H.get_embedder(10, 0)[0], H.get_embedder(4, 0)[0])


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert not torch.isnan(a).any(), what
    assert torch.equal(a, b), what


@pytest.mark.parametrize("n", [3, 33])
def test_one_product_coarse_stage_equals_its_three_launches(ops, n):
    from scnerf_amd.functional import host_linspace
    net = _nets([synth.network_params(seed=0)])[0]
    ops.inference_arithmetic("fast")
    wf, pl = ops.inference_packs(net, net.flat_parameters())
    assert pl.fast
    rays = synth.ray_batch(n, seed=5).cuda()
    rnd = synth.render_randoms(n, SC, 8, seed=7)
    t_rand, noise = rnd["t_rand"].cuda(), rnd["noise_c"].cuda()
    t_vals = host_linspace(SC, "cuda")
    z0, pts0 = ops.coarse_sample(rays, t_vals, t_rand, False)
    raw0 = ops.mlp_fwd(pts0, rays[:, 8:11], SC, wf, planes=pl).view(n, SC, 4)
    rgb0, disp0, acc0, w0, depth0 = ops.composite_fwd(raw0, z0, rays, noise, True)
    z1, pts1, raw1, rgb1, disp1, acc1, w1, depth1 = ops.coarse_stage_fwd(rays, t_vals, t_rand, False, wf, None, noise, True, planes=pl)
    for name, a, b in (("z", z0, z1), ("pts", pts0, pts1), ("raw", raw0, raw1), ("rgb", rgb0, rgb1), ("disp", disp0, disp1),
                       ("acc", acc0, acc1), ("weights", w0, w1), ("depth", depth0, depth1)):
        _same_bits(a, b, name)
    # against the yardstick: the stage's raw is the one-product network on the stage's own points
    ops.inference_arithmetic("same")
    _, pl_same = ops.inference_packs(net, net.flat_parameters())
    raw_res = ops.coarse_stage_fwd(rays, t_vals, t_rand, False, wf, None, noise, True, planes=pl_same)[2]
    yard = FM.Yardstick(synth.network_params(seed=0), pts1.view(-1, 3).cpu().numpy(), rays[:, 8:11].cpu().numpy(), SC)
    FM.check(yard, raw1.view(-1, 4).cpu().numpy(), raw_res.view(-1, 4).cpu().numpy(), "coarse stage %d rays:" % n)


def test_render_rays_without_gradients_is_the_four_fast_launches(ops):
    """render_rays under no_grad with "fast", 33 rays x (64 + 128), perturb = 0: coarse_stage_fwd, fine_sample, mlp_fwd,
    composite_fwd on the one-product packs, one after the other -- every returned tensor bit for bit, z_vals included (no
    tolerance anywhere in the sampler: the same coarse weights give the same search indices)."""
    from scnerf_amd.functional import RenderConfig, RenderRaysFunction, host_linspace
    net_c, net_f = _trained_nets()
    n = 33
    rays = synth.ray_batch(n, seed=9).cuda()
    ops.inference_arithmetic("fast")
    for fused in (False, True):                      # (the fused fine stage has no fast instantiation: the three launches)
        ops.fused_fine_stage(fused)
        with torch.no_grad():
            cfg = RenderConfig(SC, SF, False, False, torch.is_grad_enabled())
            got = RenderRaysFunction.apply(rays, cfg, None, None, None, None, net_c, net_f,
                                           *net_c.ordered_parameters(), *net_f.ordered_parameters())
        wf_c, pl_c = ops.inference_packs(net_c, net_c.flat_parameters())
        wf_f, pl_f = ops.inference_packs(net_f, net_f.flat_parameters())
        assert pl_c.fast and pl_f.fast
        z_c, _, raw_c, rgb_c, disp_c, acc_c, w_c, depth_c = ops.coarse_stage_fwd(rays, host_linspace(SC, "cuda"), None, False, wf_c,
                                                                                 None, None, False, planes=pl_c)
        z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, host_linspace(SF, "cuda"))
        raw_f = ops.mlp_fwd(pts_f, rays[:, 8:11], SC + SF, wf_f, planes=pl_f).view(n, SC + SF, 4)
        rgb_f, disp_f, acc_f, _, depth_f = ops.composite_fwd(raw_f, z_f, rays, None, False, want_weights=False)
        want = (rgb_f, disp_f, acc_f, depth_f, raw_f, rgb_c, disp_c, acc_c, depth_c, z_std, z_f, z_s)
        names = ("rgb_map", "disp_map", "acc_map", "depth_map", "raw", "rgb0", "disp0", "acc0", "depth0", "z_std", "z_vals", "z_samples")
        assert len(got) == len(want)
        for name, a, b in zip(names, got, want):
            _same_bits(a, b, "%s (fused fine stage %s)" % (name, fused))
    # and it is not the default arithmetic's render
    ops.inference_arithmetic("same")
    with torch.no_grad():
        ref = RenderRaysFunction.apply(rays, cfg, None, None, None, None, net_c, net_f,
                                       *net_c.ordered_parameters(), *net_f.ordered_parameters())
    assert not torch.equal(ref[4], got[4])


def test_nerfpp_node_without_gradients_is_its_fast_launches(ops):
    from scnerf_amd import _capi
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    from scnerf_amd.nerfplusplus.ddp_model import _OUT_KEYS
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet
    args = types.SimpleNamespace(max_freq_log2=10, max_freq_log2_viewdirs=4, netdepth=8, netwidth=256, use_viewdirs=True)
    net = NerfNet(args)
    net.load_state_dict(synth.nerfpp_params(778))
    net = net.cuda()
    n, sf, sb = 33, 64, 32
    g = torch.Generator().manual_seed(11)
    o = (torch.rand(n, 3, generator=g) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda()
    far = TR.intersect_sphere(o, d)
    fg_z = 1e-4 + torch.sort(torch.rand(n, sf, generator=g), -1)[0].cuda() * (far[:, None] - 1e-4)
    bg_z = torch.sort(torch.rand(n, sb, generator=g), -1, descending=True)[0].cuda().contiguous()
    ops.inference_arithmetic("fast")
    with torch.no_grad():
        got = net(o, d, far, fg_z, bg_z)
    lib = _capi.load()
    st = _capi.current_stream()
    fg_pts = torch.empty((n * sf, 3), device="cuda")
    bg_pts = torch.empty((n * sb, 4), device="cuda")
    views = torch.empty((n, 3), device="cuda")
    zf, zb, zmax = fg_z.contiguous(), bg_z.contiguous(), far.contiguous()
    assert lib.scnerf_npp_points_fwd(o.data_ptr(), d.data_ptr(), zf.data_ptr(), zb.data_ptr(), fg_pts.data_ptr(), bg_pts.data_ptr(),
                                     views.data_ptr(), None, n, sf, sb, st) == 0
    wf_f, pl_f = ops.inference_packs(net.fg_net, net.fg_net.flat_parameters(), 3, remap=net.fg_net.pack_remap())
    wf_b, pl_b = ops.inference_packs(net.bg_net, net.bg_net.flat_parameters(), 4, remap=net.bg_net.pack_remap())
    assert pl_f.fast and pl_b.fast
    raw_f = ops.mlp_fwd(fg_pts, views, sf, wf_f, pd=3, planes=pl_f)
    raw_b = ops.mlp_fwd(bg_pts, views, sb, wf_b, pd=4, planes=pl_b)
    shapes = {"rgb": (n, 3), "fg_weights": (n, sf), "bg_weights": (n, sb), "fg_rgb": (n, 3), "fg_depth": (n,), "bg_rgb": (n, 3),
              "bg_depth": (n,), "bg_lambda": (n,)}
    t = {k: torch.full(sh, float("nan"), device="cuda") for k, sh in shapes.items()}
    assert lib.scnerf_npp_composite_fwd(raw_f.data_ptr(), raw_b.data_ptr(), zf.data_ptr(), zmax.data_ptr(), zb.data_ptr(), d.data_ptr(),
                                        *[t[k].data_ptr() for k in _OUT_KEYS], n, sf, sb, st) == 0
    for k in _OUT_KEYS:
        _same_bits(got[k], t[k], k)
    ops.inference_arithmetic("same")
    with torch.no_grad():
        ref = net(o, d, far, fg_z, bg_z)
    assert not torch.equal(ref["rgb"], got["rgb"])


def _training_step(nets, n=33, seed=5):
    from scnerf_amd import render
    for net in nets:                                  # .grad tensors as views of one flat buffer (what FusedAdam attaches)
        net.flat_parameters()
        params = [q for _, q in net.named_parameters()]
        buf = torch.zeros(sum(q.numel() for q in params), device="cuda")
        o = 0
        for q in params:
            q.grad = buf[o:o + q.numel()].view(q.shape)
            o += q.numel()
        assert net.attached_flat_grad() is not None
    rays = synth.ray_batch(n, seed=seed).cuda().requires_grad_(True)
    rnd = {k: v.cuda() for k, v in synth.render_randoms(n, SC, SF, seed=seed + 1).items()}
    ret = render.render_rays(rays, nets[0], _query(), SC, retraw=True, perturb=1.0, N_importance=SF, network_fine=nets[1],
                             raw_noise_std=1.0, _randoms=rnd)
    loss = (ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["disp_map"].sum() + ret["acc0"].sum()
    loss.backward()
    return ({k: v.detach().clone() for k, v in ret.items()}, rays.grad.clone(), [net.attached_flat_grad().clone() for net in nets])


def test_a_training_step_does_not_notice_the_switch(ops):
    nets = _trained_nets()
    ops.inference_arithmetic("same")
    a = _training_step(nets)
    ops.inference_arithmetic("fast")
    b = _training_step(nets)
    for k in a[0]:
        _same_bits(a[0][k], b[0][k], k)
    _same_bits(a[1], b[1], "d rays")
    for i in (0, 1):
        assert float(a[2][i].abs().max()) > 0
        _same_bits(a[2][i], b[2][i], "flat gradient %d" % i)


def _render(nets, n=33, seed=9):
    from scnerf_amd import render
    rays = synth.ray_batch(n, seed=seed).cuda()
    with torch.no_grad():
        return render.render_rays(rays, nets[0], _query(), SC, retraw=True, perturb=0.0, N_importance=SF, network_fine=nets[1])


def test_fp32_arithmetic_ignores_the_switch(ops):
    nets = _trained_nets()
    ops.mlp_arithmetic("fp32")
    a = _render(nets)
    ops.inference_arithmetic("fast")
    b = _render(nets)
    for k in a:
        _same_bits(a[k], b[k], k)


def test_pack_cache_keys_on_the_inference_arithmetic(ops):
    nets = _trained_nets()
    st = ops.PACK_CACHE_STATS
    st["hits"] = st["packs"] = 0
    a = _render(nets)
    assert (st["packs"], st["hits"]) == (2, 0)
    ops.inference_arithmetic("fast")
    b = _render(nets)
    assert (st["packs"], st["hits"]) == (4, 0)          # packed again for the other arithmetic: no stale hit
    b2 = _render(nets)
    assert (st["packs"], st["hits"]) == (4, 2)
    ops.inference_arithmetic("same")
    c = _render(nets)
    assert (st["packs"], st["hits"]) == (6, 2)
    assert not torch.equal(a["raw"], b["raw"])
    for k in a:
        _same_bits(a[k], c[k], k)
        _same_bits(b[k], b2[k], k)


def test_fast_passes_take_no_guard_record(ops):
    nets = _trained_nets()
    ops.resident_guard("report")
    _render(nets)
    m = ops.resident_margins()
    assert "coarse" in m and "fine" in m
    ops.inference_arithmetic("fast")
    b = _render(nets)
    m = ops.resident_margins()
    assert "coarse" not in m and "fine" not in m, sorted(m)
    ops.resident_guard("off")
    c = _render(nets)
    for k in b:
        _same_bits(b[k], c[k], k)


def test_the_switch_validates_its_argument(ops):
    with pytest.raises(ValueError):
        ops.inference_arithmetic("half")
    assert ops.inference_arithmetic() == "same"
    assert ops.inference_arithmetic("fast") == "fast"
