"""The lean workspace in the NeRF++ node (both networks: 3-D foreground, 4-D background points) and in the differentiable
network query node, switched by ops.lean_workspace_scope("all") -- against the same nodes under scope "render", which run
the full workspace as before.

Between the two scopes everything but the three derived tensors of each network (feature_linear.weight, feature_linear.bias,
views_linears.0.weight[:, :256]; in the NeRF++ module: base_remap_layers.0.weight / .bias, rgb_layers.0.weight[:, :256]) is
bit-identical; the derived tensors are judged against direct fp64 sums over the "render"-scope run's own workspaces with the
exact-fp32-MFMA group on those workspaces as the yardstick, K = 4 (test_gpu_lean_workspace.py).  The foreground network's
module order differs from the kernels' canonical one: a parameter snapshot in module order would put other weights where
the finishing kernel reads W_f, b_f and W_vf, and fail the judgment by orders of magnitude.

Ratios measured on the MI355X over this file's cases (NeRF++ foreground, background, query node): feature_linear.weight
0.38, 0.46, 0.76; feature_linear.bias 1.28, 1.07, 1.82; views_linears.0.weight[:, :256] 0.35, 0.50, 0.60.  Largest: 1.82."""
import types

import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from scnerf_amd import synthetic as synth

pytestmark = pytest.mark.gpu

K = 4.0                        # the project's acceptance factor (test_gpu_lean_workspace.py), unchanged
DERIVED = ("feature_linear.weight", "feature_linear.bias", "views_linears.0.weight[:, :256]")
ARGS = types.SimpleNamespace(max_freq_log2=10, max_freq_log2_viewdirs=4, netdepth=8, netwidth=256, use_viewdirs=True)
N_RAYS, S_FG, S_BG = 50, 34, 34                # 1700 samples per network: a partial 128-block, six chunks


@pytest.fixture
def ops():
    """the switches these tests move, restored after every test"""
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from scnerf_amd import ops as _ops
    _ops.check_layout()
    before = (_ops.lean_workspace_scope(), _ops.wgrad_arithmetic(), _ops.mlp_arithmetic(), _ops.resident_guard())
    _ops.mlp_arithmetic("resident")
    _ops.wgrad_arithmetic("half")
    _ops.resident_guard("off")
    yield _ops
    _ops.lean_workspace_scope(before[0])
    _ops.wgrad_arithmetic(before[1])
    _ops.mlp_arithmetic(before[2])
    _ops.resident_guard(before[3])


def _words(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _derived(flat, pd):
    off = ML.layout(pd).param_offsets
    flat = np.asarray(flat)
    wv = flat[off["views_linears.0.weight"]:off["views_linears.0.weight"] + 128 * 283].reshape(128, 283)
    return {DERIVED[0]: flat[off["feature_linear.weight"]:off["feature_linear.weight"] + 256 * 256].reshape(256, 256),
            DERIVED[1]: flat[off["feature_linear.bias"]:off["feature_linear.bias"] + 256],
            DERIVED[2]: wv[:, :256]}


def _derived_mask(pd):
    lay = ML.layout(pd)
    off = lay.param_offsets
    m = np.zeros(lay.n_params, bool)
    m[off["feature_linear.weight"]:off["feature_linear.weight"] + 256 * 256] = True
    m[off["feature_linear.bias"]:off["feature_linear.bias"] + 256] = True
    m[off["views_linears.0.weight"]:off["views_linears.0.weight"] + 128 * 283].reshape(128, 283)[:, :256] = True
    return m


def _fp64_reference(save, grads, P, pd):
    """the three derived gradients as direct fp64 sums over the samples, from a FULL pass's saved sections"""
    Pp = ML.padded_samples(P)
    so, _ = ML.section_offsets(ML.layout(pd).save_sections, P)
    go, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)

    def rows(buf, o, w):
        return ML.untile(buf[o:o + w * Pp].cpu().numpy(), w, P).astype(np.float64)
    act7, feat = rows(save, so["act7"], 256), rows(save, so["feat"], 256)
    dzv, dfeat = rows(grads, go["dzv"], 128), rows(grads, go["dfeat"], 256)
    return {DERIVED[0]: dfeat.T @ act7, DERIVED[1]: dfeat.sum(0), DERIVED[2]: dzv.T @ feat}


def _judge(what, lean, yard, ref):
    """lean, yard, ref: {derived tensor: array}"""
    def err(got):
        return {k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in DERIVED}
    e_lean, e_yard = err(lean), err(yard)
    for k in DERIVED:
        print("[lean nodes] %s %s: lean %.3e fp32-MFMA %.3e ratio %.2f" % (what, k, e_lean[k], e_yard[k], e_lean[k] / e_yard[k]))
    for k in DERIVED:
        assert e_lean[k] <= K * e_yard[k], (what, k, e_lean[k], e_yard[k])


def _spy(ops, monkeypatch):
    captured = []
    real = ops.nerf_wgrad

    def spy(save, grads, d_raw, P, **kw):
        captured.append({"save": save, "grads": grads, "d_raw": d_raw, "P": P, "pd": kw.get("pd", 3), "maxima": kw.get("maxima"),
                         "lean": bool(kw.get("lean")), "flat_params": kw.get("flat_params")})
        return real(save, grads, d_raw, P, **kw)
    monkeypatch.setattr(ops, "nerf_wgrad", spy)
    return captured, real


def _yardstick(ops, real, call):
    """the exact-fp32-MFMA group on a captured full workspace -> its derived tensors"""
    ops.wgrad_arithmetic("fp32")
    flat = real(call["save"], call["grads"], call["d_raw"], call["P"], pd=call["pd"], maxima=call["maxima"]).cpu().numpy()
    ops.wgrad_arithmetic("half")
    return _derived(flat, call["pd"])


# ---- the NeRF++ node ------------------------------------------------------------------------------------------------------
NPP_DERIVED = {"base_remap_layers.0.weight": DERIVED[0], "base_remap_layers.0.bias": DERIVED[1], "rgb_layers.0.weight": DERIVED[2]}


def _npp_net(seed=778):
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet
    net = NerfNet(ARGS)
    net.load_state_dict(synth.nerfpp_params(seed))
    return net.cuda()


@pytest.fixture(scope="module")
def npp_inputs():
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    g = torch.Generator().manual_seed(5)
    n = N_RAYS
    o = (torch.randn(n, 3, generator=g) * 0.25).cuda()
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda() * 1.3
    frac = torch.sort(torch.rand(n, S_FG, generator=g), -1)[0].cuda()
    bg_z = torch.sort(torch.rand(n, S_BG, generator=g), -1)[0].cuda()
    far = TR.intersect_sphere(o, d).detach()
    fg_z = (1e-4 + frac * (far - 1e-4)[:, None]).detach()
    target = torch.rand(n, 3, generator=g).cuda()
    return {"o": o, "d": d, "far": far, "fg_z": fg_z, "bg_z": bg_z, "target": target}


def _npp_step(net, inp, between=None):
    """forward + backward with every input requiring grad -> (the eight outputs, the four input gradients, {network:
    {parameter name: gradient}})"""
    leaves = [inp[k].clone().requires_grad_(True) for k in ("o", "d", "far", "fg_z", "bg_z")]
    ret = net(*leaves)
    loss = ((ret["rgb"] - inp["target"]) ** 2).mean() + 0.1 * ret["fg_depth"].mean() + 0.1 * ret["bg_depth"].mean() \
        + 0.05 * ret["bg_lambda"].mean() + 0.01 * (ret["fg_weights"] ** 2).sum() + 0.01 * (ret["bg_weights"] ** 2).sum() \
        + 0.1 * (ret["fg_rgb"] * ret["bg_rgb"]).mean()
    if between is not None:
        between()
    named = {"fg": list(net.fg_net.named_parameters()), "bg": list(net.bg_net.named_parameters())}
    params = [p for _, p in named["fg"]] + [p for _, p in named["bg"]]
    got = torch.autograd.grad(loss, leaves[:4] + params)
    n_fg = len(named["fg"])
    pg = {"fg": {name: g.detach().clone() for (name, _), g in zip(named["fg"], got[4:4 + n_fg])},
          "bg": {name: g.detach().clone() for (name, _), g in zip(named["bg"], got[4 + n_fg:])}}
    return [ret[k].detach().clone() for k in ret], [x.detach().clone() for x in got[:4]], pg


def _assert_same_bits(a, b, what):
    outs_a, in_a, pg_a = a
    outs_b, in_b, pg_b = b
    assert len(outs_a) == 8
    for i, (x, y) in enumerate(zip(outs_a, outs_b)):
        assert torch.equal(_words(x), _words(y)), "%s: output %d" % (what, i)
    for name, x, y in zip(("ray_o", "ray_d", "fg_z_max", "fg_z_vals"), in_a, in_b):
        assert torch.equal(_words(x), _words(y)), "%s: d %s" % (what, name)
    for netname in ("fg", "bg"):
        for name in pg_a[netname]:
            assert torch.equal(_words(pg_a[netname][name]), _words(pg_b[netname][name])), "%s: %s.%s" % (what, netname, name)


def test_nerfpp_node_scope_all_against_scope_render(ops, monkeypatch, npp_inputs):
    net = _npp_net()
    from scnerf_amd.nerfplusplus.nerf_network import canonical_to_module_name
    assert [n for n, _ in net.fg_net.named_parameters()] != [canonical_to_module_name(n) for n, _ in ML.layout(3).param_shapes], \
        "the module order is expected to differ from the canonical one"
    captured, real = _spy(ops, monkeypatch)
    ops.lean_workspace_scope("render")
    assert ops.lean_workspace() is True
    full = _npp_step(net, npp_inputs)
    assert [(c["pd"], c["lean"]) for c in captured] == [(3, False), (4, False)]        # nothing changes by default
    full_calls = list(captured)
    ops.lean_workspace_scope("all")
    assert ops.lean_workspace() is True
    lean = _npp_step(net, npp_inputs)
    assert [(c["pd"], c["lean"]) for c in captured[2:]] == [(3, True), (4, True)]
    assert all(c["flat_params"] is not None and c["flat_params"].numel() == ML.layout(c["pd"]).n_params for c in captured[2:])
    monkeypatch.setattr(ops, "nerf_wgrad", real)
    for i, (x, y) in enumerate(zip(full[0], lean[0])):
        assert torch.equal(_words(x), _words(y)), "output %d" % i
    for name, x, y in zip(("ray_o", "ray_d", "fg_z_max", "fg_z_vals"), full[1], lean[1]):
        assert torch.equal(_words(x), _words(y)), "d " + name
    for netname, call in zip(("fg", "bg"), full_calls):
        a, b = full[2][netname], lean[2][netname]
        got = {}
        for name in a:
            if name not in NPP_DERIVED:
                assert torch.equal(_words(a[name]), _words(b[name])), (netname, name)
            elif name == "rgb_layers.0.weight":
                assert torch.equal(_words(a[name][:, 256:]), _words(b[name][:, 256:])), (netname, name, "direction columns")
                got[NPP_DERIVED[name]] = b[name][:, :256].cpu().numpy()
            else:
                got[NPP_DERIVED[name]] = b[name].cpu().numpy()
            assert bool(torch.isfinite(b[name]).all()), (netname, name)
        assert sorted(got) == sorted(DERIVED)
        _judge("nerfpp/%s P=%d" % (netname, call["P"]), got, _yardstick(ops, real, call),
               _fp64_reference(call["save"], call["grads"], call["P"], call["pd"]))


def test_nerfpp_node_follows_its_forward_decision(ops, monkeypatch, npp_inputs):
    """the scope moves between forward and backward: the backward runs what the forward decided"""
    net = _npp_net()
    captured, _ = _spy(ops, monkeypatch)
    ops.lean_workspace_scope("all")
    _npp_step(net, npp_inputs, between=lambda: ops.lean_workspace_scope("off"))
    assert [(c["pd"], c["lean"]) for c in captured] == [(3, True), (4, True)]
    del captured[:]
    _npp_step(net, npp_inputs, between=lambda: ops.lean_workspace_scope("all"))
    assert [(c["pd"], c["lean"]) for c in captured] == [(3, False), (4, False)]


def test_nerfpp_node_backward_reads_a_parameter_snapshot(ops, npp_inputs):
    """an in-place update of both networks' base_remap_layers.0.weight between forward and backward must not reach the
    backward: the finishing kernel reads that tensor"""
    net = _npp_net()
    ops.lean_workspace_scope("all")
    calm = _npp_step(net, npp_inputs)
    tensors = [net.fg_net.base_remap_layers[0].weight, net.bg_net.base_remap_layers[0].weight]
    kept = [t.detach().clone() for t in tensors]

    def disturb():
        with torch.no_grad():
            for t in tensors:
                t.add_(0.25)
    disturbed = _npp_step(net, npp_inputs, between=disturb)
    assert all(not torch.equal(t.detach(), k) for t, k in zip(tensors, kept))
    with torch.no_grad():
        for t, k in zip(tensors, kept):
            t.copy_(k)
    _assert_same_bits(calm, disturbed, "in-place update between forward and backward")


def test_nerfpp_node_under_the_scale_guard(ops, npp_inputs):
    """resident_guard("fallback") with scope "all": bit-identical to the guard off (no block of these inputs trips; DESIGN
    section 2 states the property for the render step)"""
    net = _npp_net()
    ops.lean_workspace_scope("all")
    plain = _npp_step(net, npp_inputs)
    ops.resident_guard("fallback")
    guarded = _npp_step(net, npp_inputs)
    ops.resident_guard("off")
    _assert_same_bits(plain, guarded, "guard fallback against guard off")


# ---- the network query node -----------------------------------------------------------------------------------------------
def _query_step(ops, net, embed, embeddirs, pts0, vd0, w):
    from scnerf_amd import create_nerf
    pts, vd = pts0.clone().requires_grad_(True), vd0.clone().requires_grad_(True)
    raw = create_nerf.run_network(pts, vd, net, embed, embeddirs)
    params = list(net.ordered_parameters())
    got = torch.autograd.grad((raw * w).sum(), [pts, vd] + params)
    return raw.detach().clone(), got[0].detach().clone(), got[1].detach().clone(), torch.cat([g.reshape(-1) for g in got[2:]])


def test_query_node_scope_all_against_scope_render(ops, monkeypatch):
    from scnerf_amd import run_nerf_helpers as H
    net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
    net.load_state_dict(synth.network_params(seed=2))
    net = net.cuda()
    embed, embeddirs = H.get_embedder(10, 0)[0], H.get_embedder(4, 0)[0]
    g = torch.Generator().manual_seed(31)
    n, s = 6, 50                                   # 300 samples: a partial 128-block
    pts0 = (torch.rand(n, s, 3, generator=g) * 2.4 - 1.2).cuda()
    vd0 = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).cuda()
    w = torch.randn(n, s, 4, generator=g).cuda()
    captured, real = _spy(ops, monkeypatch)
    ops.lean_workspace_scope("render")
    full = _query_step(ops, net, embed, embeddirs, pts0, vd0, w)
    assert [(c["pd"], c["lean"]) for c in captured] == [(3, False)]
    call = captured[0]
    ops.lean_workspace_scope("all")
    lean = _query_step(ops, net, embed, embeddirs, pts0, vd0, w)
    assert [(c["pd"], c["lean"]) for c in captured[1:]] == [(3, True)]
    monkeypatch.setattr(ops, "nerf_wgrad", real)
    for what, a, b in zip(("raw", "d pts", "d viewdirs"), full[:3], lean[:3]):
        assert torch.equal(_words(a), _words(b)), what
    a, b = full[3].cpu().numpy(), lean[3].cpu().numpy()
    assert np.isfinite(b).all()
    keep = ~_derived_mask(3)
    np.testing.assert_array_equal(a.view(np.int32)[keep], b.view(np.int32)[keep])
    _judge("query P=%d" % call["P"], _derived(b, 3), _yardstick(ops, real, call),
           _fp64_reference(call["save"], call["grads"], call["P"], 3))
