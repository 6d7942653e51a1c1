"""TEST INFRASTRUCTURE shared by tests/test_gpu_skip_background.py and tests/test_emu_skip_background.py: the case bodies of
ops.inference_skip_background -- the two kernels behind it (scnerf_npp_fg_lambda, scnerf_npp_composite_fwd_skip) launched
stand-alone through a `route` object (tests/nerfpp_reference.py's convention: it holds buffers and calls the C ABI), and
the NeRF++ node and render_single_image with the switch on.  Every comparison but the error bound is for EQUALITY of bits.

References.  Kernel level: scnerf_npp_composite_fwd on the same inputs (nerfpp_reference.composite_inputs), with the
raw_bg rows of the skipped rays zeroed -- "what the call would return had the background network answered 0" --, run once
per size and route and shared.  Node level: the switch-off call on the same batch.  The bound of case 8 comes from the
derivation in DESIGN.md 4.7.5, bg_rgb_c <= bg_lambda (1 + 1e-6)^sb, capped at 1.001 eps for sb < 900 (the 0.1 % also covers
the fp32 rounding of the weights); `bound_in_fp64` checks the derivation itself on the fp64 oracle."""
import contextlib
import types

import numpy as np
import torch

from scnerf_amd import synthetic as synth
from tests import nerfpp_reference as NR

KEYS = NR.KEYS
FG_KEYS = ("fg_weights", "fg_rgb", "fg_depth", "bg_lambda")
IMAGE_KEYS = ("rgb", "fg_rgb", "fg_depth", "bg_rgb", "bg_depth", "bg_lambda")
EINVAL = -22
N, SF, SB = 24, 16, 12
INPUTS = ("raw_fg", "raw_bg", "fg_z", "z_max", "bg_z", "rd")

_REF = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a, b, err_msg=what)


# ---- kernel level ----------------------------------------------------------------------------------------------------
def composite(route, inp, zero_rows=()):
    """scnerf_npp_composite_fwd on `inp`, the raw_bg rows of the rays `zero_rows` zeroed: the reference of every kernel case,
    computed once per (route, size, rows) and left unchanged"""
    n, sf, sb = inp["fg_z"].shape[0], inp["fg_z"].shape[1], inp["bg_z"].shape[1]
    key = (route.__name__, n, sf, sb, tuple(zero_rows))
    if key not in _REF:
        raw_bg = inp["raw_bg"].copy()
        raw_bg[list(zero_rows)] = 0.0
        sh = NR.composite_shapes(n, sf, sb)
        bufs = {k: route.out(sh[k]) for k in KEYS}
        args = [route.inp(raw_bg if k == "raw_bg" else inp[k]) for k in INPUTS]
        route.call("scnerf_npp_composite_fwd", *args, *[bufs[k][1] for k in KEYS], n, sf, sb)
        _REF[key] = NR.collect(route, bufs)
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


def run_fg_lambda(route, inp, n):
    """scnerf_npp_fg_lambda on the first n rays into a NaN-filled buffer with a guard row on either side"""
    sf = inp["fg_z"].shape[1]
    buf = {"bg_lambda": route.out((n,))}
    route.call("scnerf_npp_fg_lambda", route.inp(inp["raw_fg"][:n]), route.inp(inp["fg_z"][:n]), route.inp(inp["z_max"][:n]),
               route.inp(inp["rd"][:n]), buf["bg_lambda"][1], n, sf)
    return NR.collect(route, buf)["bg_lambda"]


def fg_lambda_case(route, size):
    """case 1 (and 3): bg_lambda of the new kernel is the compositing kernel's, bit for bit, on all 7 rays and on one; the
    launch gives identical bytes twice"""
    inp = NR._cached(("composite_inputs",) + tuple(size), lambda: NR.composite_inputs(*size))
    ref = composite(route, inp)["bg_lambda"]
    for n in (NR.N_RAYS, 1):
        a, b = run_fg_lambda(route, inp, n), run_fg_lambda(route, inp, n)
        same_bits(a, ref[:n], "bg_lambda, n = %d" % n)
        same_bits(a, b, "bg_lambda twice, n = %d" % n)


def run_skip(route, inp, live, raw_bg="rows"):
    """scnerf_npp_composite_fwd_skip with a hand-made slot_of: the rays `live` (ascending) own rows 0, 1, ... of the compacted
    raw_bg, every other ray -1.  raw_bg: "rows" -- the live rows; None -- a null pointer; "empty" -- an empty buffer"""
    n, sf, sb = inp["fg_z"].shape[0], inp["fg_z"].shape[1], inp["bg_z"].shape[1]
    slot_of = np.full(n, -1, np.int32)
    slot_of[list(live)] = np.arange(len(live), dtype=np.int32)
    rows = {"rows": lambda: route.inp(inp["raw_bg"][list(live)]), None: lambda: None,
            "empty": lambda: route.inp(np.zeros((0, sb, 4), np.float32))}[raw_bg]()
    sh = NR.composite_shapes(n, sf, sb)
    bufs = {k: route.out(sh[k]) for k in KEYS}                  # NaN-filled: collect() shows that every element is written
    route.call("scnerf_npp_composite_fwd_skip", route.inp(inp["raw_fg"]), rows, route.inp(inp["fg_z"]), route.inp(inp["z_max"]),
               route.inp(inp["bg_z"]), route.inp(inp["rd"]), route.inp(slot_of), *[bufs[k][1] for k in KEYS], n, len(live), sf, sb)
    return NR.collect(route, bufs)


SKIP_PATTERNS = ("none", "all", "even_live", "odd_live")


def composite_skip_case(route, size, pattern):
    """case 2 (and 3): all eight outputs of composite_fwd_skip against composite_fwd with the skipped rows of raw_bg zeroed"""
    inp = NR._cached(("composite_inputs",) + tuple(size), lambda: NR.composite_inputs(*size))
    n = NR.N_RAYS
    live = {"none": range(n), "all": (), "even_live": range(0, n, 2), "odd_live": range(1, n, 2)}[pattern]
    live = list(live)
    dead = [r for r in range(n) if r not in live]
    ref = composite(route, inp, dead)
    runs = [run_skip(route, inp, live, "rows" if live else None), run_skip(route, inp, live, "rows" if live else "empty")]
    for got in runs:
        for k in KEYS:
            same_bits(got[k], ref[k], "%s (%s)" % (k, pattern))
        same_bits(got["rgb"][dead], got["fg_rgb"][dead], "rgb == fg_rgb on the skipped rays")
        assert not bits(got["bg_weights"][dead]).any() and not bits(got["bg_rgb"][dead]).any() and not bits(got["bg_depth"][dead]).any()
    if pattern == "none":                                       # nothing zeroed: the reference IS the plain call
        assert ref is composite(route, inp)


def argument_checks(route):
    """case 4: the C entries refuse bad arguments with SCN_EINVAL and leave the outputs as they were"""
    n, sf, sb = 3, 4, 5
    f = lambda *shape: route.inp(np.ones(shape, np.float32))
    ins = lambda: [f(n, sf, 4), f(n, sb, 4), f(n, sf), f(n), f(n, sb), f(n, 3), route.inp(np.arange(n, dtype=np.int32))]
    sh = NR.composite_shapes(n, sf, sb)

    def skip(n_=n, n_live=n, sf_=sf, sb_=sb, null=None):
        a, bufs = ins(), [route.out(sh[k]) for k in KEYS]
        outs = [b[1] for b in bufs]
        if null is not None:
            if null < 7:
                a[null] = None
            else:
                outs[null - 7] = None
        st = route.status("scnerf_npp_composite_fwd_skip", *a, *outs, n_, n_live, sf_, sb_)
        assert st == 0 or all(np.isnan(route.host(b[0])).all() for b in bufs), "an output was written by a refused call"
        return st

    assert skip(n_=-1) == EINVAL and skip(sf_=0) == EINVAL and skip(sb_=0) == EINVAL
    assert skip(n_live=-1) == EINVAL and skip(n_live=n + 1) == EINVAL
    for null in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14):   # every array but the two optional weight outputs
        assert skip(null=null) == EINVAL, null
    assert skip(null=1, n_live=0) == 0                          # no live ray: raw_bg may be null

    def lam(n_=n, sf_=sf, null=None):
        a, buf = [f(n, sf, 4), f(n, sf), f(n), f(n, 3)], route.out((n,))
        out = buf[1]
        if null is not None:
            if null < 4:
                a[null] = None
            else:
                out = None
        st = route.status("scnerf_npp_fg_lambda", *a, out, n_, sf_)
        assert np.isnan(route.host(buf[0])).all()
        return st

    assert lam(n_=-1) == EINVAL and lam(sf_=0) == EINVAL
    for null in range(5):
        assert lam(null=null) == EINVAL, null
    assert route.status("scnerf_npp_fg_lambda", None, None, None, None, route.out((1,))[1], 0, sf) == EINVAL
    assert lam(n_=0) == 0 and skip(n_=0, n_live=0) == 0         # n == 0 is a no-op


def cpu_tensors_are_rejected(ops):
    """case 4, the host layer: without a device (and outside the interpreter's context) a CPU tensor never reaches the library"""
    import pytest
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ops.npp_fg_lambda(z(2 * 3, 4), z(2, 3), z(2), z(2, 3))
    with pytest.raises(RuntimeError):
        ops.npp_composite_fwd_skip(z(2 * 3, 4), None, z(2, 3), z(2), z(2, 5), z(2, 3), z(2, dtype=torch.int32), 0)
    with pytest.raises(RuntimeError):
        ops.background_compact(z(4), 0.5)


def bound_in_fp64(size):
    """the derivation behind case 8 on the fp64 oracle: bg_rgb_c <= bg_lambda (1 + 1e-6)^sb on every ray of every kind"""
    inp = NR._cached(("composite_inputs",) + tuple(size), lambda: NR.composite_inputs(*size))
    o = NR.oracle_composite(*[torch.from_numpy(inp[k]).double() for k in INPUTS])
    cap = o["bg_lambda"][:, None] * (1.0 + 1e-6) ** size[1]
    assert bool((o["bg_rgb"] <= cap * (1.0 + 1e-12)).all()), float((o["bg_rgb"] / cap).max())
    assert bool((o["bg_weights"].sum(-1) <= (1.0 + 1e-6) ** size[1] * (1.0 + 1e-12)).all())


# ---- node level ------------------------------------------------------------------------------------------------------
ARGS = types.SimpleNamespace(max_freq_log2=10, max_freq_log2_viewdirs=4, netdepth=8, netwidth=256, use_viewdirs=True)


def make_net(device, seed=778, fg_density_bias=None):
    """NerfNet on synthetic.nerfpp_params; `fg_density_bias`: the foreground density head's bias set outright"""
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet
    net = NerfNet(ARGS)
    p = synth.nerfpp_params(seed)
    if fg_density_bias is not None:
        p["fg_net.sigma_layers.0.bias"] = torch.full_like(p["fg_net.sigma_layers.0.bias"], fg_density_bias)
    net.load_state_dict(p)
    return net.to(device)


def node_inputs(device, n=N, sf=SF, sb=SB, seed=41):
    """the suite's synthetic NeRF++ rays with evenly spaced foreground depths and sorted random inverse radii"""
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    o, d, near = (t.to(device) for t in synth.nerfpp_rays(n, seed=seed))
    g = torch.Generator().manual_seed(seed + 1)
    frac = torch.linspace(0.0, 1.0, sf)[None].expand(n, sf).contiguous().to(device)
    bg_z = torch.sort(0.01 + 0.98 * torch.rand(n, sb, generator=g), -1)[0].to(device)
    with torch.no_grad():
        far = TR.intersect_sphere(o, d)
    fg_z = near[:, None] + frac * (far - near)[:, None]
    return o, d, far, fg_z.contiguous(), bg_z


@contextlib.contextmanager
def switched(ops, eps):
    assert ops.inference_skip_background() is None
    ops.inference_skip_background(eps)
    try:
        yield
    finally:
        ops.inference_skip_background("off")


@contextlib.contextmanager
def arithmetic(ops, mode):
    """mode: "fp32" | "resident" | "fast" (resident with the one-product inference arithmetic)"""
    saved = (ops.mlp_arithmetic(), ops.inference_arithmetic())
    ops.mlp_arithmetic("fp32" if mode == "fp32" else "resident")
    ops.inference_arithmetic("fast" if mode == "fast" else "same")
    try:
        yield
    finally:
        ops.mlp_arithmetic(saved[0])
        ops.inference_arithmetic(saved[1])


def forward(net, inputs):
    with torch.no_grad():
        return net(*inputs)


def live_mask(lam, eps):
    return ~(lam <= eps)


def check_node_contract(on, off, live, what=""):
    """live rays: all eight outputs as switch off; skipped rays: the foreground's as switch off, zero background, rgb ==
    fg_rgb; the foreground outputs and bg_lambda as switch off on every ray"""
    dead = ~live
    assert list(on.keys()) == list(off.keys()) == list(KEYS)
    for k in KEYS:
        assert on[k].shape == off[k].shape and not torch.isnan(on[k]).any(), k
        same_bits(on[k][live], off[k][live], "%slive rays: %s" % (what, k))
    for k in FG_KEYS:
        same_bits(on[k], off[k], what + k)
    for k in ("bg_weights", "bg_rgb", "bg_depth"):
        assert not bits(on[k][dead]).any(), "%sskipped rays: %s is not +0" % (what, k)
    same_bits(on["rgb"][dead], on["fg_rgb"][dead], what + "skipped rays: rgb == fg_rgb")


def median_eps(off):
    """eps = the median of the switch-off bg_lambda, inside (0, 1); every ray is live or skipped, both sets non-empty"""
    lam = off["bg_lambda"]
    eps = float(lam.median())
    assert 0.0 < eps < 1.0, eps
    live = live_mask(lam, eps)
    k = int((lam <= eps).sum())
    assert int(live.sum()) + k == lam.numel() and 0 < k < lam.numel(), (k, lam.numel())
    return eps, live, k


def network_raws(ops, net, inputs):
    """raw_fg [n, sf, 4], raw_bg [n, sb, 4] of a forward-only call with the switch off: the node's own launches"""
    from scnerf_amd import _capi
    o, d, far, fg_z, bg_z = (t.contiguous().float() for t in inputs)
    n, sf, sb = o.shape[0], fg_z.shape[1], bg_z.shape[1]
    fg_pts, bg_pts, views = (torch.empty(s, dtype=torch.float32, device=o.device) for s in ((n * sf, 3), (n * sb, 4), (n, 3)))
    P = ops._p
    _capi.check(_capi.load().scnerf_npp_points_fwd(P(o), P(d), P(fg_z), P(bg_z), P(fg_pts), P(bg_pts), P(views), None, n, sf, sb,
                                                   ops._stream()), "scnerf_npp_points_fwd")
    raws = []
    for sub, pts, s, pd in ((net.fg_net, fg_pts, sf, 3), (net.bg_net, bg_pts, sb, 4)):
        wf, pl = ops.network_packs(sub, sub.flat_parameters(), False, n, pd, remap=sub.pack_remap())
        raws.append(ops.mlp_fwd(pts, views, s, wf, None, pd=pd, planes=pl).view(n, s, 4))
    return raws


def mixed_case(ops, device, mode):
    """cases 5 and 8: the switch at the median of bg_lambda"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        off = forward(net, inputs)
        eps, live, k = median_eps(off)
        before = ops.skip_empty_stats()
        ops.skip_background_stats(reset=True)
        with switched(ops, eps):
            on = forward(net, inputs)
        assert ops.skip_background_stats(reset=True) == {"rays": N, "skipped": k}
        assert ops.skip_empty_stats() == before
        check_node_contract(on, off, live)
        # case 8: what a skipped ray loses is its switch-off bg_rgb, at most eps (1 + 1e-6)^sb < 1.001 eps per channel
        dead = ~live
        lost = (off["rgb"][dead] - on["rgb"][dead]).abs()
        print("skip_background %s: eps %.6g, %d of %d skipped, largest bg_rgb(off) on them %.6g = %.6f eps, largest |d rgb| %.6g"
              % (mode, eps, k, N, float(off["bg_rgb"][dead].max()), float(off["bg_rgb"][dead].max()) / eps, float(lost.max())))
        assert bool((off["bg_rgb"][dead] <= eps * 1.001).all())
        # the fp64 oracle on the same network outputs stays inside the cap as well: the derivation, not the rounding
        raw_f, raw_b = network_raws(ops, net, inputs)
        o64 = NR.oracle_composite(raw_f.double().cpu(), raw_b.double().cpu(), inputs[3].double().cpu(), inputs[2].double().cpu(),
                                  inputs[4].double().cpu(), inputs[1].double().cpu())
        assert bool((o64["bg_rgb"][dead.cpu()] <= eps * 1.001).all()), float(o64["bg_rgb"][dead.cpu()].max()) / eps


def guarded_case(ops, device, guard="fallback"):
    """the resident arithmetic with the scale guard on (inference_skip_empty's contract): a live ray's outputs are those of a
    switch-off call on the live rays alone; the background pass takes the record sized for the dense pass"""
    saved = ops.resident_guard()
    with arithmetic(ops, "resident"):
        ops.resident_guard(guard)
        try:
            net, inputs = make_net(device), node_inputs(device)
            off = forward(net, inputs)
            eps, live, k = median_eps(off)
            sub = forward(net, tuple(t[live].contiguous() for t in inputs))
            with switched(ops, eps):
                on = forward(net, inputs)
        finally:
            ops.resident_guard(saved)
        for key in KEYS:
            same_bits(on[key][live], sub[key], "guard %s, live rays: %s" % (guard, key))
        check_node_contract(on, off, live, "guard %s: " % guard)           # (nothing trips on these weights: also the full batch's bits)


def nothing_skipped_case(ops, device, mode):
    """case 6: eps = 0 with every bg_lambda > 0 -- the compaction runs, every ray is live, today's launches, today's bits"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device), node_inputs(device)
        off = forward(net, inputs)
        assert bool((off["bg_lambda"] > 0).all())
        ops.skip_background_stats(reset=True)
        with switched(ops, 0.0):
            on = forward(net, inputs)
        assert ops.skip_background_stats(reset=True) == {"rays": N, "skipped": 0}
        for k in KEYS:
            same_bits(on[k], off[k], k)


def everything_skipped_case(ops, device, mode, monkeypatch):
    """case 7: an opaque foreground (density bias 1e3) -- no ray is live, the background network is never launched"""
    with arithmetic(ops, mode):
        net, inputs = make_net(device, fg_density_bias=1e3), node_inputs(device)
        off = forward(net, inputs)
        eps = 1e-3
        assert bool((off["bg_lambda"] <= eps).all()), float(off["bg_lambda"].max())
        launches = []
        real = ops.mlp_fwd
        monkeypatch.setattr(ops, "mlp_fwd", lambda *a, **kw: (launches.append(kw.get("pd", 3)), real(*a, **kw))[1])
        ops.skip_background_stats(reset=True)
        with switched(ops, eps):
            on = forward(net, inputs)
        monkeypatch.setattr(ops, "mlp_fwd", real)
        assert launches == [3], launches
        assert ops.skip_background_stats(reset=True) == {"rays": N, "skipped": N}
        check_node_contract(on, off, torch.zeros(N, dtype=torch.bool, device=off["rgb"].device))


def tracking_call_case(ops, device, mode):
    """case 9: a call that tracks gradients does not notice the switch"""
    with arithmetic(ops, mode):
        net = make_net(device)
        o, d, far, fg_z, bg_z = node_inputs(device, n=4)

        def step():
            net.zero_grad()
            oo = o.clone().requires_grad_(True)
            ret = net(oo, d, far, fg_z, bg_z)
            (ret["rgb"].sum() + ret["bg_depth"].sum()).backward()
            return {k: v.detach().clone() for k, v in ret.items()}, oo.grad.clone()

        a = step()
        ops.skip_background_stats(reset=True)
        with switched(ops, float(a[0]["bg_lambda"].median())):
            b = step()
        assert ops.skip_background_stats() == {"rays": 0, "skipped": 0}          # the compaction never ran
        for k in KEYS:
            same_bits(a[0][k], b[0][k], k)
        same_bits(a[1], b[1], "d ray_o")
        assert float(b[1].abs().max()) > 0


def switch_validation(ops, monkeypatch):
    """case 10"""
    import pytest
    env = "SCNERF_INFER_SKIP_BACKGROUND"
    assert ops.inference_skip_background() is None
    for bad in (-0.1, 1.0, 2.0, "x", "on", float("nan"), True):
        with pytest.raises(ValueError):
            ops.inference_skip_background(bad)
        assert ops.inference_skip_background() is None
    assert ops.inference_skip_background(0.25) == 0.25 and ops.inference_skip_background() == 0.25
    assert ops.inference_skip_background(0) == 0.0
    assert ops.inference_skip_background("off") is None and ops.inference_skip_background() is None
    assert ops.inference_skip_background(0.1) == float(torch.tensor(0.1, dtype=torch.float32))     # the fp32 value compared with
    ops.inference_skip_background("off")
    monkeypatch.setenv(env, "0.5")
    assert ops._FloatSwitch(env, 0.0, 1.0, "inference_skip_background")() == 0.5
    monkeypatch.setenv(env, "off")
    assert ops._FloatSwitch(env, 0.0, 1.0, "inference_skip_background")() is None
    for bad in ("2", "-1", "yes"):
        monkeypatch.setenv(env, bad)
        with pytest.raises(ValueError):
            ops._FloatSwitch(env, 0.0, 1.0, "inference_skip_background")
    assert ops.skip_background_stats(reset=True).keys() == {"rays", "skipped"}
    assert ops.skip_background_stats() == {"rays": 0, "skipped": 0}


def render_single_image_case(ops, device, mode, rank):
    """case 11: two cascade levels on a 6 x 4 image in chunks of 10 rays, world_size 1.  Both levels carry the same weights
    (two module instances): the finer level then sees about the same transmittances, so that the threshold -- the median of
    level 0 -- leaves rays live at both levels, which the last comparison needs"""
    from collections import OrderedDict
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    Hh, Ww = 6, 4
    o, d, near = synth.nerfpp_rays(Hh * Ww, seed=41)

    class Sampler:
        H, W = Hh, Ww

        def get_all(self, camera_model, camera_idx, sampler, rank):
            return OrderedDict(ray_o=o, ray_d=d, depth=torch.zeros(Hh * Ww), rgb=None, mask=None, min_depth=near, img_name="x")

    with arithmetic(ops, mode):
        models = OrderedDict(cascade_level=2, cascade_samples=[10, 6], net_0=make_net(device, 781), net_1=make_net(device, 781))
        render = lambda: [{k: v.reshape(Hh * Ww, -1) for k, v in lvl.items()}
                          for lvl in TR.render_single_image(rank, 1, models, Sampler(), 10, None, camera_idx=None)]
        off = render()
        eps, live0, k0 = median_eps({"bg_lambda": off[0]["bg_lambda"].reshape(-1)})
        ops.skip_background_stats(reset=True)
        with switched(ops, eps):
            on = render()
        skipped = [int((off[m]["bg_lambda"] <= eps).sum()) for m in range(2)]
        assert ops.skip_background_stats(reset=True) == {"rays": 2 * Hh * Ww, "skipped": sum(skipped)}
        live_so_far = torch.ones(Hh * Ww, dtype=torch.bool)
        for m in range(2):
            assert list(on[m].keys()) == list(IMAGE_KEYS)
            for k in ("fg_rgb", "fg_depth", "bg_lambda"):            # the foreground chain never sees the switch
                same_bits(on[m][k], off[m][k], "level %d: %s" % (m, k))
            dead = (on[m]["bg_lambda"] <= eps).reshape(-1)
            same_bits(on[m]["rgb"][dead], on[m]["fg_rgb"][dead], "level %d: rgb == fg_rgb behind an opaque foreground" % m)
            assert not bits(on[m]["bg_rgb"][dead]).any() and not bits(on[m]["bg_depth"][dead]).any()
            live_so_far &= ~dead
            for k in IMAGE_KEYS:
                same_bits(on[m][k][live_so_far], off[m][k][live_so_far], "level %d, rays live so far: %s" % (m, k))
        print("render_single_image %s: eps %.6g, skipped per level %s, live at both levels %d" % (mode, eps, skipped, int(live_so_far.sum())))
        assert 0 < int(live_so_far.sum()), "no ray is live at both levels"
        assert skipped[0] == k0 == int((~live0).sum())
