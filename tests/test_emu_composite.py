"""Compositing kernels (HIP source under the CPU SIMT interpreter) vs the reference's golden
vectors (values and autograd gradients of raw2outputs)."""
import numpy as np
import pytest
import torch

from tests.emu import harness as H

pytestmark = pytest.mark.emu


def rel_close(a, b, tol, what):
    scale = float(np.abs(b).max()) + 1e-30
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, "%s: max err %g (scale %g)" % (what, err, scale)


@pytest.mark.parametrize("tag", ["s64", "s192"])
@pytest.mark.parametrize("wb", [0, 1])
@pytest.mark.parametrize("with_noise", [0, 1])
def test_composite_forward_backward_golden(golden, tag, wb, with_noise):
    g = golden("composite")
    raw, z, rays_d = g[tag + "/raw"], g[tag + "/z"], g[tag + "/rays_d"]
    n, s = z.shape
    rays = np.zeros((n, 8), np.float32)
    rays[:, 3:6] = rays_d
    noise = g[tag + "/noise"] if with_noise else None
    rgb = np.zeros((n, 3), np.float32); disp = np.zeros(n, np.float32); acc = np.zeros(n, np.float32)
    depth = np.zeros(n, np.float32); w = np.zeros((n, s), np.float32)
    H.call("scnerf_composite_fwd", raw, z, rays, 8, noise, wb, rgb, disp, acc, depth, w, n, s, None)
    key = "%s/wb%d_n%d/" % (tag, wb, with_noise)
    # alpha = 1 - exp(-a*dist) cancels for tiny a*dist: a 1-ulp difference of expf (libm vs ATen) is 6e-8 absolute
    np.testing.assert_allclose(w, g[key + "weights"], rtol=2e-6, atol=1.5e-7)
    np.testing.assert_allclose(rgb, g[key + "rgb"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(acc, g[key + "acc"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(depth, g[key + "depth"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(disp, g[key + "disp"], rtol=2e-5)
    d_raw = np.full((n, s, 4), np.nan, np.float32)
    d_rd = np.full((n, 3), np.nan, np.float32)
    H.call("scnerf_composite_bwd", raw, z, rays, 8, noise, wb, g[tag + "/g_rgb"], g[tag + "/g_disp"],
           g[tag + "/g_acc"], g[tag + "/g_depth"], None, d_raw, d_rd, n, s, None)
    ref = g[key + "g_raw"]
    for r in range(n):                       # per ray: gradients span many orders of magnitude
        rel_close(d_raw[r], ref[r], 2e-4, "d_raw ray %d" % r)
    rel_close(d_rd, g[key + "g_rays_d"], 2e-4, "d_rays_d")


def test_composite_backward_extra_raw_gradient_and_null_inputs(golden):
    g = golden("composite")
    raw, z, rays_d = g["s64/raw"], g["s64/z"], g["s64/rays_d"]
    n, s = z.shape
    rays = np.zeros((n, 11), np.float32)
    rays[:, 3:6] = rays_d
    a = np.zeros((n, s, 4), np.float32); b = np.zeros((n, s, 4), np.float32)
    extra = np.random.default_rng(0).standard_normal((n, s, 4)).astype(np.float32)
    H.call("scnerf_composite_bwd", raw, z, rays, 11, None, 0, g["s64/g_rgb"], None, None, None, None, a, None, n, s, None)
    H.call("scnerf_composite_bwd", raw, z, rays, 11, None, 0, g["s64/g_rgb"], None, None, None, extra, b, None, n, s, None)
    np.testing.assert_allclose(b, a + extra, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("s", [64, 192, 70])
def test_ray_reduce(s):
    rng = np.random.default_rng(s)
    n = 9
    d_pts = rng.standard_normal((n, s, 3)).astype(np.float32)
    d_views = rng.standard_normal((n, s, 3)).astype(np.float32)
    z = rng.random((n, s)).astype(np.float32)
    extra = rng.standard_normal((n, 3)).astype(np.float32)
    out = np.full((n, 11), np.nan, np.float32)
    H.call("scnerf_ray_reduce", d_pts, d_views, z, extra, out, 11, 0, n, s, None)
    exp = np.zeros((n, 11))
    exp[:, 0:3] = d_pts.astype(np.float64).sum(1)
    exp[:, 3:6] = (d_pts.astype(np.float64) * z[..., None]).sum(1) + extra
    exp[:, 8:11] = d_views.astype(np.float64).sum(1)
    np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5)
    H.call("scnerf_ray_reduce", d_pts, d_views, z, None, out, 11, 1, n, s, None)
    exp2 = exp.copy()
    exp2[:, 0:6] += exp[:, 0:6]
    exp2[:, 3:6] -= extra
    exp2[:, 8:11] += exp[:, 8:11]
    np.testing.assert_allclose(out, exp2, rtol=1e-5, atol=1e-5)


# ---- sample counts that are no multiple of the 64-lane pass, against fp64 (tests/composite_reference.py) ----------------
from tests import composite_reference as CR  # noqa: E402

FWD_NAMES = ("weights", "rgb", "acc", "depth", "disp")


def emu_composite_fwd(inp, wb, want_depth=True):
    """scnerf_composite_fwd into buffers with a NaN row before and after each output -> (name -> array)"""
    n, s = inp["z"].shape
    bufs = {k: CR.guarded(sh) for k, sh in (("rgb", (n, 3)), ("disp", (n,)), ("acc", (n,)), ("depth", (n,)), ("weights", (n, s)))}
    H.call("scnerf_composite_fwd", inp["raw"], inp["z"], inp["rays"], inp["rays"].shape[1], inp["noise"], wb,
           *[H.ptr(bufs[k][1]) for k in ("rgb", "disp", "acc", "depth", "weights")], n, s, None)
    for k, (buf, _) in bufs.items():
        CR.assert_guards(buf, k)
    return {k: v[1] for k, v in bufs.items()}


def emu_composite_bwd(inp, wb, g_raw_in=None, want_d_rays_d=True):
    n, s = inp["z"].shape
    d_raw, d_rd = CR.guarded((n, s, 4)), CR.guarded((n, 3))
    H.call("scnerf_composite_bwd", inp["raw"], inp["z"], inp["rays"], inp["rays"].shape[1], inp["noise"], wb, inp["g_rgb"],
           inp["g_disp"], inp["g_acc"], inp["g_depth"], g_raw_in, H.ptr(d_raw[1]), H.ptr(d_rd[1]) if want_d_rays_d else None,
           n, s, None)
    CR.assert_guards(d_raw[0], "d_raw")
    if want_d_rays_d:
        CR.assert_guards(d_rd[0], "d_rays_d")
    else:
        assert np.isnan(d_rd[0]).all()
    return d_raw[1], d_rd[1] if want_d_rays_d else None


@pytest.mark.parametrize("case", CR.CASES, ids=CR.case_id)
def test_composite_any_sample_count_vs_fp64(case):
    """Forward maps, weights, d_raw per ray and d_rays_d at s in {2, 33, 63, 65, 70, 129, 200, 264} -- fewer than one pass,
    a partial last pass, more than 256 samples -- on 7 rays of mixed kinds (plain, saturated, tied depths, empty, a zero
    direction) against the fp64 oracle, within K = 4 x max(the fp32 oracle's own error, 2^-23), every output inside NaN
    guard rows.  Worst kernel error / fp32-oracle error measured over these cases (tests/composite_reference.py):
    interpreter  forward outputs <= 0.87 (disp; errors <= 1.0e-7), d_raw 1.97 (s = 2; errors <= 3.1e-7), d_rays_d 1.53 (<= 2.9e-7)
    MI355X       forward outputs <= 0.87 (disp; errors <= 1.0e-7), d_raw 1.97 (s = 2; errors <= 3.1e-7), d_rays_d 1.60 (<= 4.6e-7)"""
    inp, _, _ = CR.references(case)
    got = emu_composite_fwd(inp, case[3])
    got["d_raw"], got["d_rays_d"] = emu_composite_bwd(inp, case[3])
    CR.check_zero_direction_ray(got)
    CR.check(case, got, FWD_NAMES + ("d_raw", "d_rays_d"))


@pytest.mark.parametrize("case", [c for c in CR.CASES if c[0] in (70, 264)], ids=CR.case_id)
def test_composite_backward_options_any_sample_count(case):
    """a gradient arriving at raw is added (b == a + extra); without d_rays_d the d_raw is bit for bit the same"""
    inp, _, _ = CR.references(case)
    a, _ = emu_composite_bwd(inp, case[3])
    extra = np.random.default_rng(case[0]).standard_normal(a.shape).astype(np.float32)
    b, _ = emu_composite_bwd(inp, case[3], g_raw_in=extra)
    np.testing.assert_allclose(b, a + extra, rtol=1e-6, atol=1e-7)
    c, none = emu_composite_bwd(inp, case[3], want_d_rays_d=False)
    assert none is None
    np.testing.assert_array_equal(c.view(np.int32), a.view(np.int32))


def emu_ray_reduce(d_pts, d_views, z, extra, prior, accumulate):
    n, s = z.shape
    buf, rows = CR.guarded(prior.shape)
    rows[:] = prior
    H.call("scnerf_ray_reduce", d_pts, d_views, z, extra, H.ptr(rows), prior.shape[1], int(accumulate), n, s, None)
    assert np.isnan(buf[0]).all() and np.isnan(buf[-1]).all(), "d_rays: written outside its rows"
    return rows.copy()


@pytest.mark.parametrize("with_views", [True, False], ids=["views", "no_views"])
@pytest.mark.parametrize("ray_stride", [8, 11])
@pytest.mark.parametrize("s", CR.REDUCE_SIZES)
def test_ray_reduce_any_sample_count(s, ray_stride, with_views):
    CR.check_reduce(emu_ray_reduce, s, ray_stride, with_views)
