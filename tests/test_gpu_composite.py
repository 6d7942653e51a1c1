"""GPU twin of the any-sample-count cases of tests/test_emu_composite.py (pytest -m gpu): scnerf_composite_fwd / _bwd and
scnerf_ray_reduce through ops.composite_fwd, ops.composite_bwd and ops.ray_reduce at sample counts that are no multiple of
the 64-lane pass, against the fp64 oracle under the bound of tests/composite_reference.py -- the hardware's side of what
the interpreter shows: real wave shuffles in a partial pass, the LDS transmittance row, dead waves and dead lanes."""
import numpy as np
import pytest
import torch

from tests import composite_reference as CR

pytestmark = pytest.mark.gpu

FWD_NAMES = ("weights", "rgb", "acc", "depth", "disp")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from scnerf_amd import ops as _ops
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(shape):
    """-> (cuda buffer with one NaN row before and one after, its interior view of `shape`)"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[1:-1]


def gpu_composite_fwd(ops, inp, wb):
    """ops.composite_fwd, and the same launch straight through the C ABI into buffers with a NaN row before and after every
    output (ops allocates exact sizes: a write by a dead wave or lane would go unseen there): guards intact, same bits."""
    from scnerf_amd import _capi
    raw, z, rays, noise = dev(inp["raw"]), dev(inp["z"]), dev(inp["rays"]), dev(inp["noise"])
    rgb, disp, acc, w, depth = ops.composite_fwd(raw, z, rays, noise, bool(wb))
    got = dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth)
    n, s = z.shape
    bufs = {k: guarded(tuple(v.shape)) for k, v in got.items()}
    p = lambda t_: None if t_ is None else t_.data_ptr()
    st = _capi.load().scnerf_composite_fwd(p(raw), p(z), p(rays), rays.shape[1], p(noise), int(wb),
                                           *[p(bufs[k][1]) for k in ("rgb", "disp", "acc", "depth", "weights")], n, s,
                                           _capi.current_stream())
    _capi.check(st, "scnerf_composite_fwd")
    for k, (buf, rows) in bufs.items():
        CR.assert_guards(buf, k)
        assert torch.equal(rows, got[k]), k
    return {k: v.cpu().numpy() for k, v in got.items()}


def gpu_composite_bwd(ops, inp, wb, g_raw_in=None, want_d_rays_d=True):
    from scnerf_amd import _capi
    raw, z, rays, noise = dev(inp["raw"]), dev(inp["z"]), dev(inp["rays"]), dev(inp["noise"])
    g = [dev(inp[k]) for k in ("g_rgb", "g_disp", "g_acc", "g_depth")] + [dev(g_raw_in)]
    d_raw, d_rd = ops.composite_bwd(raw, z, rays, noise, bool(wb), *g, want_d_rays_d=want_d_rays_d)
    assert (d_rd is None) == (not want_d_rays_d)
    n, s = z.shape
    b_raw, b_rd = guarded((n, s, 4)), guarded((n, 3))
    p = lambda t_: None if t_ is None else t_.data_ptr()
    st = _capi.load().scnerf_composite_bwd(p(raw), p(z), p(rays), rays.shape[1], p(noise), int(wb), *[p(t_) for t_ in g],
                                           p(b_raw[1]), p(b_rd[1]) if want_d_rays_d else None, n, s, _capi.current_stream())
    _capi.check(st, "scnerf_composite_bwd")
    CR.assert_guards(b_raw[0], "d_raw")
    assert torch.equal(b_raw[1], d_raw)
    if want_d_rays_d:
        CR.assert_guards(b_rd[0], "d_rays_d")
        assert torch.equal(b_rd[1], d_rd)
    else:
        assert bool(torch.isnan(b_rd[0]).all())
    return d_raw.cpu().numpy(), d_rd.cpu().numpy() if want_d_rays_d else None


@pytest.mark.parametrize("case", CR.CASES, ids=CR.case_id)
def test_composite_any_sample_count_vs_fp64(ops, case):
    """tests/test_emu_composite.py::test_composite_any_sample_count_vs_fp64 on the GPU: the same inputs, reference and bound
    (K = 4 x max(the fp32 oracle's own error, 2^-23)); the measured worst ratios of both routes are in that docstring."""
    inp, _, _ = CR.references(case)
    got = gpu_composite_fwd(ops, inp, case[3])
    got["d_raw"], got["d_rays_d"] = gpu_composite_bwd(ops, inp, case[3])
    CR.check_zero_direction_ray(got)
    CR.check(case, got, FWD_NAMES + ("d_raw", "d_rays_d"))


@pytest.mark.parametrize("case", [c for c in CR.CASES if c[0] in (70, 264)], ids=CR.case_id)
def test_composite_backward_options_any_sample_count(ops, case):
    """a gradient arriving at raw is added (b == a + extra); without d_rays_d the d_raw is bit for bit the same"""
    inp, _, _ = CR.references(case)
    a, _ = gpu_composite_bwd(ops, inp, case[3])
    extra = np.random.default_rng(case[0]).standard_normal(a.shape).astype(np.float32)
    b, _ = gpu_composite_bwd(ops, inp, case[3], g_raw_in=extra)
    np.testing.assert_allclose(b, a + extra, rtol=1e-6, atol=1e-7)
    c, none = gpu_composite_bwd(ops, inp, case[3], want_d_rays_d=False)
    assert none is None
    np.testing.assert_array_equal(c.view(np.int32), a.view(np.int32))


@pytest.mark.parametrize("with_views", [True, False], ids=["views", "no_views"])
@pytest.mark.parametrize("ray_stride", [8, 11])
@pytest.mark.parametrize("s", CR.REDUCE_SIZES)
def test_ray_reduce_any_sample_count(ops, s, ray_stride, with_views):
    def run(d_pts, d_views, z, extra, prior, accumulate):
        buf, rows = guarded(prior.shape)
        rows.copy_(dev(prior))
        out = ops.ray_reduce(dev(d_pts), dev(d_views), dev(z), dev(extra), rows, accumulate)
        assert out.data_ptr() == rows.data_ptr()
        b = buf.cpu().numpy()
        assert np.isnan(b[0]).all() and np.isnan(b[-1]).all(), "d_rays: written outside its rows"
        return b[1:-1].copy()
    CR.check_reduce(run, s, ray_stride, with_views)
