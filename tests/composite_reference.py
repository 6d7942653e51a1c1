"""TEST INFRASTRUCTURE: inputs, fp64 reference and error bound of the compositing / ray-reduction tests at sample counts
that are no multiple of the 64-lane pass (tests/test_emu_composite.py on the CPU SIMT interpreter, tests/test_gpu_composite.py
on the GPU: both routes see the same numbers and the same bound).

Reference: oracle.scnerf_oracle.composite on torch.float64 leaves, gradients by autograd.  Bound: the same oracle in
torch.float32 on the same inputs gives the reference arithmetic's own error E32 against fp64; a kernel output must stay
within K * max(E32, 2^-23) -- K for the device expf (ulps from libm's, in 1 - e) and the other summation order, 2^-23 (one
fp32 rounding of the largest entry) as the floor where the fp32 oracle happens to round exactly.

Metric: largest |x - fp64| over a tensor / largest |fp64| entry of that tensor.  d_raw: that figure per ray (a ray's
gradients span orders of magnitude against its neighbours'), worst over the rays whose own largest entry is at least 1e-3
of the tensor's (below, the figure is a ratio of roundings).  disp: over the rays with any opacity -- a ray with acc == 0
has disp = 1 / max(1e-10, 0) = 1e10 on every side, asserted exactly, which would otherwise be the tensor's scale."""
import numpy as np
import torch

from oracle import scnerf_oracle as O

K = 4.0
FLOOR = 2.0 ** -23
N_RAYS = 7            # not a multiple of the 4 rays per workgroup: the last workgroup has a dead wave
ZERO_RAY = 6          # rays_d == 0: d_rays_d = 0, acc = 0, disp = 1e10 (composite.hip: `norm > 0 ? ... : 0`)
KINDS = ("plain", "opaque", "tied", "empty", "plain", "opaque", "plain")
SIZES = (2, 33, 63, 65, 70, 129, 200, 264)
# (s, ray_stride, with_noise, white_bkgd): every size with and without noise, both strides and both backgrounds per size
CASES = [(s, (8, 11)[(k + j) % 2], j, (k + j + k // 2) % 2) for k, s in enumerate(SIZES) for j in (1, 0)]
REDUCE_SIZES = (2, 33, 70, 264)

WORST = {}            # tensor name -> (ratio, kernel error, E32, case) of the worst ratio this session measured


def case_id(case):
    return "s%d_stride%d_noise%d_wb%d" % case


def inputs(s, ray_stride, with_noise, seed=None):
    """n = 7 rays of four kinds in ONE call (every tensor's largest entry is O(1)) + the zero-direction ray"""
    rng = np.random.default_rng(1000 + s if seed is None else seed)
    n = N_RAYS
    raw = rng.standard_normal((n, s, 4)).astype(np.float32)
    z = np.sort(2.0 + 4.0 * rng.random((n, s)), -1).astype(np.float32)
    noise = np.clip(rng.standard_normal((n, s)), -4.0, 4.0).astype(np.float32)
    for r, kind in enumerate(KINDS):
        g = rng.standard_normal(s)
        if kind == "plain":
            raw[r, :, 3] = 10.0 * g
        elif kind == "opaque":            # exp saturates to 0: q = 1e-10, the transmittance runs through the denormals
            raw[r, :, 3] = rng.choice(np.array([-1.0, 0.5, 300.0, 3000.0]), size=s)
        elif kind == "tied":              # neighbours equal: dist = 0
            z[r, 1::2] = z[r, 0:2 * (s // 2):2]
            raw[r, :, 3] = 30.0 * g
        elif kind == "empty":             # sigma + noise < 0 everywhere
            raw[r, :, 3] = -5.0 - 10.0 * np.abs(g)
    rays = rng.standard_normal((n, ray_stride)).astype(np.float32)      # rays_d ~ N(0, 1), not unit: d|d| is live
    rays[ZERO_RAY, 3:6] = 0.0
    return dict(raw=raw, z=z, rays=rays, noise=noise if with_noise else None,
                g_rgb=rng.standard_normal((n, 3)).astype(np.float32),
                g_disp=(0.1 * rng.standard_normal(n)).astype(np.float32),
                g_acc=rng.standard_normal(n).astype(np.float32),
                g_depth=rng.standard_normal(n).astype(np.float32))


def oracle(inp, white_bkgd, dtype):
    """-> dict of float64 arrays: the five maps and the autograd gradients d_raw, d_rays_d in arithmetic `dtype`"""
    cast = lambda a: torch.from_numpy(a).to(dtype)
    raw = cast(inp["raw"]).requires_grad_(True)
    rays_d = cast(inp["rays"][:, 3:6].copy()).requires_grad_(True)
    noise = None if inp["noise"] is None else cast(inp["noise"])
    rgb, disp, acc, w, depth = O.composite(raw, cast(inp["z"]), rays_d, noise, bool(white_bkgd))
    ((rgb * cast(inp["g_rgb"])).sum() + (disp * cast(inp["g_disp"])).sum() + (acc * cast(inp["g_acc"])).sum()
     + (depth * cast(inp["g_depth"])).sum()).backward()
    out = dict(rgb=rgb, disp=disp, acc=acc, weights=w, depth=depth, d_raw=raw.grad, d_rays_d=rays_d.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


_ORACLES = {}


def references(case):
    """(inputs, fp64 oracle, fp32 oracle) of a case, computed once per session and shared"""
    if case not in _ORACLES:
        s, stride, with_noise, wb = case
        inp = inputs(s, stride, with_noise)
        _ORACLES[case] = (inp, oracle(inp, wb, torch.float64), oracle(inp, wb, torch.float32))
    return _ORACLES[case]


def metric(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) / (float(np.abs(ref).max()) + 1e-300)


def metric_per_ray(x, ref):
    n = ref.shape[0]
    x = np.asarray(x, np.float64).reshape(n, -1)
    ref = ref.reshape(n, -1)
    scale = np.abs(ref).max(1)
    keep = scale >= 1e-3 * scale.max()
    assert keep.sum() >= 2, "the d_raw metric needs rays of comparable gradients"
    return float((np.abs(x - ref).max(1)[keep] / scale[keep]).max())


def check(case, got, names):
    """`got`: name -> float32 array of the kernel.  Prints every figure, then asserts the bound; -> name -> ratio."""
    _, o64, o32 = references(case)
    lit = o64["disp"] < 1e9                 # (an unlit ray: acc == 0, disp == 1e10)
    assert lit.sum() >= 2 and not lit[ZERO_RAY]
    ratios, failed = {}, []
    for name in names:
        x = np.asarray(got[name])
        if name == "d_raw":
            err, e32 = metric_per_ray(x, o64[name]), metric_per_ray(o32[name], o64[name])
        elif name == "disp":
            err, e32 = metric(x[lit], o64[name][lit]), metric(o32[name][lit], o64[name][lit])
            np.testing.assert_array_equal(x[~lit], np.float32(1e10))
        else:
            err, e32 = metric(x, o64[name]), metric(o32[name], o64[name])
        ratio = err / max(e32, FLOOR)
        ratios[name] = ratio
        print("composite %s %-8s kernel %.3g  fp32 oracle %.3g  ratio %.3g" % (case_id(case), name, err, e32, ratio))
        if ratio > WORST.get(name, (0.0,))[0]:
            WORST[name] = (ratio, err, e32, case_id(case))
        if not ratio <= K:                  # (also catches NaN)
            failed.append((name, err, e32, ratio))
    assert not failed, (case_id(case), failed)
    # ceilings: the golden test's tolerances
    if "weights" in names:
        np.testing.assert_allclose(got["weights"], o64["weights"], rtol=2e-6, atol=1.5e-7)
    if "d_raw" in names:
        assert metric_per_ray(got["d_raw"], o64["d_raw"]) <= 2e-4
    if "d_rays_d" in names:
        assert metric(got["d_rays_d"], o64["d_rays_d"]) <= 2e-4
    return ratios


def check_zero_direction_ray(got):
    """the kernel's documented behaviour on a ray with rays_d == 0"""
    r = ZERO_RAY
    assert got["acc"][r] == 0.0 and got["disp"][r] == np.float32(1e10) and got["depth"][r] == 0.0
    assert not got["weights"][r].any()
    if "d_rays_d" in got:
        assert not got["d_rays_d"][r].any() and not got["d_raw"][r].any()


def guarded(shape, dtype=np.float32):
    """-> (buffer with one NaN row before and one after, its interior view of `shape`)"""
    buf = np.full((shape[0] + 2,) + tuple(shape[1:]), np.nan, dtype)
    return buf, buf[1:-1]


def assert_guards(buf, what):
    """poison survives: no write by a dead wave or a dead lane outside the n rows; everything inside is written"""
    b = buf.detach().cpu().numpy() if torch.is_tensor(buf) else buf
    assert np.isnan(b[0]).all() and np.isnan(b[-1]).all(), what + ": written outside its rows"
    assert not np.isnan(b[1:-1]).any(), what + ": not written everywhere inside"


def reduce_inputs(s, ray_stride, seed=None):
    rng = np.random.default_rng(7000 + s if seed is None else seed)
    n = 9
    return dict(d_pts=rng.standard_normal((n, s, 3)).astype(np.float32),
                d_views=rng.standard_normal((n, s, 3)).astype(np.float32),
                z=rng.random((n, s)).astype(np.float32), extra=rng.standard_normal((n, 3)).astype(np.float32),
                prior=rng.standard_normal((n, ray_stride)).astype(np.float32))


def reduce_expected(inp, ray_stride, with_views):
    """fp64 sums of one overwrite call: [n, ray_stride] (columns 6:8 zero, 8:11 only when the stride holds them)"""
    n = inp["z"].shape[0]
    exp = np.zeros((n, ray_stride))
    d = inp["d_pts"].astype(np.float64)
    exp[:, 0:3] = d.sum(1)
    exp[:, 3:6] = (d * inp["z"].astype(np.float64)[..., None]).sum(1) + inp["extra"]
    if ray_stride > 8 and with_views:
        exp[:, 8:11] = inp["d_views"].astype(np.float64).sum(1)
    return exp


def check_reduce(run, s, ray_stride, with_views):
    """`run(d_pts, d_views | None, z, extra | None, prior [n, stride], accumulate) -> [n, stride]` float32 array of one
    scnerf_ray_reduce call on a row buffer pre-filled with `prior`, guards checked by the route."""
    inp = reduce_inputs(s, ray_stride)
    exp = reduce_expected(inp, ray_stride, with_views)
    dv = inp["d_views"] if with_views else None
    poison = np.full_like(inp["prior"], np.nan)                 # overwrite: whatever is there goes, 6:8 become zero
    out = run(inp["d_pts"], dv, inp["z"], inp["extra"], poison, False)
    np.testing.assert_allclose(out, exp, rtol=1e-5, atol=1e-5)
    assert not out[:, 6:8].any()
    prior = inp["prior"].copy()
    out = run(inp["d_pts"], dv, inp["z"], None, prior.copy(), True)
    exp2 = exp + prior
    exp2[:, 3:6] -= inp["extra"]
    np.testing.assert_allclose(out, exp2, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(out[:, 6:8], prior[:, 6:8])   # accumulate: near / far columns untouched
