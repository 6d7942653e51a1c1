"""TEST INFRASTRUCTURE: cases, fp64 references and error bounds of the stand-alone tests of the NeRF++ per-ray kernels
(csrc/nerfpp.hip): tests/test_emu_nerfpp.py on the CPU SIMT interpreter and tests/test_gpu_nerfpp_kernels.py on the GPU.
Both routes run the SAME launches (the run_* functions below, through a `route` object that only knows how to hold a
buffer and call the C ABI), see the same inputs, the same references and the same bounds.

References.  Compositing: `oracle_composite` (the compositing half of NerfNet.forward).  Geometry: intersect_sphere and
depth2pts_outside of oracle.nerfpp_oracle.  Each runs once on torch.float64 leaves (the reference; gradients by autograd)
and once on torch.float32 leaves (the yardstick E32: the reference arithmetic's own error against fp64).  Sampler forward and
jitter forward: bit for bit against the fp32 oracle on the CPU.  Sampler backward: the fp64 scatter-add of g (1 - t) / g t
over the forward's (below, above, t); yardstick: the same sum taken sequentially in fp32.  Jitter backward: fp64 autograd,
to 2e-6 of the largest entry.  The module asserts that every oracle output is finite, in both precisions, on every case.

Metric: largest |x - fp64| over a tensor / largest |fp64| entry of that tensor.  Per-sample and per-ray gradients and the
geometry tensors take that figure per ray and the worst ray counts; for d_raw_fg, d_raw_bg and d_fg_z only the rays whose
own largest entry is at least 1e-3 of the tensor's (below, the figure is a ratio of roundings: an empty ray's gradient IS
zero, an opaque foreground leaves the background nothing through rgb), and at least 5 of the 7 rays must remain.
Bound: figure <= K * max(E32, 2^-23), K per family the smallest power of two >= twice the worst ratio measured on either
route, never under 4 (composite_reference.K), never over 16.  Second line of defence, on the well-conditioned rays only (kind
plain; 0.3 <= m <= 0.9), the ceilings the golden tests use, on the largest error over those rays / the tensor's largest entry:
2e-5 compositing outputs, d_raw, d_z_max; 5e-5 d_fg_z, d_norm; 2e-4 g_ray_o / g_ray_d; 2e-5 the intersection gradients.

Compositing rays (7, all in one call; ray_d ~ N(0, 1), not unit, so d|ray_d| is live):
  plain   sigma = 10 g on both networks           opaque  raw sigma from {-1, 0.5, 300, -3000}: T runs through the denormals
  tied    neighbouring depths equal, fg and bg            while the backward divides the suffix by q = 1e-6; abs and its sign
  empty   raw sigma exactly 0: alpha = 0, d sigma's sign term 0, bg_lambda = (1 + 1e-6)^sf
  thin    the last background sample's |sigma| ~ 1e-10: the gradient through the 1e10 interval is live (behind an optical
          depth of 24, so that this one entry, dalpha * 1e10 * e, is of the size of the tensor's other entries)
The translucent rays' depths are scaled per ray to a foreground optical depth of 1.5 (bg_lambda ~ 0.2), so that what reaches
the background through rgb is of one size on all of them and the 5-of-7 condition holds by construction.
Geometry rays (9): origin inside the unit sphere, built from the closest-approach distance m in GEO_M -- grazing (m -> 1:
sqrt(1 - m^2) and asin lose their digits) and near-centre (m -> 0: the backward forms g_m / m); |d| log-normal; inverse radii
in (0, 1).  m == 0 exactly, a ray through the centre, is OUT OF SCOPE: the reference divides by zero there as well.
Sampler rows (7): generic, spike (one non-zero weight: every sample of the ray in one bin, ns LDS atomics on one address),
zero (all weights 0: uniform through + 1e-6), steep (rand^8 * 1e3), u = linspace(0, 1, ns) (u == 1), steep and generic with
u == 0.  7 and 9 rays: the last workgroup of 4 waves has dead waves.

Worst ratio figure / max(E32, 2^-23) measured over these cases, interpreter | MI355X (the figure itself in brackets):
  compositing  rgb 1.00 | 1.05   fg_rgb 1.05 | 1.18   bg_rgb 1.00 | 1.12   fg_weights 1.13 | 0.87   bg_weights 0.66 | 0.72
               fg_depth 1.16 | 1.16   bg_depth 1.06 | 1.11   bg_lambda 1.00 | 1.00   (all <= 4.7e-6)
               d_raw_fg 1.18 | 1.18 (5.8e-7)   d_raw_bg 1.11 | 1.16 (1.5e-6)   d_fg_z 1.49 | 1.25 (5.2e-7, sf = 33)
               d_z_max 1.12 | 1.09 (3.5e-6)   d_norm 1.35 | 1.22 (3.2e-6)                    worst 1.49 -> K_COMPOSITE = 4
  geometry     far 1.00 | 1.00 (1.7e-5)   gi_o 1.01 | 1.01 (7.6e-6)   gi_d 1.17 | 1.17 (2.9e-6)   fg_pts 0.68 | 0.68
               viewdirs 0.55 | 0.55   bg_pts 3.35 | 3.35 (1.1e-6, also the sf = 0 launch)   bg_depth_real 1.33 | 1.38 (1.6e-7)
               g_ray_o 3.35 | 3.28 (2.3e-3: the m = 1e-3 ray, fp32 oracle 6.9e-4)   g_ray_d 3.44 | 3.34 (1.7e-5)
               g_fg_z 1.00 | 1.00                                                           worst 3.44 -> K_GEOMETRY = 8
  sampler bwd  g_bins 2.09 (m = 65, ns = 128; 2.9e-7) | 1.64 (m = 2, ns = 128; 1.2e-6)         worst 2.09 -> K_SAMPLER = 8
  sampler forward (cdf, below, above, t, samples) and jitter forward: bit for bit on both routes at every size;
  jitter backward <= 7.3e-8 on both.
"""
import numpy as np
import torch

from oracle import nerfpp_oracle as NO
from tests.composite_reference import assert_guards, metric

FLOOR = 2.0 ** -23
K_COMPOSITE = 4.0
K_GEOMETRY = 8.0
K_SAMPLER = 8.0
K = {"composite": K_COMPOSITE, "geometry": K_GEOMETRY, "sampler": K_SAMPLER}

KEYS = ("rgb", "fg_weights", "bg_weights", "fg_rgb", "fg_depth", "bg_rgb", "bg_depth", "bg_lambda")
COMP_BWD = ("d_raw_fg", "d_raw_bg", "d_fg_z", "d_z_max", "d_norm")
COMP_KINDS = ("plain", "opaque", "tied", "empty", "thin", "plain", "tied")
COMP_PLAIN = [r for r, k in enumerate(COMP_KINDS) if k == "plain"]
EMPTY_RAY = COMP_KINDS.index("empty")
COMP_SIZES = ((2, 2), (33, 65), (63, 64), (70, 40), (129, 63), (192, 192), (264, 200))
# (sf, sb, full): full = all eight upstream gradients, else g_rgb alone and the other seven NULL
COMP_CASES = [(sf, sb, full) for sf, sb in COMP_SIZES for full in (1, 0)]
KEEP_MIN = 5

GEO_M = (0.3, 0.5, 0.6, 0.8, 0.9, 0.99, 0.999, 1e-2, 1e-3)
GEO_WELL = [r for r, m in enumerate(GEO_M) if 0.3 <= m <= 0.9]
GEO_SIZES = ((1, 2), (70, 65), (192, 200))
GEO_NAMES = ("far", "gi_o", "gi_d", "fg_pts", "bg_pts", "viewdirs", "bg_depth_real", "g_ray_o", "g_ray_d", "g_fg_z")

SAMPLER_M = (1, 2, 17, 62, 63, 64, 65, 190, 513)
SAMPLER_NS = (1, 65, 128)
SAMPLER_CASES = [(m, ns) for m in SAMPLER_M for ns in SAMPLER_NS]
SAMPLER_ROWS = ("generic", "spike", "zero", "steep", "linspace", "steep_u0", "generic_u0")
JITTER_S = (1, 2, 65, 200)
N_RAYS = 7
INT_GUARD = -1                # below | above << 16 is never negative (m <= 32767)

WORST = {}                    # "family/tensor" -> (ratio, kernel figure, E32, case) of the worst ratio this session measured


def oracle_composite(raw_fg, raw_bg, fg_z, z_max, bg_z, rd):
    """the compositing half of NerfNet.forward on given raw outputs (raw_bg in flipped order)"""
    norm = torch.norm(rd, dim=-1, keepdim=True)
    rgb, sigma = torch.sigmoid(raw_fg[..., :3]), torch.abs(raw_fg[..., 3])
    dist = norm * torch.cat([fg_z[..., 1:] - fg_z[..., :-1], z_max[..., None] - fg_z[..., -1:]], -1)
    alpha = 1.0 - torch.exp(-sigma * dist)
    Tt = torch.cumprod(1.0 - alpha + NO.TINY, -1)
    lam = Tt[..., -1]
    Tt = torch.cat([torch.ones_like(Tt[..., :1]), Tt[..., :-1]], -1)
    fw = alpha * Tt
    f_rgb = (fw[..., None] * rgb).sum(-2)
    f_depth = (fw * fg_z).sum(-1)
    zf = torch.flip(bg_z, dims=[-1])
    rgb_b, sig_b = torch.sigmoid(raw_bg[..., :3]), torch.abs(raw_bg[..., 3])
    dist_b = torch.cat([zf[..., :-1] - zf[..., 1:], NO.HUGE * torch.ones_like(zf[..., :1])], -1)
    alpha_b = 1.0 - torch.exp(-sig_b * dist_b)
    Tb = torch.cumprod(1.0 - alpha_b + NO.TINY, -1)[..., :-1]
    Tb = torch.cat([torch.ones_like(Tb[..., :1]), Tb], -1)
    bw = alpha_b * Tb
    b_rgb = lam[..., None] * (bw[..., None] * rgb_b).sum(-2)
    b_depth = lam * (bw * zf).sum(-1)
    return {"rgb": f_rgb + b_rgb, "fg_weights": fw, "bg_weights": bw, "fg_rgb": f_rgb, "fg_depth": f_depth,
            "bg_rgb": b_rgb, "bg_depth": b_depth, "bg_lambda": lam}


# ---- metric and bound ------------------------------------------------------------------------------------------------
def per_ray(x, ref, keep_rule):
    """-> (worst per-ray figure over the kept rays, number of rays kept)"""
    n = ref.shape[0]
    x = np.asarray(x, np.float64).reshape(n, -1)
    ref = ref.reshape(n, -1)
    scale = np.abs(ref).max(1)
    keep = scale >= 1e-3 * scale.max() if keep_rule else np.ones(n, bool)
    assert not keep_rule or keep.sum() >= KEEP_MIN, "only %d of %d rays carry a comparable gradient" % (keep.sum(), n)
    return float((np.abs(x - ref).max(1)[keep] / (scale[keep] + 1e-300)).max()), int(keep.sum())


def rows_metric(x, ref, rows):
    """the golden tests' figure on the rows named: their largest error / the largest |fp64| entry of the whole tensor"""
    return float(np.abs(np.asarray(x, np.float64)[rows] - ref[rows]).max()) / (float(np.abs(ref).max()) + 1e-300)


def bound_check(family, case, got, o64, o32, names, per_ray_names=(), keep_names=()):
    """prints every figure, then asserts figure <= K[family] * max(E32, 2^-23) for every name; -> name -> ratio"""
    ratios, failed = {}, []
    for name in names:
        x = np.asarray(got[name])
        assert x.shape == o64[name].shape, (name, x.shape, o64[name].shape)
        if name in per_ray_names:
            (err, kept), (e32, _) = per_ray(x, o64[name], name in keep_names), per_ray(o32[name], o64[name], name in keep_names)
        else:
            err, e32, kept = metric(x, o64[name]), metric(o32[name], o64[name]), x.shape[0]
        ratio = err / max(e32, FLOOR)
        ratios[name] = ratio
        print("%s %s %-13s kernel %.3g  fp32 oracle %.3g  ratio %.3g  (%d rays)" % (family, case, name, err, e32, ratio, kept))
        key = family + "/" + name
        if ratio > WORST.get(key, (0.0,))[0]:
            WORST[key] = (ratio, err, e32, case)
        if not ratio <= K[family]:                 # (also catches NaN)
            failed.append((name, err, e32, ratio))
    assert not failed, (family, case, failed)
    return ratios


def assert_finite(tag, *oracles):
    for o in oracles:
        for k, v in o.items():
            assert np.isfinite(v).all(), "precondition: the oracle's %s is not finite on %s" % (k, tag)


def _np64(d):
    return {k: v.detach().double().numpy() for k, v in d.items()}


# ---- compositing -----------------------------------------------------------------------------------------------------
def composite_shapes(n, sf, sb):
    return {"rgb": (n, 3), "fg_weights": (n, sf), "bg_weights": (n, sb), "fg_rgb": (n, 3), "fg_depth": (n,),
            "bg_rgb": (n, 3), "bg_depth": (n,), "bg_lambda": (n,), "d_raw_fg": (n, sf, 4), "d_raw_bg": (n, sb, 4),
            "d_fg_z": (n, sf), "d_z_max": (n,), "d_norm": (n,)}


def composite_inputs(sf, sb):
    rng = np.random.default_rng(20000 + 1000 * sf + sb)
    n = N_RAYS
    raw_fg, raw_bg = rng.standard_normal((n, sf, 4)), rng.standard_normal((n, sb, 4))
    uf = np.sort(rng.random((n, sf)), -1)                       # foreground depths before the per-ray scale
    gap = 0.05 + 0.2 * rng.random(n)
    bg_z = np.sort(0.01 + 0.98 * rng.random((n, sb)), -1)       # inverse radii in (0, 1), ascending (the kernel flips)
    rd = rng.standard_normal((n, 3))
    span = np.ones(n)
    for r, kind in enumerate(COMP_KINDS):
        gf, gb = rng.standard_normal(sf), rng.standard_normal(sb)
        if kind == "opaque":
            raw_fg[r, :, 3] = rng.choice(np.array([-1.0, 0.5, 300.0, -3000.0]), size=sf)
            raw_bg[r, :, 3] = rng.choice(np.array([-1.0, 0.5, 300.0, -3000.0]), size=sb)
            continue
        if kind == "empty":
            raw_fg[r, :, 3] = 0.0
            raw_bg[r, :, 3] = 0.0
            continue
        raw_fg[r, :, 3], raw_bg[r, :, 3] = 10.0 * gf, 10.0 * gb
        if kind == "tied":
            uf[r, 1::2] = uf[r, 0:2 * (sf // 2):2]
            bg_z[r, 1::2] = bg_z[r, 0:2 * (sb // 2):2]
        if kind == "thin":                                      # raw_bg is in flipped order: its last row closes the ray
            # d sigma of that row is dalpha * 1e10 * e: with T ~ 1 in front of it, 1e10 times every other entry of the tensor,
            # and no other ray would count.  An optical depth of 24 in front (T = 4e-11) makes it an entry like the others.
            zf = bg_z[r, ::-1]
            raw_bg[r, :-1, 3] *= 24.0 / float((np.abs(raw_bg[r, :-1, 3]) * (zf[:-1] - zf[1:])).sum())
            # (each q is at least 1e-6: with a single sample in front, sb = 2, T stops at 1e-6 and |sigma| grows to 1e-9)
            T_last = float(np.prod(np.exp(-np.abs(raw_bg[r, :-1, 3]) * (zf[:-1] - zf[1:])) + 1e-6))
            raw_bg[r, -1, 3] = 1e-10 * max(0.5, np.log(T_last * 1e11)) * (1.0 if rng.random() < 0.5 else -1.0)
        delta = np.append(uf[r, 1:] - uf[r, :-1], gap[r])
        tau = float((np.abs(raw_fg[r, :, 3]) * delta).sum() * np.linalg.norm(rd[r]))
        span[r] = float(np.clip(1.5 / max(tau, 1e-30), 0.02, 8.0))
    fg_z = 0.05 + span[:, None] * uf
    z_max = fg_z[:, -1] + span * gap
    sh = composite_shapes(n, sf, sb)
    inp = dict(raw_fg=raw_fg, raw_bg=raw_bg, fg_z=fg_z, z_max=z_max, bg_z=bg_z, rd=rd)
    inp.update({"g_" + k: rng.standard_normal(sh[k]) for k in KEYS})
    return {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}


def composite_oracle(inp, full, dtype):
    cast = lambda k: torch.from_numpy(inp[k]).to(dtype)
    leaves = {k: cast(k).requires_grad_(True) for k in ("raw_fg", "raw_bg", "fg_z", "z_max", "rd")}
    ref = oracle_composite(leaves["raw_fg"], leaves["raw_bg"], leaves["fg_z"], leaves["z_max"], cast("bg_z"), leaves["rd"])
    sum((ref[k] * cast("g_" + k)).sum() for k in (KEYS if full else ("rgb",))).backward()
    out = dict(ref)
    out.update(d_raw_fg=leaves["raw_fg"].grad, d_raw_bg=leaves["raw_bg"].grad, d_fg_z=leaves["fg_z"].grad,
               d_z_max=leaves["z_max"].grad)
    rd = leaves["rd"]                                           # rd enters only through |rd|
    out["d_norm"] = (rd.grad * rd.detach()).sum(-1) / torch.norm(rd.detach(), dim=-1)
    return _np64(out)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def composite_references(case):
    """(inputs, fp64 oracle, fp32 oracle) of a case, computed once per session and shared; the inputs per size"""
    sf, sb, full = case

    def make():
        inp = _cached(("composite_inputs", sf, sb), lambda: composite_inputs(sf, sb))
        o64, o32 = composite_oracle(inp, full, torch.float64), composite_oracle(inp, full, torch.float32)
        assert_finite("composite %s" % (case,), o64, o32)
        return inp, o64, o32
    return _cached(("composite", case), make)


def run_composite(route, inp, full):
    """scnerf_npp_composite_fwd and _bwd into buffers with a NaN row before and after every output -> name -> array"""
    n, sf, sb = inp["fg_z"].shape[0], inp["fg_z"].shape[1], inp["bg_z"].shape[1]
    sh = composite_shapes(n, sf, sb)
    args = [route.inp(inp[k]) for k in ("raw_fg", "raw_bg", "fg_z", "z_max", "bg_z", "rd")]
    bufs = {k: route.out(sh[k]) for k in KEYS + COMP_BWD}
    route.call("scnerf_npp_composite_fwd", *args, *[bufs[k][1] for k in KEYS], n, sf, sb)
    gs = [route.inp(inp["g_" + k]) if (full or k == "rgb") else None for k in KEYS]
    route.call("scnerf_npp_composite_bwd", *args, *gs, *[bufs[k][1] for k in COMP_BWD], n, sf, sb)
    return collect(route, bufs)


def collect(route, bufs):
    got = {}
    for k, (buf, _) in bufs.items():
        b = route.host(buf)
        if b.dtype == np.int32:
            assert (b[0] == INT_GUARD).all() and (b[-1] == INT_GUARD).all(), k + ": written outside its rows"
            assert (b[1:-1] != INT_GUARD).all(), k + ": not written everywhere inside"
        else:
            assert_guards(b, k)
        got[k] = b[1:-1].copy()
    return got


def check_composite(case, got):
    sf, sb, full = case
    _, o64, o32 = composite_references(case)
    tag = "sf%d_sb%d_%s" % (sf, sb, "all" if full else "rgb")
    ratios = bound_check("composite", tag, got, o64, o32, KEYS + COMP_BWD, per_ray_names=COMP_BWD[:3], keep_names=COMP_BWD[:3])
    # the empty ray: alpha == 0 on both networks, no gradient through |sigma| at 0, lambda = (1 + 1e-6)^sf
    e = EMPTY_RAY
    assert not got["fg_weights"][e].any() and not got["bg_weights"][e].any()
    assert not got["d_raw_fg"][e, :, 3].any() and not got["d_raw_bg"][e, :, 3].any()
    lam = float(np.float32(1.0) + np.float32(1e-6)) ** sf
    assert abs(float(got["bg_lambda"][e]) - lam) <= 1.2e-7 * lam
    # ceilings, plain rays
    p = COMP_PLAIN
    # (d_z_max and d_norm with all eight gradients only, as in test_composite_fwd_bwd: through rgb alone d_norm is a sum that
    # cancels to a few 1e-2 and the fp32 oracle itself is 4e-5 from fp64 at sf = 264)
    tols = [(k, 2e-5) for k in KEYS + ("d_raw_fg", "d_raw_bg")] + [("d_fg_z", 5e-5)] + ([("d_z_max", 2e-5), ("d_norm", 5e-5)] if full else [])
    for name, tol in tols:
        assert rows_metric(got[name], o64[name], p) <= tol, name
    return ratios


# ---- geometry: intersect_sphere, foreground / background point placement -----------------------------------------------
def geometry_inputs(sf, sb):
    rng = np.random.default_rng(30000 + 1000 * sf + sb)
    n = len(GEO_M)
    m = np.array(GEO_M)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    v = np.cross(u, rng.standard_normal((n, 3)))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    along = rng.uniform(-0.9, 0.9, n) * np.sqrt(1.0 - m * m)          # the origin stays inside the sphere
    o = m[:, None] * v + along[:, None] * u
    d = np.exp(0.5 * rng.standard_normal(n))[:, None] * u
    inp = dict(ray_o=o, ray_d=d, fg_z=np.sort(rng.random((n, sf)), -1), bg_z=0.01 + 0.98 * rng.random((n, sb)),
               g_far=rng.standard_normal(n), g_fg=rng.standard_normal((n, sf, 3)), g_bg=rng.standard_normal((n, sb, 4)),
               g_vf=0.1 * rng.standard_normal((n, sf, 3)), g_vb=0.1 * rng.standard_normal((n, sb, 3)),
               g_norm=rng.standard_normal(n), g_zin=rng.standard_normal((n, sf)))
    return {k: np.ascontiguousarray(v_, np.float32) for k, v_ in inp.items()}


def geometry_oracle(inp, dtype):
    cast = lambda k: torch.from_numpy(inp[k]).to(dtype)
    n, sf, sb = inp["fg_z"].shape[0], inp["fg_z"].shape[1], inp["bg_z"].shape[1]
    o, d = cast("ray_o").requires_grad_(True), cast("ray_d").requires_grad_(True)
    far = NO.intersect_sphere(o, d)
    (far * cast("g_far")).sum().backward()
    out = dict(far=far, gi_o=o.grad, gi_d=d.grad)
    o, d, z = cast("ray_o").requires_grad_(True), cast("ray_d").requires_grad_(True), cast("fg_z").requires_grad_(True)
    pts_b, real = NO.depth2pts_outside(o[:, None].expand(n, sb, 3), d[:, None].expand(n, sb, 3), cast("bg_z"))
    pts_b, real = torch.flip(pts_b, dims=[-2]), torch.flip(real, dims=[-1])          # the kernel stores them far -> near
    pts_f = o[:, None] + z[..., None] * d[:, None]
    norm = torch.norm(d, dim=-1)
    view = d / norm[:, None]
    ((pts_f * cast("g_fg")).sum() + (pts_b[..., :3] * cast("g_bg")[..., :3]).sum() + (view[:, None] * cast("g_vf")).sum()
     + (view[:, None] * cast("g_vb")).sum() + (norm * cast("g_norm")).sum() + (z * cast("g_zin")).sum()).backward()
    out.update(fg_pts=pts_f, bg_pts=pts_b, viewdirs=view, bg_depth_real=real, g_ray_o=o.grad, g_ray_d=d.grad, g_fg_z=z.grad)
    return _np64(out)


def geometry_references(size):
    def make():
        inp = geometry_inputs(*size)
        o64, o32 = geometry_oracle(inp, torch.float64), geometry_oracle(inp, torch.float32)
        assert_finite("geometry %s" % (size,), o64, o32)
        return inp, o64, o32
    return _cached(("geometry", size), make)


def run_geometry(route, inp):
    n, sf, sb = inp["fg_z"].shape[0], inp["fg_z"].shape[1], inp["bg_z"].shape[1]
    I = route.inp
    o, d, fg_z, bg_z = I(inp["ray_o"]), I(inp["ray_d"]), I(inp["fg_z"]), I(inp["bg_z"])
    sh = dict(far=(n,), gi_o=(n, 3), gi_d=(n, 3), fg_pts=(n, sf, 3), bg_pts=(n, sb, 4), viewdirs=(n, 3),
              bg_depth_real=(n, sb), g_ray_o=(n, 3), g_ray_d=(n, 3), g_fg_z=(n, sf))
    bufs = {k: route.out(s) for k, s in sh.items()}
    flag = route.inp(np.zeros(1, np.int32))
    route.call("scnerf_npp_intersect_fwd", o, d, bufs["far"][1], flag, n)
    assert int(route.host(flag)[0]) == 0, "origins inside the unit sphere were flagged"
    route.call("scnerf_npp_intersect_bwd", o, d, I(inp["g_far"]), bufs["gi_o"][1], bufs["gi_d"][1], n)
    route.call("scnerf_npp_points_fwd", o, d, fg_z, bg_z, bufs["fg_pts"][1], bufs["bg_pts"][1], bufs["viewdirs"][1],
               bufs["bg_depth_real"][1], n, sf, sb)
    route.call("scnerf_npp_points_bwd", o, d, fg_z, bg_z, I(inp["g_fg"]), I(inp["g_bg"]), I(inp["g_vf"]), I(inp["g_vb"]),
               I(inp["g_norm"]), I(inp["g_zin"]), bufs["g_ray_o"][1], bufs["g_ray_d"][1], bufs["g_fg_z"][1], n, sf, sb)
    return collect(route, bufs)


def check_geometry(size, got):
    _, o64, o32 = geometry_references(size)
    ratios = bound_check("geometry", "sf%d_sb%d" % size, got, o64, o32, GEO_NAMES, per_ray_names=GEO_NAMES)
    w = GEO_WELL
    for name, tol in (("gi_o", 2e-5), ("gi_d", 2e-5), ("g_ray_o", 2e-4), ("g_ray_d", 2e-4)):
        assert rows_metric(got[name], o64[name], w) <= tol, name
    return ratios


def run_points_outside(route, inp):
    """the sf = 0, sb = 1 forward of depth2pts_outside: one row per (ray, inverse radius), no foreground, no view"""
    n, sb = inp["bg_z"].shape
    o = np.repeat(inp["ray_o"], sb, 0)
    d = np.repeat(inp["ray_d"], sb, 0)
    bufs = dict(pts=route.out((n * sb, 4)), real=route.out((n * sb, 1)))
    route.call("scnerf_npp_points_fwd", route.inp(o), route.inp(d), None, route.inp(inp["bg_z"].reshape(-1, 1)), None,
               bufs["pts"][1], None, bufs["real"][1], n * sb, 0, 1)
    return collect(route, bufs)


def check_points_outside(size, got):
    """the same values as the per-ray launch, row by row (the oracle's, unflipped), under the same bound"""
    inp, o64, o32 = geometry_references(size)
    n, sb = inp["bg_z"].shape
    pick = lambda o_: dict(pts=o_["bg_pts"][:, ::-1].reshape(n * sb, 4), real=o_["bg_depth_real"][:, ::-1].reshape(n * sb, 1))
    return bound_check("geometry", "outside_sb%d" % sb, got, pick(o64), pick(o32), ("pts", "real"), per_ray_names=("pts", "real"))


# ---- sampler ---------------------------------------------------------------------------------------------------------
def sampler_inputs(m, ns):
    rng = np.random.default_rng(40000 + 1000 * m + ns)
    n = N_RAYS
    bins = 0.5 + 4.0 * np.sort(rng.random((n, m + 1)), -1)
    w = rng.random((n, m))
    u = rng.random((n, ns))
    lin = torch.linspace(0.0, 1.0, ns).numpy()
    for r, kind in enumerate(SAMPLER_ROWS):
        if kind == "spike":
            w[r] = 0.0
            w[r, rng.integers(m)] = 1.0 + rng.random()
        elif kind == "zero":
            w[r] = 0.0
        elif kind.startswith("steep"):
            w[r] = rng.random(m) ** 8 * 1e3
        elif kind == "linspace":
            u[r] = lin
        if kind.endswith("_u0"):
            u[r, 0] = 0.0
    inp = dict(bins=bins, weights=w, u=u, g=rng.standard_normal((n, ns)))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in inp.items()}


def sampler_references(case):
    """(inputs, forward state of the fp32 oracle on the CPU, fp64 g_bins, sequential-fp32 g_bins)"""
    def make():
        m, ns = case
        inp = sampler_inputs(m, ns)
        T = lambda k: torch.from_numpy(inp[k])
        samples, cdf, below, above = NO.sample_pdf_state(T("bins"), T("weights"), T("u"))
        c0, c1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
        denom = c1 - c0
        denom = torch.where(denom < NO.TINY, torch.ones_like(denom), denom)
        fwd = dict(samples=samples.numpy(), cdf=cdf.numpy(), below=below.numpy(), above=above.numpy(),
                   t=((T("u") - c0) / denom).numpy())
        assert_finite("sampler %s" % (case,), fwd)
        rows = np.arange(inp["u"].shape[0])[:, None].repeat(ns, 1)
        g, t = inp["g"], fwd["t"]
        g64, g32 = np.zeros((rows.shape[0], m + 1)), np.zeros((rows.shape[0], m + 1), np.float32)
        np.add.at(g64, (rows, fwd["below"]), g.astype(np.float64) * (1.0 - t.astype(np.float64)))
        np.add.at(g64, (rows, fwd["above"]), g.astype(np.float64) * t.astype(np.float64))
        for j in range(ns):                                     # the kernel's lane order: sample by sample, below then above
            np.add.at(g32, (rows[:, j], fwd["below"][:, j]), g[:, j] * (np.float32(1.0) - t[:, j]))
            np.add.at(g32, (rows[:, j], fwd["above"][:, j]), g[:, j] * t[:, j])
        return inp, fwd, dict(g_bins=g64), dict(g_bins=g32.astype(np.float64))
    return _cached(("sampler", case), make)


def run_sampler(route, inp):
    n, m, ns = inp["weights"].shape[0], inp["weights"].shape[1], inp["u"].shape[1]
    bufs = dict(samples=route.out((n, ns)), ba=route.out((n, ns), np.int32), t=route.out((n, ns)), cdf=route.out((n, m + 1)),
                g_bins=route.out((n, m + 1)))
    route.call("scnerf_npp_sample_pdf", route.inp(inp["bins"]), route.inp(inp["weights"]), route.inp(inp["u"]),
               bufs["samples"][1], bufs["ba"][1], bufs["t"][1], bufs["cdf"][1], n, m, ns)
    route.call("scnerf_npp_sample_pdf_bwd", route.inp(inp["g"]), bufs["ba"][1], bufs["t"][1], bufs["g_bins"][1], n, m, ns)
    return collect(route, bufs)


def check_sampler(case, got):
    """forward bit for bit against the fp32 oracle; g_bins against the fp64 scatter-add under the bound"""
    _, fwd, g64, g32 = sampler_references(case)
    np.testing.assert_array_equal(got["cdf"], fwd["cdf"])
    np.testing.assert_array_equal(got["ba"] >> 16, fwd["above"])
    np.testing.assert_array_equal(got["ba"] & 0xffff, fwd["below"])
    np.testing.assert_array_equal(got["t"], fwd["t"])
    np.testing.assert_array_equal(got["samples"], fwd["samples"])
    return bound_check("sampler", "m%d_ns%d" % case, got, g64, g32, ("g_bins",), per_ray_names=("g_bins",))


# ---- jitter ----------------------------------------------------------------------------------------------------------
def jitter_references(s):
    def make():
        rng = np.random.default_rng(50000 + s)
        inp = dict(z=np.sort(rng.random((N_RAYS, s)), -1).astype(np.float32), t=rng.random((N_RAYS, s)).astype(np.float32),
                   g=rng.standard_normal((N_RAYS, s)).astype(np.float32))
        T = lambda k: torch.from_numpy(inp[k])
        z64 = T("z").double().requires_grad_(True)
        (NO.perturb_samples(z64, T("t").double()) * T("g").double()).sum().backward()
        ref = dict(out=NO.perturb_samples(T("z"), T("t")).numpy(), g_z=z64.grad.numpy())
        assert_finite("jitter %d" % s, ref)
        return inp, ref
    return _cached(("jitter", s), make)


def run_jitter(route, inp):
    n, s = inp["z"].shape
    bufs = dict(out=route.out((n, s)), g_z=route.out((n, s)))
    t = route.inp(inp["t"])
    route.call("scnerf_npp_perturb_fwd", route.inp(inp["z"]), t, bufs["out"][1], n, s)
    route.call("scnerf_npp_perturb_bwd", route.inp(inp["g"]), t, bufs["g_z"][1], n, s)
    return collect(route, bufs)


def check_jitter(s, got):
    _, ref = jitter_references(s)
    np.testing.assert_array_equal(got["out"], ref["out"])
    err = metric(got["g_z"], ref["g_z"])
    print("jitter s%d g_z kernel %.3g" % (s, err))
    assert err <= 2e-6
