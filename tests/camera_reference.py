"""TEST INFRASTRUCTURE: cases, fp64 references and error bounds of the stand-alone tests of the camera kernels
(csrc/camera_rays.hip, all 14 C entry points): tests/test_emu_camera_kernels.py on the CPU SIMT interpreter and
tests/test_gpu_camera_kernels.py on the GPU.  Both routes run the SAME launches (the run_* functions below, through a `route`
object that only knows how to hold a buffer and call the C ABI), see the same float32 inputs, references and bounds.

References: plain torch on float64 leaves, gradients by autograd -- oracle.scnerf_oracle's camera_intrinsic_params,
camera_extrinsics, camera_K, camera_E, upsample_noise_grid, ndc_rays, pinhole_rays; `ref_rays` is camera_rays of that module
extended by a single index, a shared matrix, per-ray matrices and the clamp of the noise pixel (asserted equal to it, bit for
bit, where both apply); `ref_npp_rays` restates render_ray_from_camera (nerfpp_oracle.camera_rays_pixel_centre keeps the pixel
centres in float32, which a float64 run would inherit; asserted equal to it in float32).  Yardstick E32: the same function on
float32 leaves.  Key points reach both as the same float32 values, so .long() truncates alike.

Metric: largest |x - fp64| over a tensor / largest |fp64| entry of that tensor; per ray (per camera for E and d_extr_noise,
whose rows differ by 1e6 in the conditioning cases) for the per-ray outputs, the worst row counts.  The sums taken by atomics
in no fixed order (d_intr_noise, the grid gradients, g_focal_xy, d_dist2) are measured over the whole tensor against the fp32
oracle's own sum; no margin for the order of summation was needed.
Bound: figure <= K * max(E32, 2^-23), K per family the smallest power of two >= twice the worst ratio measured on either
route, never under 4, never over 16.  Second line of defence on the well-conditioned default cases: the golden tests' ceilings
(rtol 1e-5 / atol 1e-6 on rays, 2e-5 / 2e-6 on NDC).
Exact statements: guard rows untouched (one NaN row before and after every output); d_extr_noise rows of unused cameras,
grid-gradient cells no ray's taps touch, d_extrinsic row 3: exactly 0; per-ray outputs bit for bit between two launches.

Worst ratio figure / max(E32, 2^-23) measured over these cases, interpreter | MI355X (the fp32 oracle runs on the host of either
route, so its own sums differ between the two columns; the per-ray figures of the NDC warp are the same arithmetic):
  rays      rays_o 1.00 | 1.00   rays_d 1.20 | 1.38   d_intr_noise 2.04 | 2.14   d_extr_noise 2.93 | 2.88
  (+ NeRF++,  d_grid_o 2.90 | 1.99   d_grid_d 2.43 | 1.36   d_extrinsic 1.57 | 1.57   d_dist2 3.10 | 2.18
   pinhole)                                                                          worst 3.10 -> K["rays"] = 8
  matrices  K 0.41 | 0.41   E 1.00 | 1.37   d_intr_noise 0.48 | 0.48   d_extr_noise 2.19 | 3.17 (C = 130)
                                                                                     worst 3.17 -> K["matrices"] = 8
  NDC/pack  ndc_o 1.00 | 1.00   ndc_d 1.00 | 1.00   pack_o 1.00 | 1.00   pack_d 1.00 | 1.00   pack_v 1.00 | 1.00
            g_rays_d 2.94 | 2.94   g_focal_xy 1.57 | 1.57
            g_rays_o 6.08 | 6.08 (1.7e-6, n = 63, ray 11: a |d_z| = 1e-2 |d| ray, whose g_o_z = g_oz - g_t / d_z is the
            difference of two terms 100 times its size; the fp32 oracle's worst ray at n = 257 is that kind too, at 9.0e-7)
                                                                                     worst 6.08 -> K["ndc"] = 16
  upsample  out 1.10 | 1.10   d_grid 1.24 | 1.02                                     worst 1.24 -> K["upsample"] = 4
Mutations of camera_rays.hip that the interpreter route catches (tests failing of 95): a sign of one cross term in
gram_schmidt_bwd 53, `t.x0 <= gw - 1` in bilinear_taps 46, no flush of the LDS pre-reduction 48, +1.f in the gk[2] term 38.
"""
import numpy as np
import torch

from oracle import scnerf_oracle as O
from tests.composite_reference import metric
from tests.nerfpp_reference import FLOOR, assert_finite, collect, per_ray

K = {"rays": 8.0, "matrices": 8.0, "ndc": 16.0, "upsample": 4.0}
WORST = {}                    # "family/tensor" -> (ratio, kernel figure, E32, case) of the worst ratio this session measured

SHAPES = ((37, 50, 378, 504), (1, 1, 7, 5), (6, 8, 6, 8), (3, 4, 20, 30), (12, 16, 6, 8))      # gh, gw, H, W
RAY_COUNTS = (1, 63, 64, 65, 257, 1000)
INTR_SCALE = {0: 0.7, 1: 0.013}          # additive (pixels per unit of noise) | multiplicative
EXTR_SCALE, SCALE_O, SCALE_D = 0.3, 0.05, 0.08
GS_ANGLES, GS_NORMS = (90.0, 10.0, 0.5), (1e-3, 1.0, 1e3)
NDC_HW, NDC_F2, NDC_NEAR = (48, 64), (55.0, 57.5), 1.0
PACK_NEAR_FAR = (0.25, 3.0)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_id(case):
    return "-".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in case.items()
                    if k != "seed")


def _key(case):
    return tuple(sorted(case.items()))


def _f32(d):
    return {k: (np.ascontiguousarray(v, np.float32) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v)
            for k, v in d.items()}


def _np64(d):
    return {k: v.detach().double().numpy() for k, v in d.items()}


def _grad(leaf):
    return torch.zeros_like(leaf) if leaf.grad is None else leaf.grad


# ---- metric and bound ------------------------------------------------------------------------------------------------
def bound_check(family, tag, got, o64, o32, names, per_ray_names=()):
    """prints every figure, then asserts figure <= K[family] * max(E32, 2^-23) for every name; -> name -> ratio"""
    ratios, failed = {}, []
    for name in names:
        x = np.asarray(got[name])
        assert x.shape == o64[name].shape, (name, x.shape, o64[name].shape)
        if name in per_ray_names and x.ndim >= 2:
            err, e32 = per_ray(x, o64[name], False)[0], per_ray(o32[name], o64[name], False)[0]
        else:
            err, e32 = metric(x, o64[name]), metric(o32[name], o64[name])
        ratio = err / max(e32, FLOOR)
        ratios[name] = ratio
        print("%s %s %-13s kernel %.3g  fp32 oracle %.3g  ratio %.3g" % (family, tag, name, err, e32, ratio))
        key = family + "/" + name
        if ratio > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (ratio, err, e32, tag)
        if not ratio <= K[family]:                 # (also catches NaN)
            failed.append((name, err, e32, ratio))
    assert not failed, (family, tag, failed)
    return ratios


def report():
    print()
    for key in sorted(WORST):
        print("WORST %-26s ratio %.3g  (kernel %.3g, fp32 oracle %.3g, %s)" % ((key,) + WORST[key]))


def same_bits(a, b, names):
    for name in names:
        if name in a:
            np.testing.assert_array_equal(np.ascontiguousarray(a[name]).view(np.int32),
                                          np.ascontiguousarray(b[name]).view(np.int32), err_msg=name)


# ---- camera parameters -----------------------------------------------------------------------------------------------------
def gs_poses(rng):
    """[9, 6]: a1, a2 at the angles GS_ANGLES with |a1| in GS_NORMS (|a2| = 0.5 .. 1.5 |a1|)"""
    rows = []
    for ang in GS_ANGLES:
        for s in GS_NORMS:
            u = rng.standard_normal(3)
            u /= np.linalg.norm(u)
            w = np.cross(u, rng.standard_normal(3))
            w /= np.linalg.norm(w)
            a = np.deg2rad(ang)
            rows.append(np.concatenate([s * u, s * (0.5 + rng.random()) * (np.cos(a) * u + np.sin(a) * w)]))
    return np.array(rows)


def camera_params(rng, C, H, W, mult, gs=False, centre_on_pixel=False):
    """the learnable camera's tensors.  `gs`: the nine Gram-Schmidt conditioning poses first, their rotation residual a
    relative 1e-4 (a residual of the usual size would BE the pose at |a1| = 1e-3).  `centre_on_pixel`: the principal point
    1e-3 .. 1e-2 of a pixel from the centre of pixel (W // 2, H // 2) (the NeRF++ distortion at ux ~ 0)"""
    intr_init = np.array([1.2 * W, 1.25 * W, 0.5 * W + 0.3, 0.5 * H - 0.2])
    intr_noise = rng.standard_normal(4) * (1.0 if mult else 3.0)
    if centre_on_pixel:
        intr_init[2:] = (W // 2 + 0.5, H // 2 + 0.5)
        intr_noise[2:] = np.array([4e-3, -9e-3]) / (INTR_SCALE[mult] * (intr_init[2:] if mult else 1.0))
    extr_init = np.concatenate([rng.standard_normal((C, 6)), 0.5 * rng.standard_normal((C, 3))], -1)
    extr_noise = 0.05 * rng.standard_normal((C, 9))
    if gs:
        g = gs_poses(rng)
        m = min(C, len(g))
        extr_init[:m, :6] = g[:m]
        extr_noise[:m, :6] = 1e-4 / EXTR_SCALE * g[:m] * rng.standard_normal((m, 6))
    return dict(intr_init=intr_init, intr_noise=intr_noise, extr_init=extr_init, extr_noise=extr_noise)


def oracle_cam(inp, mult, dtype, grids=()):
    """the oracle's camera dictionary on leaves of `dtype` -> (cam, leaves)"""
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    leaves = {k: T(k).requires_grad_(True) for k in ("intr_noise", "extr_noise") + tuple(grids)}
    cam = {"intrinsics_initial": T("intr_init"), "extrinsics_initial": T("extr_init"),
           "intrinsics_noise": leaves["intr_noise"], "extrinsics_noise": leaves["extr_noise"],
           "intrinsics_noise_scale": INTR_SCALE[mult], "extrinsics_noise_scale": EXTR_SCALE,
           "ray_o_noise_scale": SCALE_O, "ray_d_noise_scale": SCALE_D, "multiplicative_noise": bool(mult)}
    return cam, leaves


def _cam_args(route, inp, mult, C):
    I = route.inp
    return (I(inp["intr_init"]), I(inp["intr_noise"]), INTR_SCALE[mult], mult, I(inp["extr_init"]), I(inp["extr_noise"]),
            EXTR_SCALE, C)


def workspace(route, slots):
    """scnerf_camera_bwd_workspace_floats(slots) floats of NaN: the entry point clears what it accumulates into"""
    return route.inp(np.full(4 + 12 * max(1, slots), np.nan, np.float32))


# ---- key points ----------------------------------------------------------------------------------------------------------
def make_kps(rng, kind, n, H, W):
    rand = np.stack([rng.random(n) * (W - 1), rng.random(n) * (H - 1)], -1)          # fractional, inside
    fx_, fy_ = rng.random() * (W - 1), rng.random() * (H - 1)
    xb = min(12, max(W - 2, 0)) + 0.999999                                          # just below an integer
    edges = [(0, 0), (W - 1, H - 1), (W - 1, fy_), (fx_, H - 1), (W - 1, 0), (0, H - 1), (xb, min(1.0, H - 1)),
             (W // 2, H // 2), (W - 1 + 0.25, H - 1 + 0.75), (min(3, W - 1), min(2, H - 1))]
    if kind == "interior":
        return rand
    if kind == "integer":
        return np.floor(rand)
    if kind == "mixed":                       # the edge points, then interior ones
        return np.concatenate([np.array(edges, np.float64), rand])[:n]
    if kind == "edges":
        pool = edges
    elif kind == "lastrowcol":
        pool = [(W - 1, fy_), (fx_, H - 1), (W - 1, H - 1), (W - 1 + 0.5, fy_), (np.floor(fx_), H - 1 + 0.5)]
    elif kind == "outside":                   # direction from the coordinate itself, noise from the clamped pixel
        xs, ys = (-3.5, W + 9.25), (-2.25, H + 4.5)
        pool = [(xs[0], fy_), (xs[1], fy_), (fx_, ys[0]), (fx_, ys[1]), (xs[0], ys[0]), (xs[1], ys[1]), (xs[0], ys[1]),
                (xs[1], ys[0]), (fx_, fy_)]
    else:
        raise ValueError(kind)
    return np.array([pool[i % len(pool)] for i in range(n)], np.float64)


def taps_touched(px, py, gh, gw, H, W):
    """bool [gh, gw]: the cells any of the four taps of upsample_bilinear2d (align_corners=False) at the pixels (py, px)
    can reach -- the union of the float64 and the float32 source index, which may truncate apart at an integer"""
    hit = np.zeros((gh, gw), bool)
    for ft in (np.float64, np.float32):
        fy = np.maximum(ft(gh) / ft(H) * (py.astype(ft) + ft(0.5)) - ft(0.5), 0)
        fx = np.maximum(ft(gw) / ft(W) * (px.astype(ft) + ft(0.5)) - ft(0.5), 0)
        y0, x0 = np.minimum(fy.astype(np.int64), gh - 1), np.minimum(fx.astype(np.int64), gw - 1)
        y1, x1 = np.minimum(y0 + 1, gh - 1), np.minimum(x0 + 1, gw - 1)
        for yy in (y0, y1):
            for xx in (x0, x1):
                hit[yy, xx] = True
    return hit


# ---- camera rays: scnerf_camera_rays_fwd / _bwd ------------------------------------------------------------------------------
def rays_case(n=65, pose="idx", C=5, shape=SHAPES[0], grids="both", mult=0, kps="mixed", up="both", gs=0):
    """pose: idx (per-ray camera index) | sparse (idx, cameras 0, C - 1, C - 2 and three more only) | single | shared |
    perray;  grids: both | o | d | none | aliased;  up: both | o (g_d NULL) | d (g_o NULL)"""
    return dict(n=n, pose=pose, C=C, shape=shape, grids=grids, mult=mult, kps=kps, up=up, gs=gs)


DEFAULT_RAYS = rays_case(n=64, kps="interior")
RAYS_CASES = (
    [rays_case(n=n) for n in RAY_COUNTS if n != 65] + [DEFAULT_RAYS]
    + [rays_case(pose=p) for p in ("idx", "single", "shared", "perray")]
    + [rays_case(n=257, pose="sparse", C=C) for C in (1024, 1025)]
    + [rays_case(n=64, kps=k) for k in ("integer", "edges", "lastrowcol", "outside")]
    + [rays_case(shape=s, kps=k) for s in SHAPES[1:] for k in ("mixed", "outside")]
    + [rays_case(shape=s, grids=g) for s in (SHAPES[0], SHAPES[3]) for g in ("o", "d", "none", "aliased")]
    + [rays_case(mult=1), rays_case(mult=1, pose="shared", grids="aliased")]
    + [rays_case(n=257, C=9, gs=1), rays_case(n=63, C=9, gs=1, pose="single", mult=1)]
    + [rays_case(up=u, pose=p) for u in ("o", "d") for p in ("idx", "perray")])
RAYS_PER_RAY = ("rays_o", "rays_d", "d_extr_noise")


def _has(case, which):
    return case["grids"] in {"o": ("both", "o", "aliased"), "d": ("both", "d", "aliased")}[which]


def rays_inputs(case):
    n, C, (gh, gw, H, W) = case["n"], case["C"], case["shape"]
    rng = np.random.default_rng(1000 + sum(map(ord, case_id(case))))
    inp = camera_params(rng, C, H, W, case["mult"], gs=bool(case["gs"]))
    inp.update(kps=make_kps(rng, case["kps"], n, H, W), grid_o=rng.standard_normal((gh, gw, 3)),
               grid_d=rng.standard_normal((gh, gw, 3)), g_o=rng.standard_normal((n, 3)), g_d=rng.standard_normal((n, 3)))
    if case["pose"] == "sparse":
        used = np.array([0, C - 1, C - 2, 5, 511, 777])
        idx = used[rng.integers(0, len(used), n)]
        idx[:3] = used[:3]
    else:
        idx = rng.integers(0, C, n)
    inp["idx"] = idx.astype(np.int64)
    inp["single"] = C - 2 if C > 1 else 0
    if case["pose"] in ("shared", "perray"):                # poses near rotations, not orthonormal: every entry is live
        m = 1 if case["pose"] == "shared" else n
        E = np.zeros((m, 4, 4))
        E[:, :3, :3] = np.linalg.qr(rng.standard_normal((m, 3, 3)))[0] + 0.05 * rng.standard_normal((m, 3, 3))
        E[:, :3, 3] = 0.5 * rng.standard_normal((m, 3))
        E[:, 3, 3] = 1.0
        inp["E"] = E
    return _f32(inp)


def ref_rays(cam, H, W, kps, idx=None, E=None):
    """oracle.scnerf_oracle.camera_rays (get_rays_kps_use_camera) with `idx` a tensor or an int, or the pose(s) E [4,4] /
    [N,4,4] given; the pixel the noise is read at is clamped into the image as the kernel's is"""
    fx, fy, cx, cy = O.camera_intrinsic_params(cam)
    Km = torch.eye(3, dtype=fx.dtype)
    Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2] = fx, fy, cx, cy
    Kinv = torch.inverse(Km)
    hom = torch.stack([kps[:, 0], kps[:, 1], torch.ones_like(kps[:, 0])], dim=-1)
    dirs = hom @ Kinv.T
    dirs = torch.cat([dirs[:, :1], -dirs[:, 1:3]], dim=-1)
    n = kps.shape[0]
    if E is None:
        R, t = O.camera_extrinsics(cam)
        if not torch.is_tensor(idx):
            idx = torch.full((n,), int(idx), dtype=torch.long)
        Rn, tn = R[idx], t[idx]
    elif E.dim() == 2:
        Rn, tn = E[None, :3, :3].expand(n, 3, 3), E[None, :3, 3].expand(n, 3)
    else:
        Rn, tn = E[:, :3, :3], E[:, :3, 3]
    rays_d = torch.sum(dirs[:, None, :] * Rn, dim=-1)
    rays_o = tn
    px = kps.long()
    lin = px[:, 1].clamp(0, H - 1) * W + px[:, 0].clamp(0, W - 1)
    if "ray_o_noise" in cam:
        rays_o = rays_o + O.upsample_noise_grid(cam["ray_o_noise"], H, W, cam["ray_o_noise_scale"])[lin]
    if "ray_d_noise" in cam:
        rays_d = rays_d + O.upsample_noise_grid(cam["ray_d_noise"], H, W, cam["ray_d_noise_scale"])[lin]
        rays_d = rays_d / (rays_d.norm(dim=1)[:, None] + 1e-10)
    return rays_o, rays_d


def _pose_leaves(inp, case, cam, leaves, dtype):
    """-> keyword arguments of ref_rays / ref_npp_rays for the case's pose source"""
    pose = case["pose"]
    if pose in ("idx", "sparse"):
        return dict(idx=torch.from_numpy(inp["idx"]))
    if pose == "single":
        return dict(idx=int(inp["single"]))
    E = torch.from_numpy(inp["E"]).to(dtype)
    leaves["E"] = (E[0] if pose == "shared" else E).clone().requires_grad_(True)
    return dict(E=leaves["E"])


def rays_oracle(inp, case, dtype):
    gh, gw, H, W = case["shape"]
    grids = ("grid_o",) * _has(case, "o") + ("grid_d",) * (_has(case, "d") and case["grids"] != "aliased")
    cam, leaves = oracle_cam(inp, case["mult"], dtype, grids)
    if _has(case, "o"):
        cam["ray_o_noise"] = leaves["grid_o"]
    if _has(case, "d"):
        cam["ray_d_noise"] = leaves["grid_o" if case["grids"] == "aliased" else "grid_d"]      # one leaf read twice
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    ro, rd = ref_rays(cam, H, W, T("kps"), **_pose_leaves(inp, case, cam, leaves, dtype))
    loss = 0.0
    if case["up"] in ("both", "o"):
        loss = loss + (ro * T("g_o")).sum()
    if case["up"] in ("both", "d"):
        loss = loss + (rd * T("g_d")).sum()
    if loss.requires_grad:
        loss.backward()
    out = dict(rays_o=ro, rays_d=rd, d_intr_noise=_grad(leaves["intr_noise"]))
    if case["pose"] != "perray":
        out["d_extr_noise"] = _grad(leaves["extr_noise"])
    for k in grids:
        out["d_" + k] = _grad(leaves[k])
    if "E" in leaves:
        out["d_extrinsic"] = _grad(leaves["E"]).reshape(-1, 4, 4)
    return _np64(out)


def _references(kind, case, inputs, oracle):
    def make():
        inp = inputs(case)
        o64, o32 = oracle(inp, case, torch.float64), oracle(inp, case, torch.float32)
        assert_finite("%s %s" % (kind, case_id(case)), o64, o32)
        return inp, o64, o32
    return _cached((kind, _key(case)), make)


def rays_references(case):
    return _references("rays", case, rays_inputs, rays_oracle)


def _pose_args(route, inp, case):
    """-> (cam_idx, single_idx, extrinsic, n_ext)"""
    pose, n = case["pose"], case["n"]
    if pose in ("idx", "sparse"):
        return route.inp(inp["idx"]), 0, None, 0
    if pose == "single":
        return None, int(inp["single"]), None, 0
    return None, 0, route.inp(inp["E"]), 1 if pose == "shared" else n


def run_rays(route, inp, case):
    """scnerf_camera_rays_fwd and _bwd into NaN buffers with a guard row on each side -> name -> array"""
    n, C, (gh, gw, H, W) = case["n"], case["C"], case["shape"]
    I = route.inp
    idx, single, ext, n_ext = _pose_args(route, inp, case)
    grid_o = I(inp["grid_o"]) if _has(case, "o") else None
    grid_d = None if not _has(case, "d") else grid_o if case["grids"] == "aliased" else I(inp["grid_d"])
    common = (I(inp["kps"]), idx, single, ext, n_ext) + _cam_args(route, inp, case["mult"], C) + (
        grid_o, SCALE_O, grid_d, SCALE_D, gh, gw, H, W)
    bufs = dict(rays_o=route.out((n, 3)), rays_d=route.out((n, 3)))
    route.call("scnerf_camera_rays_fwd", *common, bufs["rays_o"][1], bufs["rays_d"][1], n)
    bufs["d_intr_noise"] = route.out((4,))
    if case["pose"] != "perray":
        bufs["d_extr_noise"] = route.out((C, 9))
    if grid_o is not None:
        bufs["d_grid_o"] = route.out((gh, gw, 3))
    if grid_d is not None and case["grids"] != "aliased":
        bufs["d_grid_d"] = route.out((gh, gw, 3))
    if ext is not None:
        bufs["d_extrinsic"] = route.out((n_ext, 4, 4))
    view = lambda k: bufs[k][1] if k in bufs else None
    route.call("scnerf_camera_rays_bwd", *common, I(inp["g_o"]) if case["up"] in ("both", "o") else None,
               I(inp["g_d"]) if case["up"] in ("both", "d") else None, view("d_intr_noise"), view("d_extr_noise"),
               view("d_grid_o"), view("d_grid_o") if case["grids"] == "aliased" else view("d_grid_d"), view("d_extrinsic"),
               workspace(route, n_ext if ext is not None else C), n)
    return collect(route, bufs)


def check_exact_rays(case, inp, got, px, py):
    """the statements that hold exactly: unused cameras, untouched grid cells, the matrix gradient's last row"""
    gh, gw, H, W = case["shape"]
    if "d_extr_noise" in got:
        used = np.zeros(case["C"], bool)
        if case["pose"] in ("idx", "sparse"):
            used[inp["idx"]] = True
        elif case["pose"] == "single":
            used[inp["single"]] = True
        assert not got["d_extr_noise"][~used].any(), "d_extr_noise of a camera no ray uses"
        assert case["n"] == 0 or case["pose"] == "shared" or got["d_extr_noise"][used].any()
    hit = taps_touched(np.clip(px, 0, W - 1), np.clip(py, 0, H - 1), gh, gw, H, W)
    for k in ("d_grid_o", "d_grid_d"):
        if k in got:
            assert not got[k][~hit].any(), k + ": a cell no ray's taps touch"
    if "d_extrinsic" in got:
        assert not got["d_extrinsic"][:, 3].any(), "d_extrinsic row 3"


def check_rays(case, got):
    inp, o64, o32 = rays_references(case)
    ratios = bound_check("rays", case_id(case), got, o64, o32, tuple(o64), RAYS_PER_RAY + (
        ("d_extrinsic",) if case["pose"] == "perray" else ()))
    trunc = inp["kps"].astype(np.int64)
    check_exact_rays(case, inp, got, trunc[:, 0], trunc[:, 1])
    if case == DEFAULT_RAYS:                                   # the golden tests' ceilings
        np.testing.assert_allclose(got["rays_o"], o64["rays_o"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got["rays_d"], o64["rays_d"], rtol=1e-5, atol=1e-6)
    return ratios


# ---- NeRF++ generator: scnerf_npp_camera_rays_fwd / _bwd -----------------------------------------------------------------------
def npp_case(n=65, pose="single", dist=(0.05, -0.01), shape=SHAPES[0], mult=0, grids="both"):
    return dict(n=n, pose=pose, dist=dist, shape=shape, mult=mult, grids=grids, C=5, up="both")


NPP_CASES = ([npp_case(n=n) for n in RAY_COUNTS] + [npp_case(dist=d) for d in (None, (0.0, 0.0))]
             + [npp_case(pose="shared", dist=d, mult=1) for d in (None, (0.05, -0.01))]
             + [npp_case(shape=SHAPES[3], grids=g) for g in ("aliased", "none")])


def npp_inputs(case):
    n, C, (gh, gw, H, W) = case["n"], case["C"], case["shape"]
    rng = np.random.default_rng(2000 + sum(map(ord, case_id(case))))
    inp = camera_params(rng, C, H, W, case["mult"], centre_on_pixel=True)
    centre = (H // 2) * W + W // 2                              # the pixel whose centre is nearest the principal point
    select = np.concatenate([[centre, 0, H * W - 1], rng.integers(0, H * W, n)])[:n]
    inp.update(select=select.astype(np.int64), grid_o=rng.standard_normal((gh, gw, 3)), grid_d=rng.standard_normal((gh, gw, 3)),
               g_o=rng.standard_normal((n, 3)), g_d=rng.standard_normal((n, 3)), single=C - 2)
    if case["dist"] is not None:
        inp["dist"] = np.array(case["dist"], np.float64)
    if case["pose"] == "shared":
        E = np.eye(4)
        E[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0] + 0.05 * rng.standard_normal((3, 3))
        E[:3, 3] = 0.5 * rng.standard_normal(3)
        inp["E"] = E[None]
    return _f32(inp)


def ref_npp_rays(cam, H, W, select, dist=None, idx=None, E=None):
    """render_ray_from_camera (see oracle.nerfpp_oracle.camera_rays_pixel_centre) on the learnable camera, in the dtype of
    `cam`: pixel centres, optional radial distortion, K^-1 written out, no axis flips, noise at the selected pixels,
    renormalisation without an epsilon"""
    fx, fy, cx, cy = O.camera_intrinsic_params(cam)
    u = (select % W).to(fx.dtype) + 0.5
    v = torch.div(select, W, rounding_mode="floor").to(fx.dtype) + 0.5
    if dist is not None:
        ru, rv = (u - cx) / cx, (v - cy) / cy
        u = (u - cx) * (1 + ru ** 2 * dist[0] + ru ** 4 * dist[1]) + cx
        v = (v - cy) * (1 + rv ** 2 * dist[0] + rv ** 4 * dist[1]) + cy
    dirs = torch.stack([u * (1.0 / fx) + (-cx / fx), v * (1.0 / fy) + (-cy / fy), torch.ones_like(u)], 0)
    c2w = O.camera_E(cam)[idx] if E is None else E
    rays_d = (c2w[:3, :3] @ dirs).t()
    rays_o = c2w[:3, 3][None].expand(select.shape[0], 3)
    if "ray_o_noise" in cam:
        rays_o = rays_o + O.upsample_noise_grid(cam["ray_o_noise"], H, W, cam["ray_o_noise_scale"])[select]
    if "ray_d_noise" in cam:
        rays_d = rays_d + O.upsample_noise_grid(cam["ray_d_noise"], H, W, cam["ray_d_noise_scale"])[select]
        rays_d = rays_d / rays_d.norm(dim=1, keepdim=True)
    return rays_o, rays_d


def npp_oracle(inp, case, dtype):
    gh, gw, H, W = case["shape"]
    grids = ("grid_o",) * _has(case, "o") + ("grid_d",) * (_has(case, "d") and case["grids"] != "aliased")
    cam, leaves = oracle_cam(inp, case["mult"], dtype, grids)
    if _has(case, "o"):
        cam["ray_o_noise"] = leaves["grid_o"]
    if _has(case, "d"):
        cam["ray_d_noise"] = leaves["grid_o" if case["grids"] == "aliased" else "grid_d"]
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    if "dist" in inp:
        leaves["dist"] = T("dist").requires_grad_(True)
    ro, rd = ref_npp_rays(cam, H, W, torch.from_numpy(inp["select"]), leaves.get("dist"),
                          **_pose_leaves(inp, case, cam, leaves, dtype))
    ((ro * T("g_o")).sum() + (rd * T("g_d")).sum()).backward()
    out = dict(rays_o=ro, rays_d=rd, d_intr_noise=_grad(leaves["intr_noise"]), d_extr_noise=_grad(leaves["extr_noise"]))
    for k in grids:
        out["d_" + k] = _grad(leaves[k])
    if "E" in leaves:
        out["d_extrinsic"] = _grad(leaves["E"]).reshape(-1, 4, 4)
    if "dist" in leaves:
        out["d_dist2"] = _grad(leaves["dist"])
    return _np64(out)


def npp_references(case):
    return _references("npp", case, npp_inputs, npp_oracle)


def run_npp(route, inp, case):
    n, C, (gh, gw, H, W) = case["n"], case["C"], case["shape"]
    I = route.inp
    ext = I(inp["E"]) if case["pose"] == "shared" else None
    grid_o = I(inp["grid_o"]) if _has(case, "o") else None
    grid_d = None if not _has(case, "d") else grid_o if case["grids"] == "aliased" else I(inp["grid_d"])
    common = (I(inp["select"]), I(inp["dist"]) if "dist" in inp else None, int(inp["single"]), ext) + _cam_args(
        route, inp, case["mult"], C) + (grid_o, SCALE_O, grid_d, SCALE_D, gh, gw, H, W)
    bufs = dict(rays_o=route.out((n, 3)), rays_d=route.out((n, 3)))
    route.call("scnerf_npp_camera_rays_fwd", *common, bufs["rays_o"][1], bufs["rays_d"][1], n)
    bufs.update(d_intr_noise=route.out((4,)), d_extr_noise=route.out((C, 9)))
    if grid_o is not None:
        bufs["d_grid_o"] = route.out((gh, gw, 3))
    if grid_d is not None and case["grids"] != "aliased":
        bufs["d_grid_d"] = route.out((gh, gw, 3))
    if ext is not None:
        bufs["d_extrinsic"] = route.out((1, 4, 4))
    if "dist" in inp:
        bufs["d_dist2"] = route.out((2,))
    view = lambda k: bufs[k][1] if k in bufs else None
    route.call("scnerf_npp_camera_rays_bwd", *common, I(inp["g_o"]), I(inp["g_d"]), view("d_intr_noise"), view("d_extr_noise"),
               view("d_grid_o"), view("d_grid_o") if case["grids"] == "aliased" else view("d_grid_d"), view("d_extrinsic"),
               view("d_dist2"), workspace(route, 1 if ext is not None else C), n)
    return collect(route, bufs)


def check_npp(case, got):
    inp, o64, o32 = npp_references(case)
    ratios = bound_check("rays", "npp-" + case_id(case), got, o64, o32, tuple(o64), RAYS_PER_RAY)
    W = case["shape"][3]
    check_exact_rays(case, inp, got, inp["select"] % W, inp["select"] // W)
    return ratios


# ---- K and E: scnerf_camera_matrices_fwd / _bwd --------------------------------------------------------------------------------
def matrices_case(C=9, mult=0, gs=1, null=None):
    """null: g_K | g_E | d_intr_noise | d_extr_noise passed as NULL"""
    return dict(C=C, mult=mult, gs=gs, null=null)


MATRICES_CASES = ([matrices_case(C=C, gs=0, mult=C % 2) for C in (1, 63, 64, 130)] + [matrices_case(), matrices_case(mult=1)]
                  + [matrices_case(null=k) for k in ("g_K", "g_E", "d_intr_noise", "d_extr_noise")]
                  + [matrices_case(C=1, gs=0, null="g_K")])


def matrices_inputs(case):
    C = case["C"]
    rng = np.random.default_rng(3000 + sum(map(ord, case_id(case))))
    inp = camera_params(rng, C, 378, 504, case["mult"], gs=bool(case["gs"]))
    inp.update(g_K=rng.standard_normal((4, 4)), g_E=rng.standard_normal((C, 4, 4)))
    return _f32(inp)


def matrices_oracle(inp, case, dtype):
    cam, leaves = oracle_cam(inp, case["mult"], dtype)
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    Km, Em = O.camera_K(cam), O.camera_E(cam)
    loss = 0.0 * Km.sum()
    if case["null"] != "g_K":
        loss = loss + (Km * T("g_K")).sum()
    if case["null"] != "g_E":
        loss = loss + (Em * T("g_E")).sum()
    loss.backward()
    out = dict(K=Km, E=Em)
    for k in ("intr_noise", "extr_noise"):
        if case["null"] != "d_" + k:
            out["d_" + k] = _grad(leaves[k])
    return _np64(out)


def matrices_references(case):
    return _references("matrices", case, matrices_inputs, matrices_oracle)


def run_matrices(route, inp, case):
    C, I, null = case["C"], route.inp, case["null"]
    bufs = dict(K=route.out((4, 4)), E=route.out((C, 4, 4)))
    route.call("scnerf_camera_matrices_fwd", *_cam_args(route, inp, case["mult"], C), bufs["K"][1], bufs["E"][1])
    if null != "d_intr_noise":
        bufs["d_intr_noise"] = route.out((4,))
    if null != "d_extr_noise":
        bufs["d_extr_noise"] = route.out((C, 9))
    view = lambda k: bufs[k][1] if k in bufs else None
    route.call("scnerf_camera_matrices_bwd", I(inp["intr_init"]), INTR_SCALE[case["mult"]], case["mult"], I(inp["extr_init"]),
               I(inp["extr_noise"]), EXTR_SCALE, C, None if null == "g_K" else I(inp["g_K"]),
               None if null == "g_E" else I(inp["g_E"]), view("d_intr_noise"), view("d_extr_noise"))
    return collect(route, bufs)


def check_matrices(case, got):
    _, o64, o32 = matrices_references(case)
    ratios = bound_check("matrices", case_id(case), got, o64, o32, tuple(o64), ("E", "d_extr_noise"))
    # the constant entries are exact: K is the identity outside its four parameters, row 3 of every E is (0, 0, 0, 1)
    mask = np.ones((4, 4), bool)
    mask[[0, 1, 0, 1], [0, 1, 2, 2]] = False
    np.testing.assert_array_equal(got["K"][mask], np.eye(4, dtype=np.float32)[mask])
    np.testing.assert_array_equal(got["E"][:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (case["C"], 1)))
    if case["null"] == "g_K" and "d_intr_noise" in got:
        assert not got["d_intr_noise"].any()
    if case["null"] == "g_E" and "d_extr_noise" in got:
        assert not got["d_extr_noise"].any()
    return ratios


# ---- NDC warp and ray-batch packing ------------------------------------------------------------------------------------------
def ndc_case(n=65, null=None):
    """null: g_ndc_o | g_ndc_d | g_focal_xy passed as NULL"""
    return dict(n=n, null=null)


def pack_case(n=65, cols=11, ndc=1, null=None):
    """ndc: focal_xy given (the NDC warp) or NULL;  null: g_focal_xy passed as NULL"""
    return dict(n=n, cols=cols, ndc=ndc, null=null)


NDC_CASES = [ndc_case(n=n) for n in RAY_COUNTS] + [ndc_case(null=k) for k in ("g_ndc_o", "g_ndc_d", "g_focal_xy")]
PACK_CASES = ([pack_case(n=n) for n in RAY_COUNTS] + [pack_case(cols=8), pack_case(ndc=0), pack_case(cols=8, ndc=0),
                                                       pack_case(null="g_focal_xy"), pack_case(cols=8, null="g_focal_xy")])
NDC_WELL = 0                       # rows i % 8 == NDC_WELL: |d| = 1, |d_z| = 1, origin off the near plane


def ndc_inputs(n, cols=11):
    """rows cycle through |d| in {1, 1e-3, 1e3} x |d_z| / |d| in {1, 1e-2}; every 7th origin lies on the near plane (t = 0)"""
    rng = np.random.default_rng(4000 + n)
    i = np.arange(n)
    mag = np.array([1.0, 1e-3, 1e3, 1.0, 1.0, 1e-3, 1e3, 1.0])[i % 8]
    dz = np.array([1.0, 1.0, 1.0, 1e-2, 1.0, 1e-2, 1e-2, 1.0])[i % 8]
    d = np.stack([0.4 * rng.standard_normal(n), 0.4 * rng.standard_normal(n), -dz * (1.0 + 0.3 * rng.random(n))], -1) * mag[:, None]
    o = 0.3 * rng.standard_normal((n, 3))
    o[i % 7 == 3, 2] = -NDC_NEAR
    inp = dict(o=o, d=d, f2=np.array(NDC_F2), g_no=rng.standard_normal((n, 3)), g_nd=rng.standard_normal((n, 3)),
               g_batch=rng.standard_normal((n, cols)))
    return _f32(inp)


def ndc_oracle(inp, case, dtype):
    H, W = NDC_HW
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    o, d, f = T("o").requires_grad_(True), T("d").requires_grad_(True), T("f2").requires_grad_(True)
    no, nd = O.ndc_rays(H, W, f[0], f[1], NDC_NEAR, o, d)
    loss = 0.0 * no.sum()
    if case["null"] != "g_ndc_o":
        loss = loss + (no * T("g_no")).sum()
    if case["null"] != "g_ndc_d":
        loss = loss + (nd * T("g_nd")).sum()
    loss.backward()
    out = dict(ndc_o=no, ndc_d=nd, g_rays_o=_grad(o), g_rays_d=_grad(d))
    if case["null"] != "g_focal_xy":
        out["g_focal_xy"] = _grad(f)
    return _np64(out)


def ndc_references(case):
    return _references("ndc", case, lambda c: ndc_inputs(c["n"]), ndc_oracle)


def run_ndc(route, inp, case):
    (H, W), n, I, null = NDC_HW, case["n"], route.inp, case["null"]
    o, d, f2 = I(inp["o"]), I(inp["d"]), I(inp["f2"])
    bufs = {k: route.out((n, 3)) for k in ("ndc_o", "ndc_d", "g_rays_o", "g_rays_d")}
    if null != "g_focal_xy":
        bufs["g_focal_xy"] = route.out((2,))
    route.call("scnerf_ndc_fwd", H, W, f2, NDC_NEAR, o, d, bufs["ndc_o"][1], bufs["ndc_d"][1], n)
    route.call("scnerf_ndc_bwd", H, W, f2, NDC_NEAR, o, d, None if null == "g_ndc_o" else I(inp["g_no"]),
               None if null == "g_ndc_d" else I(inp["g_nd"]), bufs["g_rays_o"][1], bufs["g_rays_d"][1],
               bufs["g_focal_xy"][1] if "g_focal_xy" in bufs else None, n)
    return collect(route, bufs)


NDC_PER_RAY = ("ndc_o", "ndc_d", "g_rays_o", "g_rays_d", "pack_o", "pack_d", "pack_v")


def check_ndc(case, got):
    _, o64, o32 = ndc_references(case)
    ratios = bound_check("ndc", "ndc-" + case_id(case), got, o64, o32, tuple(o64), NDC_PER_RAY)
    well = np.arange(case["n"])[np.arange(case["n"]) % 8 == NDC_WELL]
    for k in ("ndc_o", "ndc_d"):                                # the golden tests' ceilings
        np.testing.assert_allclose(got[k][well], o64[k][well], rtol=2e-5, atol=2e-6)
    return ratios


def pack_oracle(inp, case, dtype):
    """render()'s view-direction / NDC / concatenation steps (render.py:105-128) written with torch ops"""
    H, W = NDC_HW
    T = lambda k: torch.from_numpy(inp[k]).to(dtype)
    o, d, f = T("o").requires_grad_(True), T("d").requires_grad_(True), T("f2").requires_grad_(True)
    ro, rd = O.ndc_rays(H, W, f[0], f[1], 1.0, o, d) if case["ndc"] else (o, d)
    ones = torch.ones_like(rd[:, :1])
    cols = [ro, rd, PACK_NEAR_FAR[0] * ones, PACK_NEAR_FAR[1] * ones]
    if case["cols"] > 8:
        cols.append(d / torch.norm(d, dim=-1, keepdim=True))
    batch = torch.cat(cols, -1)
    (batch * T("g_batch")).sum().backward()
    out = dict(pack_o=batch[:, 0:3], pack_d=batch[:, 3:6], g_rays_o=_grad(o), g_rays_d=_grad(d))
    if case["cols"] > 8:
        out["pack_v"] = batch[:, 8:11]
    if case["ndc"] and case["null"] != "g_focal_xy":
        out["g_focal_xy"] = _grad(f)
    return _np64(out)


def pack_references(case):
    return _references("pack", case, lambda c: ndc_inputs(c["n"], c["cols"]), pack_oracle)


def run_pack(route, inp, case):
    (H, W), n, I, cols = NDC_HW, case["n"], route.inp, case["cols"]
    o, d = I(inp["o"]), I(inp["d"])
    f2 = I(inp["f2"]) if case["ndc"] else None
    bufs = dict(batch=route.out((n, cols)), g_rays_o=route.out((n, 3)), g_rays_d=route.out((n, 3)))
    if case["ndc"] and case["null"] != "g_focal_xy":
        bufs["g_focal_xy"] = route.out((2,))
    route.call("scnerf_pack_rays_fwd", H, W, f2, 1.0, o, d, PACK_NEAR_FAR[0], PACK_NEAR_FAR[1], cols, bufs["batch"][1], n)
    route.call("scnerf_pack_rays_bwd", H, W, f2, 1.0, o, d, cols, I(inp["g_batch"]), bufs["g_rays_o"][1], bufs["g_rays_d"][1],
               bufs["g_focal_xy"][1] if "g_focal_xy" in bufs else None, n)
    got = collect(route, bufs)
    b = got.pop("batch")
    got.update(pack_o=b[:, 0:3], pack_d=b[:, 3:6], pack_nf=b[:, 6:8])
    if cols > 8:
        got["pack_v"] = b[:, 8:11]
    return got


def check_pack(case, got):
    _, o64, o32 = pack_references(case)
    ratios = bound_check("ndc", "pack-" + case_id(case), got, o64, o32, tuple(o64), NDC_PER_RAY)
    np.testing.assert_array_equal(got["pack_nf"], np.tile(np.array(PACK_NEAR_FAR, np.float32), (case["n"], 1)))
    if not case["ndc"]:                                         # without the warp the rays are copied
        inp = pack_references(case)[0]
        np.testing.assert_array_equal(got["pack_o"], inp["o"])
        np.testing.assert_array_equal(got["pack_d"], inp["d"])
    return ratios


# ---- grid upsampling: scnerf_upsample_grid_fwd / _bwd --------------------------------------------------------------------------
UPSAMPLE_SCALE = 0.37


def upsample_references(shape):
    def make():
        gh, gw, H, W = shape
        rng = np.random.default_rng(5000 + gh * 100 + H)
        inp = _f32(dict(grid=rng.standard_normal((gh, gw, 3)), g_out=rng.standard_normal((H * W, 3))))
        outs = []
        for dtype in (torch.float64, torch.float32):
            g = torch.from_numpy(inp["grid"]).to(dtype).requires_grad_(True)
            up = O.upsample_noise_grid(g, H, W, UPSAMPLE_SCALE)
            (up * torch.from_numpy(inp["g_out"]).to(dtype)).sum().backward()
            outs.append(_np64(dict(out=up, d_grid=g.grad)))
        assert_finite("upsample %s" % (shape,), *outs)
        return inp, outs[0], outs[1]
    return _cached(("upsample", shape), make)


def run_upsample(route, inp, shape):
    gh, gw, H, W = shape
    bufs = dict(out=route.out((H * W, 3)), d_grid=route.out((gh, gw, 3)))
    route.call("scnerf_upsample_grid_fwd", route.inp(inp["grid"]), UPSAMPLE_SCALE, gh, gw, H, W, bufs["out"][1])
    route.call("scnerf_upsample_grid_bwd", route.inp(inp["g_out"]), UPSAMPLE_SCALE, gh, gw, H, W, bufs["d_grid"][1])
    return collect(route, bufs)


def check_upsample(shape, got):
    _, o64, o32 = upsample_references(shape)
    return bound_check("upsample", "x".join(map(str, shape)), got, o64, o32, ("out", "d_grid"))


# ---- pinhole rays: scnerf_pinhole_rays ---------------------------------------------------------------------------------------
PINHOLE_CASES = [dict(n=65, stride=2, H=48, W=64), dict(n=257, stride=3, H=48, W=64), dict(n=54, stride=0, H=6, W=9)]
PINHOLE_FOCAL = 55.5


def ref_pinhole(H, W, focal, c2w, kps):
    """oracle.scnerf_oracle.pinhole_rays with the directions formed in the dtype of c2w (there: in float32, then cast)"""
    px = kps.long().to(c2w.dtype)
    dirs = torch.stack([(px[:, 0] - W * 0.5) / focal, -(px[:, 1] - H * 0.5) / focal, -torch.ones_like(px[:, 0])], dim=-1)
    rays_d = torch.sum(dirs[:, None, :] * c2w[:3, :3], dim=-1)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def pinhole_references(case):
    def make():
        n, H, W = case["n"], case["H"], case["W"]
        rng = np.random.default_rng(6000 + n)
        c2w = np.eye(4)
        c2w[:3] = rng.standard_normal((3, 4))
        inp = dict(c2w=c2w)
        if case["stride"]:                                      # fractional key points are truncated; extra columns ignored
            kps = rng.random((n, case["stride"])) * 40.0
            kps[:, 0], kps[:, 1] = rng.random(n) * (W - 1), rng.random(n) * (H - 1)
            kps[:3, :2] = [(0, 0), (W - 1, H - 1), (12.999999, 7.5)]
            inp["kps"] = kps
            pix = kps[:, :2].astype(np.float32)
        else:
            yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            pix = np.stack([xx.reshape(-1), yy.reshape(-1)], -1).astype(np.float32)
        inp = _f32(inp)
        outs = []
        for dtype in (torch.float64, torch.float32):
            ro, rd = ref_pinhole(H, W, PINHOLE_FOCAL, torch.from_numpy(inp["c2w"]).to(dtype), torch.from_numpy(pix))
            outs.append(_np64(dict(rays_o=ro, rays_d=rd)))
        ro, rd = O.pinhole_rays(H, W, PINHOLE_FOCAL, torch.from_numpy(inp["c2w"]), torch.from_numpy(pix))
        assert torch.equal(rd, torch.from_numpy(outs[1]["rays_d"]).float()), "ref_pinhole is not oracle.pinhole_rays"
        return inp, outs[0], outs[1]
    return _cached(("pinhole", _key(case)), make)


def run_pinhole(route, inp, case):
    n = case["n"]
    bufs = dict(rays_o=route.out((n, 3)), rays_d=route.out((n, 3)))
    route.call("scnerf_pinhole_rays", route.inp(inp["kps"]) if case["stride"] else None, case["stride"], route.inp(inp["c2w"]),
               PINHOLE_FOCAL, case["H"], case["W"], bufs["rays_o"][1], bufs["rays_d"][1], n)
    return collect(route, bufs)


def check_pinhole(case, got):
    inp, o64, o32 = pinhole_references(case)
    np.testing.assert_array_equal(got["rays_o"], np.tile(inp["c2w"][:3, 3], (case["n"], 1)))
    return bound_check("rays", "pinhole-" + case_id(case), got, o64, o32, ("rays_o", "rays_d"), ("rays_o", "rays_d"))


# ---- empty batches -----------------------------------------------------------------------------------------------------------
def run_and_check_empty(route):
    """n = 0 through every entry point that takes n: status 0 (route.call asserts it), guards intact (collect asserts it), the
    accumulated gradients exactly zero"""
    for pose in ("idx", "single", "shared", "perray"):
        case = rays_case(n=0, pose=pose)
        got = run_rays(route, rays_inputs(case), case)
        for k in ("d_intr_noise", "d_extr_noise", "d_grid_o", "d_grid_d", "d_extrinsic"):
            assert k not in got or not got[k].any(), (pose, k)
        assert got["rays_o"].shape == (0, 3) and ("d_extrinsic" in got) == (pose in ("shared", "perray"))
    for pose in ("single", "shared"):
        case = npp_case(n=0, pose=pose)
        got = run_npp(route, npp_inputs(case), case)
        for k in ("d_intr_noise", "d_extr_noise", "d_grid_o", "d_grid_d", "d_extrinsic", "d_dist2"):
            assert k not in got or not got[k].any(), ("npp", pose, k)
    got = run_ndc(route, ndc_inputs(0), ndc_case(n=0))
    assert not got["g_focal_xy"].any()
    for cols in (8, 11):
        got = run_pack(route, ndc_inputs(0, cols), pack_case(n=0, cols=cols))
        assert not got["g_focal_xy"].any()
    case = dict(n=0, stride=2, H=48, W=64)
    run_pinhole(route, dict(kps=np.zeros((0, 2), np.float32), c2w=np.eye(4, dtype=np.float32)), case)
