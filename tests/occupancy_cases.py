"""TEST INFRASTRUCTURE shared by tests/test_emu_occupancy.py and tests/test_gpu_occupancy.py: the case bodies of the
occupancy grid (csrc/occupancy.hip, scnerf_amd/occupancy.py, ops.inference_occupancy).

The kernel cases are written against a `backend` that runs the C ABI on numpy arrays -- the CPU SIMT interpreter build (host
pointers) or the product library (device copies) -- and compare with tests/occupancy_reference.py for EQUALITY, every
launch twice for identical bytes.  The render cases compare a forward-only render_rays call under the switch, bit for bit,
with an oracle built here from the stand-alone launches: the samplers, a DENSE ops.mlp_fwd with samples_per_ray = 1 and
expanded view directions, the rows of the dead samples zeroed in torch by the transcription's mask, ops.composite_fwd."""
import numpy as np
import torch

from scnerf_amd import synthetic as synth
from tests import occupancy_reference as REF
from tests import skip_empty_case as SE

SENTINEL = -7
EINVAL = -22
ALL_TWELVE = SE.ALL_TWELVE

# ---- the kernels ---------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 70 * 16, 4 * 1024 + 49)
GRIDS = ("all", "none", "ball")
KR = 32
KLO, KHI = (0.0, -2.0, -3.0), (4.0, 2.0, 1.0)          # lo_x = 0: a coordinate -0.0 is inside, in cell 0


def kernel_grid(kind, R=KR):
    """-> (bits, R, lo, inv) of the kernel cases: every cell, no cell, the cells whose centre is within 1.5 of the box's"""
    lo, hi, inv, cell = REF.box(KLO, KHI, R)
    if kind == "all":
        mask = np.ones((R, R, R), bool)
    elif kind == "none":
        mask = np.zeros((R, R, R), bool)
    else:
        c = (np.arange(R) + 0.5) / R * 4.0 - 2.0
        mask = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= 1.5 ** 2
    return REF.bits_of_mask(mask), R, lo, inv


def kernel_points(P, spr, seed=0):
    """-> (pts [P, 3], viewdirs [rays, 5] with two unused columns: a row stride of 5).  Points over a box a quarter wider
    than the grid's; rows 0 .. 4 (where P has them): exactly on lo (inside, cell 0), x exactly on hi (outside: live), a NaN
    y (live), x = -0.0 (inside), a huge coordinate (outside)."""
    rng = np.random.default_rng(100 * seed + P)
    lo, hi = np.asarray(KLO, np.float32), np.asarray(KHI, np.float32)
    pts = (lo - 0.5 + rng.random((P, 3), dtype=np.float32) * (hi - lo + 1.0)).astype(np.float32)
    special = [lo.copy(), np.array([hi[0], 0.0, -1.0], np.float32), np.array([1.0, np.nan, -1.0], np.float32),
               np.array([-0.0, -1.9, -2.9], np.float32), np.array([3e38, 0.0, -1.0], np.float32)]
    for i, row in enumerate(special[:P]):
        pts[i] = row
    rays = (P + spr - 1) // spr
    vd = rng.standard_normal((max(rays, 1), 5)).astype(np.float32)
    return pts, vd


def check_compact_and_expand(backend, P, spr, kind):
    bits, R, lo, inv = kernel_grid(kind)
    pts, vd = kernel_points(P, spr)
    live, slot_of, pts_live, vd_live = REF.compact(pts, vd, spr, bits, R, lo, inv)
    nl = live.shape[0]
    dead = REF.dead_mask(pts, bits, R, lo, inv)
    if kind == "all":
        assert nl == P
    if kind == "none" and P >= 5:
        assert dead[0] and not dead[1] and not dead[2] and dead[3] and not dead[4] and 0 < nl < P
    if kind == "ball" and P >= 63:
        assert 0 < nl < P
    runs = [backend.compact(pts, vd, 5, spr, bits, R, lo, inv) for _ in range(2)]
    for got_idx, got_slot, got_pts, got_vd, n_dev, n_host in runs:
        assert n_dev == nl and n_host == nl, (n_dev, n_host, nl)
        assert np.array_equal(got_idx[:nl], live) and (np.diff(got_idx[:nl]) > 0).all()
        assert (got_idx[nl:] == SENTINEL).all(), "live_idx written past n_live"
        assert np.array_equal(got_slot, slot_of) and (got_slot[dead] == -1).all()
        assert got_pts[:nl].tobytes() == pts_live.tobytes() and got_vd[:nl].tobytes() == vd_live.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][:4], runs[1][:4]))
    rng = np.random.default_rng(P + 1)
    raw_live = rng.standard_normal((nl, 4)).astype(np.float32)
    if nl:
        raw_live[rng.integers(0, nl), 1] = np.nan                     # bits travel, whatever they are
    want = REF.expand(raw_live, slot_of)
    outs = [backend.expand(raw_live, slot_of, nl) for _ in range(2)]
    for got in outs:
        assert got.shape == (P, 4) and got.tobytes() == want.tobytes()
    assert (want[dead] == 0).all()


def check_probe_points(backend, k):
    R = 32
    lo, hi, inv, cell = REF.box((-1.5, -1.0, 0.25), (1.5, 2.0, 0.75), R)
    for first, n_cells in ((0, 64), (64 * 37, 64 * 3 + 17), (R ** 3 - 64, 64)):
        want = REF.probe_points(first, n_cells, R, k, lo, cell)
        runs = [backend.probe(first, n_cells, R, k, lo, cell) for _ in range(2)]
        for got in runs:
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (k, first)
        # every point lies in its own cell by the samples' lookup
        c = first + np.arange(n_cells).repeat(k ** 3)
        t = ((want - lo) * inv).astype(np.float32)
        assert np.array_equal(np.floor(t).astype(np.int64), np.stack([c % R, (c // R) % R, c // (R * R)], 1))


def check_accumulate(backend, k):
    """synthetic raw, no network: sigma == sigma_min does not set a cell, the next float above it does, a NaN does (the
    conservative choice: a density we cannot read is not empty space); two accumulations OR together"""
    R, first, n_cells, k3 = 32, 64 * 3, 64 * 5 + 17, k ** 3
    sigma_min = np.float32(0.25)
    rng = np.random.default_rng(k)
    raws = []
    for rep in range(2):
        raw = rng.standard_normal((n_cells, k3, 4)).astype(np.float32)
        raw[:, :, 3] -= np.float32(1.2)                                # most cells stay empty
        below = np.float32(-3.0)
        raw[0 + 8 * rep, :, 3] = sigma_min                             # not set
        raw[1 + 8 * rep, :, 3] = sigma_min
        raw[1 + 8 * rep, k3 - 1, 3] = np.nextafter(sigma_min, np.float32(1))      # set
        raw[2 + 8 * rep, :, 3] = below
        raw[2 + 8 * rep, 0, 3] = np.nan                                # set
        raw[3 + 8 * rep, :, 3] = below                                 # not set
        raws.append(raw.reshape(-1, 4))
    zero = np.zeros(R ** 3 // 32, np.int32)
    one = REF.accumulate(zero, raws[0], sigma_min, first, n_cells, R, k)
    m = REF.mask_of_bits(one, R).reshape(-1)
    assert not m[first + 0] and m[first + 1] and m[first + 2] and not m[first + 3]
    assert 0 < m.sum() < n_cells and not m[:first].any() and not m[first + n_cells:].any()
    both = REF.accumulate(one, raws[1], sigma_min, first, n_cells, R, k)
    assert REF.mask_of_bits(both, R).sum() > m.sum()
    for _ in range(2):
        got = backend.accumulate(raws[0], sigma_min, first, n_cells, R, k, zero.copy())
        assert got.tobytes() == one.tobytes()
        got = backend.accumulate(raws[1], sigma_min, first, n_cells, R, k, got)
        assert got.tobytes() == both.tobytes()


def dilate_cells(R):
    """single set cells (x, y, z): two corners, an edge, bit 31 and bit 0 of a word, the interior"""
    return [(0, 0, 0), (R - 1, R - 1, R - 1), (0, 5, R - 1), (31, 7, 9), (R - 32, 9, 7), (10, 11, 12)]


def check_dilate(backend, R):
    for x, y, z in dilate_cells(R):
        mask = np.zeros((R, R, R), bool)
        mask[z, y, x] = True
        bits = REF.bits_of_mask(mask)
        for rounds in (1, 2):
            cube = np.zeros_like(mask)
            cube[max(z - rounds, 0):z + rounds + 1, max(y - rounds, 0):y + rounds + 1, max(x - rounds, 0):x + rounds + 1] = True
            runs = []
            for _ in range(2):
                got = bits
                for _r in range(rounds):
                    got = backend.dilate(got, R)
                runs.append(got)
                assert np.array_equal(REF.mask_of_bits(got, R), cube), (R, (x, y, z), rounds)
            assert runs[0].tobytes() == runs[1].tobytes()
    # a random grid against the transcription
    rng = np.random.default_rng(R)
    bits = REF.bits_of_mask(rng.random((R, R, R)) < 0.01)
    assert backend.dilate(bits, R).tobytes() == REF.dilate(bits, R).tobytes()


# ---- the render path -------------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI, BOX_R = (-2.0, -2.0, -3.0), (2.0, 2.0, 1.0), 32


def mixed_mask(R=BOX_R):
    """[z, y, x]: a cell is set when its centre is within 1.0 of (0, 0, -1)"""
    c = (np.arange(R, dtype=np.float64) + 0.5) * (4.0 / R)
    x, y, z = c - 2.0, c - 2.0, c - 3.0
    return (z[:, None, None] + 1.0) ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2 <= 1.0


def hand_grid(mask, device, lo=BOX_LO, hi=BOX_HI):
    from scnerf_amd.occupancy import OccupancyGrid
    return OccupancyGrid.from_mask(torch.from_numpy(np.ascontiguousarray(mask)), lo, hi).to(device)


def node(rays, nets, sc, sf, white_bkgd=False, lindisp=False, randoms=None, noise=None):
    """the twelve outputs of a forward-only call of the render node"""
    from scnerf_amd.functional import RenderConfig, RenderRaysFunction
    r = randoms or {}
    nz = noise or {}
    with torch.no_grad():
        cfg = RenderConfig(sc, sf, lindisp, white_bkgd, torch.is_grad_enabled())
        params = list(nets[0].ordered_parameters()) + (list(nets[1].ordered_parameters()) if nets[1] is not None else [])
        return dict(zip(ALL_TWELVE, RenderRaysFunction.apply(rays, cfg, r.get("t_rand"), r.get("u"), nz.get("noise_c"),
                                                             nz.get("noise_f"), nets[0], nets[1], *params)))


def grid_arrays(grid):
    return (grid.bits.cpu().numpy(), grid.resolution, np.asarray(grid.lo, np.float32), np.asarray(grid.inv, np.float32))


def _masked_network(ops, pts, rays, spr, net, n, grid):
    """dense network on every sample with one view direction per sample, the dead rows zeroed -> (raw [n, spr, 4], dead)"""
    flat = net.flat_parameters()
    wf, pl = ops.network_packs(net, flat, False, n)
    vd = rays[:, 8:11].repeat_interleave(spr, 0).contiguous()
    raw = ops.mlp_fwd(pts.view(-1, 3), vd, 1, wf, None, planes=pl)
    dead = torch.from_numpy(REF.dead_mask(pts.cpu().numpy(), *grid_arrays(grid))).to(raw.device)
    raw = torch.where(dead[:, None], torch.zeros_like(raw), raw)
    return raw.view(n, spr, 4), dead.view(n, spr)


def coarse_oracle(ops, rays, nets, sc, grid, white_bkgd=False, lindisp=False, randoms=None):
    from scnerf_amd.functional import host_linspace
    r = randoms or {}
    n = rays.shape[0]
    z_c, pts_c = ops.coarse_sample(rays, host_linspace(sc, rays.device), r.get("t_rand"), lindisp)
    raw_c, dead_c = _masked_network(ops, pts_c, rays, sc, nets[0], n, grid)
    rgb_c, disp_c, acc_c, w_c, depth_c = ops.composite_fwd(raw_c, z_c, rays, None, white_bkgd)
    return {"z": z_c, "pts": pts_c, "raw": raw_c, "dead": dead_c, "w": w_c, "out": (rgb_c, disp_c, acc_c, depth_c)}


def fine_oracle(ops, rays, nets, sc, sf, grid, z_c, w_c, white_bkgd=False, randoms=None):
    """-> (rgb, disp, acc, depth, raw, z_std, z_vals, z_samples, dead mask [n, sc + sf]) of the fine stage on `rays`"""
    from scnerf_amd.functional import host_linspace
    r = randoms or {}
    n = rays.shape[0]
    u = r["u"] if "u" in r else host_linspace(sf, rays.device)
    z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, u)
    raw_f, dead_f = _masked_network(ops, pts_f, rays, sc + sf, nets[1] if nets[1] is not None else nets[0], n, grid)
    rgb_f, disp_f, acc_f, _, depth_f = ops.composite_fwd(raw_f, z_f, rays, None, white_bkgd, want_weights=False)
    return rgb_f, disp_f, acc_f, depth_f, raw_f, z_std, z_f, z_s, dead_f


def oracle(ops, rays, nets, sc, sf, grid, white_bkgd=False, lindisp=False, randoms=None):
    """section 1 of the feature as stand-alone launches -> (the twelve outputs, the coarse stage's dead mask [n, sc], the
    coarse points, the number of dead samples of both stages)"""
    assert ops.inference_occupancy() is None
    with torch.no_grad():
        c = coarse_oracle(ops, rays, nets, sc, grid, white_bkgd, lindisp, randoms)
        rgb_c, disp_c, acc_c, depth_c = c["out"]
        n_dead = int(c["dead"].sum())
        if sf == 0:
            out = (rgb_c, disp_c, acc_c, depth_c, c["raw"], None, None, None, None, None, c["z"], None)
        else:
            rgb_f, disp_f, acc_f, depth_f, raw_f, z_std, z_f, z_s, dead_f = fine_oracle(ops, rays, nets, sc, sf, grid, c["z"],
                                                                                       c["w"], white_bkgd, randoms)
            out = (rgb_f, disp_f, acc_f, depth_f, raw_f, rgb_c, disp_c, acc_c, depth_c, z_std, z_f, z_s)
            n_dead += int(dead_f.sum())
    return dict(zip(ALL_TWELVE, out)), c["dead"], c["pts"], n_dead


def same_twelve(got, want, what=""):
    for k in ALL_TWELVE:
        if want[k] is None:
            assert got[k] is None, what + k
        else:
            SE.same_bits(got[k], want[k], what + k)


def with_grid(ops, grid, fn):
    ops.inference_occupancy(grid)
    try:
        return fn()
    finally:
        ops.inference_occupancy("off")


def mixed_case(ops, device, nets, n, sc, sf, white_bkgd=False, lindisp=False, randoms=None, what=""):
    """synthetic.ray_batch(n, seed=1) through the ball grid: the call under the switch equals the oracle in all twelve
    outputs; the batch holds every kind of ray and sample; occupancy_stats() reports this call's counts.  With `lindisp`
    the batch is synthetic.ray_batch's lindisp one (near 0.25, far 1.5: at near = 0 the reference's 1 / (1 / near ...) depths
    are NaN); its rays start further out, and at 16 coarse samples none of them has every sample dead (computed on the
    CPU: live share 0.71 .. 0.74, 1 .. 11 rays all live, 3 .. 5 % of the samples outside) -- that one population check is
    the plain batch's alone."""
    rays = synth.ray_batch(n, seed=1, lindisp=lindisp).to(device)
    grid = hand_grid(mixed_mask(), device)
    want, dead_c, pts_c, n_dead = oracle(ops, rays, nets, sc, sf, grid, white_bkgd, lindisp, randoms)
    share = 1.0 - float(dead_c.float().mean())
    assert 0.25 <= share <= 0.75, share
    assert lindisp or bool(dead_c.all(1).any()), "no ray with every coarse sample dead"
    assert bool((~dead_c).all(1).any()), "no ray with every coarse sample live"
    p = pts_c.cpu().numpy().reshape(-1, 3)
    outside = ((p < np.asarray(BOX_LO, np.float32)) | (p >= np.asarray(BOX_HI, np.float32))).any(1)
    assert outside.any(), "no sample outside the box"
    ops.occupancy_stats(reset=True)
    got = with_grid(ops, grid, lambda: node(rays, nets, sc, sf, white_bkgd, lindisp, randoms))
    stats = ops.occupancy_stats(reset=True)
    same_twelve(got, want, what)
    assert stats == {"samples": n * sc + (n * (sc + sf) if sf else 0), "skipped": n_dead}, (stats, n_dead)
    return rays, grid, got


def all_set_case(ops, device, nets, n, sc, sf, what=""):
    """a grid with every bit set returns the switch-off call's bits"""
    rays = synth.ray_batch(n, seed=1).to(device)
    off = node(rays, nets, sc, sf)
    grid = hand_grid(np.ones((BOX_R,) * 3, bool), device)
    ops.occupancy_stats(reset=True)
    on = with_grid(ops, grid, lambda: node(rays, nets, sc, sf))
    assert ops.occupancy_stats(reset=True) == {"samples": n * (2 * sc + sf), "skipped": 0}
    same_twelve(on, off, what)


class _NoPacks:
    """a pack cache that must not be asked: stands in for ops.network_packs' result"""


def none_set_case(ops, device, nets, n, sc, sf, monkeypatch):
    """no bit set and a box that holds every sample: no network launch at all, the background colour, acc = 0"""
    rays = synth.ray_batch(n, seed=1).to(device)
    grid = hand_grid(np.zeros((BOX_R,) * 3, bool), device, lo=(-64.0,) * 3, hi=(64.0,) * 3)
    launched = []
    real = ops.mlp_fwd
    monkeypatch.setattr(ops, "mlp_fwd", lambda *a, **k: (launched.append(1), real(*a, **k))[1])
    for white in (False, True):
        ops.occupancy_stats(reset=True)
        got = with_grid(ops, grid, lambda: node(rays, nets, sc, sf, white_bkgd=white))
        assert ops.occupancy_stats(reset=True) == {"samples": n * (2 * sc + sf), "skipped": n * (2 * sc + sf)}
        assert not launched, "a network was launched"
        bg = 1.0 if white else 0.0
        for k in ("rgb_map", "rgb0"):
            assert got[k].shape == (n, 3) and (got[k] == bg).all(), k
        for k in ("acc_map", "acc0"):
            assert (got[k] == 0).all(), k
        assert got["raw"].shape == (n, sc + sf, 4) and (got["raw"] == 0).all()
    monkeypatch.setattr(ops, "mlp_fwd", real)


def with_skip_empty_case(ops, device, nets, n, sc, sf):
    """with inference_skip_empty(tau): the coarse stage with the grid, ray compaction by acc0, the fine stage with the grid
    on the live rays -- written out by hand.  tau = the median of the grid-on acc0; both kinds of ray present."""
    rays = synth.ray_batch(n, seed=1).to(device)
    grid = hand_grid(mixed_mask(), device)
    with torch.no_grad():
        c = coarse_oracle(ops, rays, nets, sc, grid)
        rgb_c, disp_c, acc_c, depth_c = c["out"]
        tau = float(acc_c.median())
        assert 0.0 <= tau < 1.0, tau
        live = SE.live_mask(acc_c, tau)
        n_live = int(live.sum())
        assert 0.25 * n <= n_live <= 0.75 * n, (n_live, n, tau)
        sub = fine_oracle(ops, rays[live].contiguous(), nets, sc, sf, grid, c["z"][live].contiguous(), c["w"][live].contiguous())
    ops.skip_empty_stats(reset=True)
    ops.inference_skip_empty(tau)
    try:
        got = with_grid(ops, grid, lambda: node(rays, nets, sc, sf))
    finally:
        ops.inference_skip_empty("off")
    assert ops.skip_empty_stats(reset=True) == {"rays": n, "skipped": n - n_live}
    dead = ~live
    for k, t in zip(("rgb_map", "disp_map", "acc_map", "depth_map", "raw", "z_std", "z_vals", "z_samples"), sub[:8]):
        SE.same_bits(got[k][live], t, "live rays: " + k)
    for k, t in zip(("rgb_map", "disp_map", "acc_map", "depth_map"), (rgb_c, disp_c, acc_c, depth_c)):
        SE.same_bits(got[k][dead], t[dead], "skipped rays: " + k)
    for k, t in zip(("rgb0", "disp0", "acc0", "depth0"), (rgb_c, disp_c, acc_c, depth_c)):
        SE.same_bits(got[k], t, k)
    for k in ("z_std", "raw", "z_vals", "z_samples"):
        assert (got[k][dead] == 0).all(), k


def noise_case(ops, device, nets, n, sc, sf):
    """a call with density noise does not notice the switch"""
    rays = synth.ray_batch(n, seed=1).to(device)
    rnd = {k: v.to(device) for k, v in synth.render_randoms(n, sc, sf, seed=3).items()}
    noise = {"noise_c": rnd["noise_c"], "noise_f": rnd["noise_f"]}
    off = node(rays, nets, sc, sf, noise=noise)
    ops.occupancy_stats(reset=True)
    on = with_grid(ops, hand_grid(mixed_mask(), device), lambda: node(rays, nets, sc, sf, noise=noise))
    assert ops.occupancy_stats(reset=True) == {"samples": 0, "skipped": 0}
    same_twelve(on, off)


def tracking_case(ops, device, nets, n, sc, sf):
    """a call that tracks gradients does not notice the switch: outputs and gradients"""
    from scnerf_amd import render as R

    def step():
        for net in nets:
            for q in net.parameters():
                q.grad = None
        rays = synth.ray_batch(n, seed=5).to(device).requires_grad_(True)
        ret = R.render_rays(rays, nets[0], SE.query(), sc, retraw=True, perturb=0.0, N_importance=sf, network_fine=nets[1])
        ((ret["rgb_map"] ** 2).sum() + (ret["rgb0"] ** 2).sum() + ret["acc0"].sum()).backward()
        grads = [q.grad.detach().clone() for net in nets for q in net.parameters()]
        return {k: v.detach().clone() for k, v in ret.items()}, rays.grad.clone(), grads

    a = step()
    ops.occupancy_stats(reset=True)
    b = with_grid(ops, hand_grid(mixed_mask(), device), step)
    assert ops.occupancy_stats(reset=True) == {"samples": 0, "skipped": 0}          # the compaction never ran
    for k in a[0]:
        SE.same_bits(a[0][k], b[0][k], k)
    SE.same_bits(a[1], b[1], "d rays")
    assert len(a[2]) == len(b[2]) and any(float(g.abs().max()) > 0 for g in a[2])
    for i, (ga, gb) in enumerate(zip(a[2], b[2])):
        SE.same_bits(ga, gb, "gradient of parameter %d" % i)


def bake_case(ops, device, nets, probes, R=32, first=None, n_cells=None, sigma_min=0.0, dilate=1):
    """OccupancyGrid.bake against the transcription fed with the very raw ops.mlp_fwd returns for the probe points; the
    state_dict round trip; occupied_fraction.  `first` / `n_cells`: compare one pass's cells only through the stand-alone
    ops (the interpreter twin), else the whole bake."""
    from scnerf_amd.occupancy import OccupancyGrid
    lo, hi, inv, cell = REF.box((-1.5,) * 3, (1.5,) * 3, R)
    k = probes
    direction = torch.tensor([[0.0, 0.0, 1.0]], device=device)
    want = np.zeros(R ** 3 // 32, np.int32)
    whole = first is None
    from scnerf_amd.occupancy import MAX_PASS_POINTS
    per_pass = MAX_PASS_POINTS // k ** 3 // 64 * 64               # the passes the bake itself makes
    passes = [(f, min(per_pass, R ** 3 - f)) for f in range(0, R ** 3, per_pass)] if whole else [(first, n_cells)]
    got_bits = torch.zeros(R ** 3 // 32, dtype=torch.int32, device=device)
    with torch.no_grad():
        for f, nc in passes:
            pts = ops.occ_probe_points(f, nc, R, k, [float(x) for x in lo], [float(x) for x in cell], device)
            assert pts.cpu().numpy().tobytes() == REF.probe_points(f, nc, R, k, lo, cell).tobytes()
            for net in nets:
                wf, pl = ops.network_packs(net, net.flat_parameters(), False, pts.shape[0])
                raw = ops.mlp_fwd(pts, direction, pts.shape[0], wf, None, planes=pl)
                want = REF.accumulate(want, raw.cpu().numpy(), sigma_min, f, nc, R, k)
                if not whole:
                    ops.occ_accumulate(raw, sigma_min, f, nc, R, k, got_bits)
    if not whole:
        assert got_bits.cpu().numpy().tobytes() == want.tobytes()
        assert 0 < REF.mask_of_bits(want, R).sum()
        return None
    for _ in range(dilate):
        want = REF.dilate(want, R)
    grid = OccupancyGrid.bake(nets, lo, hi, resolution=R, probes=k, sigma_min=sigma_min, dilate=dilate)
    assert grid.bits.cpu().numpy().tobytes() == want.tobytes()
    pop = int(REF.mask_of_bits(want, R).sum())
    assert grid.occupied_fraction() == pop / float(R ** 3)
    back = OccupancyGrid.from_state_dict(grid.state_dict())
    assert back.bits.numpy().tobytes() == want.tobytes() and back.lo == grid.lo and back.hi == grid.hi and back.inv == grid.inv
    assert back.resolution == R
    return grid


def stale_and_foreign_case(ops, device, nets, grid=None):
    """a baked grid serves the networks it was baked from, with the weights it was baked from"""
    from scnerf_amd.occupancy import OccupancyGrid, OccupancyStaleError
    import pytest
    if grid is None:
        # (bound by hand: what from_state_dict(sd, networks) does after a bake)
        grid = OccupancyGrid.from_state_dict(hand_grid(mixed_mask(), device).state_dict(), networks=nets)
    rays = synth.ray_batch(8, seed=1).to(device)
    grid.check(*nets)
    with_grid(ops, grid, lambda: node(rays, nets, 16, 8))
    others = SE.networks(device)
    with pytest.raises(OccupancyStaleError):
        with_grid(ops, grid, lambda: node(rays, others, 16, 8))
    with torch.no_grad():
        nets[1].alpha_linear.bias.add_(0.0)               # an in-place write: the version moves, whatever the value
    with pytest.raises(OccupancyStaleError):
        with_grid(ops, grid, lambda: node(rays, nets, 16, 8))
    # a grid made by hand checks nothing
    with_grid(ops, hand_grid(mixed_mask(), device), lambda: node(rays, others, 16, 8))


def switch_validation(ops):
    import pytest
    assert ops.inference_occupancy() is None
    for bad in (0.5, "on", True, object()):
        with pytest.raises(ValueError):
            ops.inference_occupancy(bad)
        assert ops.inference_occupancy() is None
    grid = hand_grid(mixed_mask(), "cpu")
    assert ops.inference_occupancy(grid) is grid and ops.inference_occupancy() is grid
    assert ops.inference_occupancy("off") is None and ops.inference_occupancy() is None
    assert ops.occupancy_stats(reset=True).keys() == {"samples", "skipped"}
    assert ops.occupancy_stats() == {"samples": 0, "skipped": 0}
