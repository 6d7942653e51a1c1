"""TEST INFRASTRUCTURE shared by tests/test_emu_early_stop.py and tests/test_gpu_early_stop.py: the case bodies of early ray
termination (csrc/early_stop.hip, ops.inference_early_stop).

The kernel cases are written against a `backend` that runs the C ABI on numpy arrays -- the CPU SIMT interpreter build (host
pointers) or the product library (device copies).  Compaction and expansion are compared with tests/early_stop_reference.py
for EQUALITY, every launch twice for identical bytes, outputs pre-filled with sentinels / NaN.  The transmittance is
compared to 1e-12 relative with an fp64 numpy product of the fp32 q the backend's own compositing computes (device_q), and
the decisions must be the ones that follow from the kernel's OWN transmittance.

The render cases compare a forward-only render_rays call under the switch, bit for bit in all twelve outputs, with an
oracle built here from the stand-alone launches: the project's samplers, a DENSE ops.mlp_fwd with samples_per_ray = 1 and
expanded view directions, the rows behind the stop_segment the call's kernels produced (ops.early_stop_last) zeroed in
torch, the project's compositing.  The stop decisions themselves are checked against an independent fp64 recomputation
from the dense raw."""
import numpy as np
import torch

from scnerf_amd import synthetic as synth
from tests import early_stop_reference as REF
from tests import occupancy_cases as OC
from tests import occupancy_reference as OREF
from tests import skip_empty_case as SE

SENTINEL = OC.SENTINEL
EINVAL = OC.EINVAL
ALL_TWELVE = SE.ALL_TWELVE

# ---- the kernels ---------------------------------------------------------------------------------------------------------
RAYS = (0, 1, 3, 4, 5, 257)
SAMPLES = (2, 5, 64, 65, 130, 192)
SEGMENTS = (2, 3, 8)
PATTERNS = ("all", "none", "alternating")
KEPS = 1e-3


def alive_pattern(kind, n):
    if kind == "all":
        return np.ones(n, np.int32)
    if kind == "none":
        return np.zeros(n, np.int32)
    return (np.arange(n) % 2 == 0).astype(np.int32) * 7          # (any non-zero flag is alive)


def check_compact_and_expand(backend, n, S):
    """every K <= S, every segment: the three alive patterns without a grid (and the opening pass's "no flags"), the three
    grids under the alternating pattern"""
    pts, vd = OC.kernel_points(n * S, S)
    rng = np.random.default_rng(7 * n + S)
    for K in SEGMENTS:
        if K > S:
            continue
        b = REF.bounds(S, K)
        assert b[0] == 0 and b[K] == S and all(b[k + 1] > b[k] for k in range(K))
        for k in range(K):
            first, length = b[k], b[k + 1] - b[k]
            combos = [(None, None)] + [(p, None) for p in PATTERNS] + [("alternating", g) for g in OC.GRIDS]
            for pattern, kind in combos:
                alive = None if pattern is None else alive_pattern(pattern, n)
                grid = None if kind is None else OC.kernel_grid(kind)
                live, slot_of, pts_live, vd_live, n_rays = REF.compact(pts, vd, S, first, length, alive, grid)
                nl, E = live.shape[0], n * length
                what = (n, S, K, k, pattern, kind)
                if kind is None and pattern in (None, "all"):
                    assert nl == E and n_rays == n
                if pattern == "none":
                    assert nl == 0 and n_rays == 0
                runs = [backend.compact(pts, vd, 5, S, first, length, alive, grid) for _ in range(2)]
                for got_idx, got_slot, got_pts, got_vd, c_dev, c_host in runs:
                    assert tuple(c_dev) == (nl, n_rays) and tuple(c_host) == (nl, n_rays), (what, c_dev, c_host, nl, n_rays)
                    assert np.array_equal(got_idx[:nl], live) and (np.diff(got_idx[:nl]) > 0).all(), what
                    assert (got_idx[nl:] == SENTINEL).all(), "live_idx written past n_live"
                    assert np.array_equal(got_slot, slot_of), what
                    assert got_pts[:nl].tobytes() == pts_live.tobytes() and got_vd[:nl].tobytes() == vd_live.tobytes(), what
                    assert np.isnan(got_pts[nl:]).all() and np.isnan(got_vd[nl:]).all(), "live rows written past n_live"
                assert all(a.tobytes() == c.tobytes() for a, c in zip(runs[0][:4], runs[1][:4]))
                # the expansion: every row of the segment, no row outside it
                raw_live = rng.standard_normal((nl, 4)).astype(np.float32)
                if nl:
                    raw_live[rng.integers(0, nl), 1] = np.nan                 # bits travel, whatever they are
                before = np.full((n * S, 4), np.nan, np.float32)
                before.view(np.uint32)[:] = 0x7fc00000 + 1 + np.arange(n * S * 4, dtype=np.uint32).reshape(-1, 4) % 1000
                want = REF.expand(before, raw_live, slot_of, S, first, length)
                outs = [backend.expand(raw_live, slot_of, before, n, S, first, length, nl) for _ in range(2)]
                for got in outs:
                    assert got.shape == (n * S, 4) and got.tobytes() == want.tobytes(), what
                if n:
                    seg = np.zeros((n, S), bool)
                    seg[:, first:first + length] = True
                    w = want.reshape(n, S, 4)
                    assert w[~seg].tobytes() == before.reshape(n, S, 4)[~seg].tobytes()
                    assert not np.isnan(w[seg][:, [0, 2, 3]]).any(), "a row of the segment was not written"


def transmittance_inputs(n, S, K):
    """-> (raw [n, S, 4], z [n, S], rays [n, 11]).  Densities over five decades so that rays stop behind every segment
    and some never; where n has them: ray 0 sigma = 0 throughout (T stays the product of fl32(1 + 1e-10) = 1), ray 1 a NaN
    sigma (the compositing's relu makes it 0: alive), ray 2 zeros and ONE huge sigma in the last sample of segment
    (K - 1) // 2 (stops exactly there), ray 3 a NaN depth (a NaN T: never stopped)."""
    rng = np.random.default_rng(1000 * n + 10 * S + K)
    z = np.sort(rng.uniform(2.0, 6.0, (n, S)).astype(np.float32), 1)
    z += np.arange(S, dtype=np.float32)[None, :] * np.float32(1e-3)                # strictly increasing
    rays = rng.standard_normal((n, 11)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (n, 1)))
    raw = rng.standard_normal((n, S, 4)).astype(np.float32)
    raw[:, :, 3] = (rng.standard_normal((n, S)) * scale + 0.3 * scale).astype(np.float32)
    b = REF.bounds(S, K)
    kk = (K - 1) // 2
    if n > 0:
        raw[0, :, 3] = 0.0
    if n > 1:
        raw[1, :, 3] = 0.01
        raw[1, -1, 3] = 0.0                                # (any density is opaque over the last sample's 1e10)
        raw[1, S // 2, 3] = np.nan
    if n > 2:
        raw[2, :, 3] = 0.0
        raw[2, b[kk + 1] - 1, 3] = 1e30
    if n > 3:
        raw[3, :, 3] = 0.5
        z[3, 0] = np.nan
    return raw, z, rays, kk


def device_q(backend, raw, z, rays):
    """The fp32 q of every sample as the BACKEND's compositing rounds it: the first weight of a two-sample ray (sample i
    and the depth behind it) is alpha_i times T = 1.0f, the only weight of a one-sample ray is the last sample's alpha with
    its 1e10 distance; q = fl32(fl32(1 - alpha) + 1e-10f).  So the transcription multiplies the very factors the kernel
    multiplies, and what remains is the order of an fp64 product."""
    n, S = z.shape
    alpha = np.zeros((n, S), np.float32)
    if n == 0:
        return alpha
    if S > 1:
        pair_raw = np.zeros((n, S - 1, 2, 4), np.float32)
        pair_raw[:, :, 0, 3] = raw[:, :-1, 3]
        pair_z = np.stack([z[:, :-1], z[:, 1:]], 2)
        pair_rays = np.repeat(rays, S - 1, 0)
        w = backend.weights(pair_raw.reshape(-1, 2, 4), pair_z.reshape(-1, 2), pair_rays)
        alpha[:, :-1] = w[:, 0].reshape(n, S - 1)
    last_raw = np.zeros((n, 1, 4), np.float32)
    last_raw[:, 0, 3] = raw[:, -1, 3]
    alpha[:, -1] = backend.weights(last_raw, np.ascontiguousarray(z[:, -1:]), rays)[:, 0]
    return REF.q_of_alpha(alpha)


def check_transmittance(backend, n, S):
    for K in SEGMENTS:
        if K > S:
            continue
        raw, z, rays, kk = transmittance_inputs(n, S, K)
        q = device_q(backend, raw, z, rays)
        b = REF.bounds(S, K)
        T = np.full(n, np.nan, np.float64)
        alive = np.full(n, SENTINEL, np.int32)
        stop = np.full(n, SENTINEL, np.int32)
        T_ref = T.copy()
        for k in range(K):
            first, length = b[k], b[k + 1] - b[k]
            runs = [backend.transmittance(raw, z, rays, S, first, length, k, K, KEPS, T, alive, stop) for _ in range(2)]
            assert all(a.tobytes() == c.tobytes() for a, c in zip(runs[0], runs[1]))
            T_new, alive_new, stop_new = runs[0]
            # T: the fp64 product of the device's own fp32 factors, following the kernel's own alive flags
            T_ref, _, _ = REF.transmittance(q, first, length, k, K, KEPS, T_ref, alive, stop)
            both_nan = np.isnan(T_new) & np.isnan(T_ref)
            err = np.abs(T_new - T_ref) / np.maximum(np.abs(T_ref), 1e-300)
            assert (both_nan | (err <= 1e-12)).all(), (n, S, K, k, float(np.nanmax(err)))
            # the decisions: exactly what follows from the kernel's own T
            want_alive, want_stop = REF.decide(T_new, k, K, KEPS, alive, stop)
            assert np.array_equal(alive_new, want_alive) and np.array_equal(stop_new, want_stop), (n, S, K, k)
            if k > 0:
                was = alive != 0
                assert T_new[~was].tobytes() == T[~was].tobytes(), "a stopped ray's transmittance moved"
            T, alive, stop = T_new, alive_new, stop_new
            T_ref = np.where(np.isnan(T_ref), T_ref, T)       # the next segment starts from the kernel's value
            if n > 2 and k == kk:
                assert stop[2] == kk + 1 and alive[2] == 0 and T[2] <= 1.0000001e-10, (stop[2], T[2])
            if n > 2 and k < kk:
                assert alive[2] == 1 and T[2] == 1.0
        if n > 0:
            assert alive[0] == 1 and stop[0] == K and T[0] == 1.0
        if n > 1:
            assert alive[1] == 1 and stop[1] == K and np.isfinite(T[1])
        if n > 3:
            assert alive[3] == 1 and stop[3] == K and np.isnan(T[3])
        if n >= 257:
            stops = set(stop.tolist())
            assert K in stops and len(stops) >= min(K, 3), stops


# ---- the render path -------------------------------------------------------------------------------------------------------
# The mixed case.  With the default density bias (0.5) most rays of synthetic.ray_batch end with acc = 1.0
# (tests/skip_empty_case.py), but through the LAST sample's 1e10 distance: in front of it the densities are of order one
# over a depth of one, and no ray's transmittance falls to 1e-2 (measured on the fp64 recomputation at alpha_bias -0.75,
# -0.25 and 0.25: 0 of 24 rays stop at eps 1e-2 or 1e-3, K = 2 or 4, seeds 1 .. 3).  FINE_ALPHA_BIAS = 4.0 and EPS = 1e-2
# were chosen on that recomputation (the interpreter's fp32 kernels, 24 rays, 16 + 8 samples and 16 + 0) so that between
# 20 % and 80 % of the rays stop before the last segment at K = 4: 16, 19, 17 of 24 for seeds 1, 2, 3 (16 + 8), 19, 19, 17
# (16 + 0); at K = 2: 6, 6, 4 and 7, 9, 5; with lindisp (seed 1): 5 and 6 at K = 4.  (At 3.0: 9 .. 14 at K = 4 but 1 .. 3 at
# K = 2; at 5.0: 21 .. 23 at K = 4.)  No ray of these seeds lies in the band eps (1 +- 1e-4) at any boundary.
FINE_ALPHA_BIAS = 4.0
EPS = 1e-2


def networks(device, fine_alpha_bias=FINE_ALPHA_BIAS, fine_density_bias=None):
    """skip_empty_case.networks' pair with the FINE network's (seed 1) alpha_bias chosen here; with N_importance = 0 the
    cases pass (fine, None): the network of the final stage is the one under test.  `fine_density_bias`: the density
    head's bias set outright."""
    from scnerf_amd import run_nerf_helpers as H
    nets = []
    for seed in (0, 1):
        p = synth.network_params(seed=seed, alpha_bias=SE.MIXED_ALPHA_BIAS if seed == 0 else fine_alpha_bias)
        if seed == 1 and fine_density_bias is not None:
            p["alpha_linear.bias"] = torch.full_like(p["alpha_linear.bias"], fine_density_bias)
        net = H.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(p)
        nets.append(net.to(device))
    return nets


def final_nets(nets, sf):
    return nets if sf > 0 else (nets[1], None)


node = OC.node
same_twelve = OC.same_twelve


def with_stop(ops, eps, K, fn):
    ops.inference_early_stop(eps, K)
    try:
        return fn()
    finally:
        ops.inference_early_stop("off")


def _dense(ops, pts, rays, spr, net, n, grid=None):
    """dense network on every sample with one view direction per sample (rows the grid calls dead zeroed) -> raw [n, spr, 4]"""
    flat = net.flat_parameters()
    wf, pl = ops.network_packs(net, flat, False, n)
    vd = rays[:, 8:11].repeat_interleave(spr, 0).contiguous()
    raw = ops.mlp_fwd(pts.view(-1, 3), vd, 1, wf, None, planes=pl)
    if grid is not None:
        dead = torch.from_numpy(OREF.dead_mask(pts.cpu().numpy(), *OC.grid_arrays(grid))).to(raw.device)
        raw = torch.where(dead[:, None], torch.zeros_like(raw), raw)
    return raw.view(n, spr, 4)


def final_stage_inputs(ops, rays, nets, sc, sf, white_bkgd=False, lindisp=False, randoms=None, grid=None):
    """the stages in front of the final network as stand-alone launches -> (coarse outputs or None, z [n, S], pts, z_std,
    z_samples, the final network)"""
    from scnerf_amd.functional import host_linspace
    r = randoms or {}
    n = rays.shape[0]
    z_c, pts_c = ops.coarse_sample(rays, host_linspace(sc, rays.device), r.get("t_rand"), lindisp)
    if sf == 0:
        return None, z_c, pts_c, None, None, nets[0]
    raw_c = _dense(ops, pts_c, rays, sc, nets[0], n, grid)
    rgb_c, disp_c, acc_c, w_c, depth_c = ops.composite_fwd(raw_c, z_c, rays, None, white_bkgd)
    u = r["u"] if "u" in r else host_linspace(sf, rays.device)
    z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, u)
    return (rgb_c, disp_c, acc_c, depth_c), z_f, pts_f, z_std, z_s, nets[1] if nets[1] is not None else nets[0]


def oracle(ops, rays, nets, sc, sf, K, stop_segment, white_bkgd=False, lindisp=False, randoms=None, grid=None):
    """-> (the twelve outputs had the network answered zero behind `stop_segment` [n] (and where the grid says dead), the
    dense raw of the final stage [n, S, 4] before the early-stop rows were zeroed, z [n, S])"""
    assert ops.inference_early_stop() is None and ops.inference_occupancy() is None
    with torch.no_grad():
        n = rays.shape[0]
        coarse, z, pts, z_std, z_s, net = final_stage_inputs(ops, rays, nets, sc, sf, white_bkgd, lindisp, randoms, grid)
        S = sc + sf
        dense = _dense(ops, pts, rays, S, net, n, grid)
        seg = torch.from_numpy(REF.segment_of(S, K)).to(rays.device)
        skipped = seg[None, :] >= stop_segment.to(torch.int64)[:, None]
        raw = torch.where(skipped[:, :, None], torch.zeros_like(dense), dense)
        rgb, disp, acc, _, depth = ops.composite_fwd(raw, z, rays, None, white_bkgd, want_weights=False)
        if sf == 0:
            out = (rgb, disp, acc, depth, raw, None, None, None, None, None, z, None)
        else:
            out = (rgb, disp, acc, depth, raw) + coarse + (z_std, z, z_s)
    return dict(zip(ALL_TWELVE, out)), dense, z, int(skipped.sum())


def check_decisions(rays, dense, z, K, eps, stop_segment):
    """the call's stop decisions against the independent fp64 recomputation from the dense raw: equal on every ray whose
    fp64 T lies outside eps (1 +- 1e-4) at every boundary; at most 1 % of the rays excused.  -> (fp64 decisions, band)"""
    norm = np.linalg.norm(rays[:, 3:6].double().cpu().numpy(), axis=1)
    # (rows behind a ray's stop are the dense network's here: the recomputation must not see the zeros it is checking)
    T = REF.boundary_transmittance_fp64(dense[:, :, 3].cpu().numpy(), z.cpu().numpy(), norm, K)
    want = REF.stop_segment_fp64(T, eps)
    band = REF.in_band(T, eps)
    got = stop_segment.cpu().numpy()
    assert band.mean() <= 0.01, band.mean()
    assert np.array_equal(got[~band], want[~band]), np.flatnonzero((got != want) & ~band)
    return want, band


def stopped_case(ops, device, nets, n, sc, sf, K, eps=EPS, white_bkgd=False, lindisp=False, randoms=None, seed=1, what="",
                 mixed=True):
    """synthetic.ray_batch(n, seed): the call under the switch equals the oracle in all twelve outputs; the decisions equal
    the fp64 recomputation; 0 < stopped < n (`mixed`); the bound against the switch-off call; early_stop_stats() reports
    this call's counts"""
    rays = synth.ray_batch(n, seed=seed, lindisp=lindisp).to(device)
    nets = final_nets(nets, sf)
    S = sc + sf
    off = node(rays, nets, sc, sf, white_bkgd, lindisp, randoms)
    ops.early_stop_stats(reset=True)
    got = with_stop(ops, eps, K, lambda: node(rays, nets, sc, sf, white_bkgd, lindisp, randoms))
    stats = ops.early_stop_stats(reset=True)
    stop_segment = ops.early_stop_last().clone()
    assert stop_segment.shape == (n,) and stop_segment.dtype == torch.int32
    want, dense, z, n_skipped = oracle(ops, rays, nets, sc, sf, K, stop_segment, white_bkgd, lindisp, randoms)
    same_twelve(got, want, what)
    fp64_stop, band = check_decisions(rays, dense, z, K, eps, stop_segment)
    stopped = int((stop_segment < K).sum())
    if mixed:
        assert 0 < stopped < n, (stopped, n)
    assert stats == {"samples": n * S, "skipped": n_skipped, "rays": n, "stopped": stopped}, (stats, n_skipped, stopped)
    # the bound: the skipped weights sum to at most T <= eps, colours lie in [0, 1]; S 2^-23 for two fp32 sums of S terms <= 1
    bound = eps + S * 2.0 ** -23
    for k in ("rgb_map", "acc_map"):
        d = float((got[k].double() - off[k].double()).abs().max())
        assert d <= bound, (what, k, d, bound)
    if sf > 0:
        for k in ("rgb0", "disp0", "acc0", "depth0", "z_std", "z_vals", "z_samples"):
            SE.same_bits(got[k], off[k], what + "untouched: " + k)
    return {"stopped": stopped, "band": int(band.sum()), "fp64_stopped": int((fp64_stop < K).sum()), "skipped": n_skipped}


def nothing_stops_case(ops, device, nets, n, sc, sf, K, what=""):
    """eps so small that no ray stops: the twelve outputs are the switch-off call's bits.  (The default networks' rays reach
    T = 0 in fp64 -- q is at least 1e-10 per sample, and 1e-10 ** 40 underflows --, so the case takes a fine density head at
    -50: sigma = 0, T = 1 on every ray.)"""
    rays = synth.ray_batch(n, seed=1).to(device)
    nets = final_nets(nets, sf)
    off = node(rays, nets, sc, sf)
    ops.early_stop_stats(reset=True)
    on = with_stop(ops, 1e-300, K, lambda: node(rays, nets, sc, sf))
    assert ops.early_stop_stats(reset=True) == {"samples": n * (sc + sf), "skipped": 0, "rays": n, "stopped": 0}
    assert (ops.early_stop_last() == K).all()
    same_twelve(on, off, what)


def all_stop_case(ops, device, nets, n, sc, sf, K, monkeypatch):
    """every ray opaque behind segment 0 (a fine density head at +200): the later passes launch no network"""
    rays = synth.ray_batch(n, seed=1).to(device)
    nets = final_nets(nets, sf)
    S = sc + sf
    launched = []
    real = ops.mlp_fwd
    monkeypatch.setattr(ops, "mlp_fwd", lambda *a, **k: (launched.append(a[0].numel() // 3), real(*a, **k))[1])
    ops.early_stop_stats(reset=True)
    got = with_stop(ops, 1e-3, K, lambda: node(rays, nets, sc, sf))
    monkeypatch.setattr(ops, "mlp_fwd", real)
    b = REF.bounds(S, K)
    # (the coarse pass of a two-stage call -- unless it is the one-launch coarse stage --, then segment 0 alone)
    coarse_pass = [n * sc] if (sf > 0 and sc != ops.COARSE_STAGE_SAMPLES) else []
    assert launched == coarse_pass + [n * b[1]], launched
    assert ops.early_stop_stats(reset=True) == {"samples": n * S, "skipped": n * (S - b[1]), "rays": n, "stopped": n}
    assert (ops.early_stop_last() == 1).all()
    assert (got["raw"][:, b[1]:] == 0).all() and (got["raw"][:, :b[1], 3] > 0).all()
    assert float((got["acc_map"] - 1).abs().max()) <= 1e-3 + S * 2.0 ** -23


def with_skip_empty_case(ops, device, nets, n, sc, sf, K, eps=EPS):
    """with inference_skip_empty(tau): ray compaction first, then the segments on the live rays -- a live ray's outputs are
    those of the early-stop call on the live rays alone, a skipped ray's the coarse stage's"""
    rays = synth.ray_batch(n, seed=1).to(device)
    off = node(rays, nets, sc, sf)
    tau, live, n_live = SE.median_threshold(off, n)
    sub = with_stop(ops, eps, K, lambda: node(rays[live].contiguous(), nets, sc, sf))
    sub_stop = ops.early_stop_last().clone()
    ops.inference_skip_empty(tau)
    ops.early_stop_stats(reset=True)
    try:
        got = with_stop(ops, eps, K, lambda: node(rays, nets, sc, sf))
    finally:
        ops.inference_skip_empty("off")
    stats = ops.early_stop_stats(reset=True)
    assert stats["rays"] == n_live and stats["samples"] == n_live * (sc + sf) and stats["stopped"] == int((sub_stop < K).sum())
    assert torch.equal(ops.early_stop_last(), sub_stop)
    dead = ~live
    for k in ALL_TWELVE:
        SE.same_bits(got[k][live], sub[k], "live rays: " + k)
    for k, k0 in (("rgb_map", "rgb0"), ("disp_map", "disp0"), ("acc_map", "acc0"), ("depth_map", "depth0")):
        SE.same_bits(got[k][dead], off[k0][dead], "skipped rays: " + k)
    assert (got["raw"][dead] == 0).all()
    return stats


def with_grid_case(ops, device, nets, n, sc, sf, K, eps=EPS, skip_empty=False):
    """with an occupancy grid: a sample runs iff the grid calls it live AND its ray is alive -- against the oracle with both
    maskings (both stages under the grid, the final stage's rows behind the stop zeroed as well).  `skip_empty`: all three
    switches together, on the rays the grid-on coarse stage leaves live."""
    rays = synth.ray_batch(n, seed=1).to(device)
    grid = OC.hand_grid(OC.mixed_mask(), device)
    live = torch.ones(n, dtype=torch.bool, device=device)
    tau = None
    if skip_empty:
        with torch.no_grad():
            acc_c = OC.coarse_oracle(ops, rays, nets, sc, grid)["out"][2]
        tau = float(acc_c.median())
        live = SE.live_mask(acc_c, tau)
        assert 0.0 <= tau < 1.0 and 0.25 * n <= int(live.sum()) <= 0.75 * n, (tau, int(live.sum()))
        ops.inference_skip_empty(tau)
    ops.early_stop_stats(reset=True)
    ops.occupancy_stats(reset=True)
    try:
        got = OC.with_grid(ops, grid, lambda: with_stop(ops, eps, K, lambda: node(rays, nets, sc, sf)))
    finally:
        ops.inference_skip_empty("off")
    stats = ops.early_stop_stats(reset=True)
    stop_segment = ops.early_stop_last().clone()
    rays_l = rays[live].contiguous()
    nl = rays_l.shape[0]
    assert stop_segment.shape == (nl,)
    # the oracle on the live rays: the coarse stage of a ray does not depend on its neighbours
    want, dense, z, n_skipped = oracle(ops, rays_l, nets, sc, sf, K, stop_segment, grid=grid)
    for k in ALL_TWELVE:
        SE.same_bits(got[k][live], want[k], "grid + stop: " + k)
    stopped = int((stop_segment < K).sum())
    assert 0 < stopped < nl, (stopped, nl)
    # skipped: behind the stop or dead by the grid (the oracle's dense raw has the grid's zero rows already)
    pts_dead = (want["raw"] == 0).all(2)
    assert stats == {"samples": nl * (sc + sf), "skipped": int(pts_dead.sum()), "rays": nl, "stopped": stopped}, stats
    assert int(pts_dead.sum()) > n_skipped, "the grid skipped nothing in front of the stops"
    # the decisions follow the grid-masked densities
    check_decisions(rays_l, dense, z, K, eps, stop_segment)
    # the occupancy grid's own compaction ran the coarse stage alone
    assert ops.occupancy_stats(reset=True)["samples"] == n * sc
    return stats


def noise_case(ops, device, nets, n, sc, sf, K):
    """a call with density noise does not notice the switch"""
    rays = synth.ray_batch(n, seed=1).to(device)
    rnd = {k: v.to(device) for k, v in synth.render_randoms(n, sc, sf, seed=3).items()}
    noise = {"noise_c": rnd["noise_c"], "noise_f": rnd["noise_f"]}
    off = node(rays, nets, sc, sf, noise=noise)
    ops.early_stop_stats(reset=True)
    on = with_stop(ops, EPS, K, lambda: node(rays, nets, sc, sf, noise=noise))
    assert ops.early_stop_stats(reset=True) == {"samples": 0, "skipped": 0, "rays": 0, "stopped": 0}
    same_twelve(on, off)


def tracking_case(ops, device, nets, n, sc, sf, K):
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
    ops.early_stop_stats(reset=True)
    b = with_stop(ops, EPS, K, step)
    assert ops.early_stop_stats(reset=True) == {"samples": 0, "skipped": 0, "rays": 0, "stopped": 0}
    for k in a[0]:
        SE.same_bits(a[0][k], b[0][k], k)
    SE.same_bits(a[1], b[1], "d rays")
    assert len(a[2]) == len(b[2]) and any(float(g.abs().max()) > 0 for g in a[2])
    for i, (ga, gb) in enumerate(zip(a[2], b[2])):
        SE.same_bits(ga, gb, "gradient of parameter %d" % i)


def nerfpp_case(ops, device, n=50, s_fg=34, s_bg=34):
    """the NeRF++ node under torch.no_grad() does not notice the switch: its eight outputs, the stats"""
    import types
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet
    args = types.SimpleNamespace(max_freq_log2=10, max_freq_log2_viewdirs=4, netdepth=8, netwidth=256, use_viewdirs=True)
    net = NerfNet(args)
    net.load_state_dict(synth.nerfpp_params(778))
    net = net.to(device)
    g = torch.Generator().manual_seed(5)
    o = (torch.randn(n, 3, generator=g) * 0.25).to(device)
    d = (torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 1.3).to(device)
    frac = torch.sort(torch.rand(n, s_fg, generator=g), -1)[0].to(device)
    bg_z = torch.sort(torch.rand(n, s_bg, generator=g), -1)[0].to(device)
    with torch.no_grad():
        far = TR.intersect_sphere(o, d)
        fg_z = 1e-4 + frac * (far - 1e-4)[:, None]
        off = net(o, d, far, fg_z, bg_z)
        ops.early_stop_stats(reset=True)
        on = with_stop(ops, EPS, 4, lambda: net(o, d, far, fg_z, bg_z))
    assert ops.early_stop_stats(reset=True) == {"samples": 0, "skipped": 0, "rays": 0, "stopped": 0}
    assert len(off) == 8 and off.keys() == on.keys()
    for k in off:
        SE.same_bits(on[k], off[k], "NeRF++ node: " + k)


def too_many_segments_case(ops, device, nets):
    """K > S is refused at call time: 4 samples per ray, 8 segments"""
    import pytest
    rays = synth.ray_batch(8, seed=1).to(device)
    with pytest.raises(ValueError):
        with_stop(ops, EPS, 8, lambda: node(rays, (nets[1], None), 4, 0))
    assert node(rays, (nets[1], None), 4, 0)["rgb_map"].shape == (8, 3)


def switch_validation(ops, monkeypatch):
    import pytest
    assert ops.inference_early_stop() is None
    bad = [(0.0, None), (-1e-3, None), (1.0, None), (2.0, None), (float("nan"), None), ("x", None), (True, None),
           (1e-3, 1), (1e-3, 9), (1e-3, 2.5), (1e-3, True), (1e-3, "4"), (None, 4)]
    for eps, K in bad:
        with pytest.raises(ValueError):
            ops.inference_early_stop(eps, K)
        assert ops.inference_early_stop() is None, (eps, K)
    assert ops.inference_early_stop(1e-3) == (1e-3, 4) and ops.inference_early_stop() == (1e-3, 4)
    assert ops.inference_early_stop(1e-4, 2) == (1e-4, 2)
    assert ops.inference_early_stop(0.5, 8) == (0.5, 8)
    with pytest.raises(ValueError):
        ops.inference_early_stop(1e-3, 9)
    assert ops.inference_early_stop() == (0.5, 8)                      # a refused value leaves the switch as it was
    assert ops.inference_early_stop("off") is None and ops.inference_early_stop() is None
    # the environment preset
    make = lambda: ops._EarlyStopSwitch("SCNERF_INFER_EARLY_STOP", "inference_early_stop")       # noqa: E731
    for preset, value in (("off", None), ("", None), ("1e-3", (1e-3, 4)), ("0.01:8", (0.01, 8)), ("1e-4:2", (1e-4, 2))):
        monkeypatch.setenv("SCNERF_INFER_EARLY_STOP", preset)
        assert make()() == value, preset
    for preset in ("on", "1e-3:", "1e-3:x", "1e-3:4:2", ":4", "0", "1", "nan", "1e-3:1", "1e-3:9", "1e-3,4"):
        monkeypatch.setenv("SCNERF_INFER_EARLY_STOP", preset)
        with pytest.raises(ValueError):
            make()
    monkeypatch.delenv("SCNERF_INFER_EARLY_STOP")
    assert make()() is None
    assert ops.early_stop_stats(reset=True).keys() == {"samples", "skipped", "rays", "stopped"}
    assert ops.early_stop_stats() == {"samples": 0, "skipped": 0, "rays": 0, "stopped": 0}
    with pytest.raises(ValueError):
        ops.segment_bounds(4, 8)
    assert ops.segment_bounds(5, 3) == [0, 1, 3, 5] and ops.segment_bounds(2, 2) == [0, 1, 2]
