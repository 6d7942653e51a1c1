"""autograd glue between PyTorch and the HIP kernels (no arithmetic happens here).

`RenderRaysFunction` is one differentiable node for the whole of `render_rays`
(/root/reference NeRF/render.py:186-300): stratified sampling -> coarse network -> compositing
-> inverse-CDF sampling + merge -> fine network -> compositing, with gradients to the ray batch
(origin, direction, view direction) and to every parameter of both networks.
`RawToOutputsFunction` exposes compositing on its own (raw2outputs, :302-355).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import mlp_layout as ML
from . import ops

Tensor = torch.Tensor


@dataclass
class RenderConfig:
    n_samples: int
    n_importance: int
    lindisp: bool
    white_bkgd: bool
    # torch.is_grad_enabled() where render_rays was CALLED: inside Function.forward grad mode is always off, and
    # ctx.needs_input_grad stays True for parameters that require grad under torch.no_grad() -- without this flag a
    # forward-only call (render_path) would run the training instantiation and store every activation
    track: bool = True


_host_cache = {}


def host_linspace(n: int, device) -> Tensor:
    """torch.linspace(0, 1, n) computed on the HOST (the reference path under test is the CPU one
    and ATen's CPU / GPU linspace kernels may differ in the last bit; `device="cpu"` is explicit because the reference
    script makes CUDA the default tensor type, run_nerf.py:1046), cached per device."""
    key = (n, str(device))
    if key not in _host_cache:
        _host_cache[key] = torch.linspace(0.0, 1.0, steps=n, dtype=torch.float32, device="cpu").to(device)
    return _host_cache[key]


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    return t.contiguous().float()


class RenderRaysFunction(torch.autograd.Function):
    """apply(ray_batch, cfg, t_rand, u, noise_c, noise_f, net_c, net_f, *params_c, *params_f)

    t_rand [N,S_c] / None (perturb == 0); u [N,S_f] / None (deterministic linspace);
    noise_c/f: already scaled density noise or None.  `net_c` / `net_f` are the NeRF modules
    (flat parameter storage); their parameters are also passed as inputs so autograd routes the
    gradients.  Returns (rgb_map, disp_map, acc_map, depth_map, raw, rgb0, disp0, acc0, depth0,
    z_std, z_vals, z_samples); the *0 / z_std / z_samples entries are None when S_f == 0."""

    @staticmethod
    def forward(ctx, ray_batch, cfg, t_rand, u, noise_c, noise_f, net_c, net_f, *params):
        # outputs the loss does not touch arrive in backward as None (it handles that), not as ten zero tensors
        ctx.set_materialize_grads(False)
        rays = _c(ray_batch)
        if rays.shape[1] < 11:
            raise NotImplementedError("the fused network needs view directions (ray_batch [N, 11])")
        n = rays.shape[0]
        dev = rays.device
        sc, sf = cfg.n_samples, cfg.n_importance
        train = cfg.track and any(ctx.needs_input_grad)
        viewdirs = rays[:, 8:11]

        net_c.require_standard()
        flat_c = net_c.flat_parameters()
        save_c = ops.save_workspace(n * sc, dev) if train else None
        # the packed fp32 tables + what the arithmetic in force (ops.mlp_arithmetic) needs besides them: the resident
        # kernels' streams, or nothing (the fused fp32-MFMA kernels).  Training packs per call (the weights change every
        # step); a forward-only call takes them from the network's version-keyed cache (ops.network_packs)
        wf_c, pl_c = ops.network_packs(net_c, flat_c, train, n)
        resident = isinstance(pl_c, ops.ResidentWeights)
        # (resident kernels, training: they leave the chunk maxima the fp16 weight-gradient GEMMs scale by)
        mx_c = ops.ChunkMaxima(n * sc, dev) if (train and resident) else None
        # the lean workspace (ops.lean_workspace): decided ONCE here -- the data gradients and the weight-gradient group of
        # this call follow the decision, whatever the switches say by then
        lean = ops.lean_decision(("render", "all"), mx_c)
        # (the resident kernels' scale guard, ops.resident_guard: None while it is off)
        # (one record buffer per call, every pass of both stages, forward and data gradients)
        # (forward-only with ops.inference_arithmetic("fast"): the packs say so, and such passes take no record)
        fast = resident and pl_c.fast
        guards = ops.guard_records(dev, [("coarse", n * sc)] + ([("fine", n * (sc + sf))] if sf > 0 else []), fast=fast) \
            if (resident and n > 0) else {}
        gd_c = guards.get("coarse")
        # forward-only with ops.inference_occupancy(grid): the network of both stages on the samples the grid does not call
        # empty.  Not with density noise: zero raw plus noise would paint fog into empty space
        grid = ops.inference_occupancy() if (not train and n > 0 and noise_c is None and noise_f is None) else None
        # forward-only with ops.inference_early_stop(eps, K): the network of the call's FINAL stage front to back in K depth
        # segments, the rays that have gone opaque left out of the later ones.  Under the same conditions as the grid
        stop = ops.inference_early_stop() if (not train and n > 0 and noise_c is None and noise_f is None) else None
        if grid is not None:
            grid.check(net_c, net_f)
            if grid.bits.device != dev:
                raise ValueError("the occupancy grid lives on %s, the rays on %s" % (grid.bits.device, dev))
        if grid is not None or (stop is not None and sf == 0):
            z_c, pts_c = ops.coarse_sample(rays, host_linspace(sc, dev), _c(t_rand), cfg.lindisp)
            # (with a fine stage behind it the coarse stage is never cut short: its weights feed the sampler)
            raw_c = RenderRaysFunction._stage_network(pts_c, viewdirs, sc, wf_c, pl_c, gd_c, grid,
                                                      stop + (z_c, rays) if (stop is not None and sf == 0) else None).view(n, sc, 4)
            rgb_c, disp_c, acc_c, w_c, depth_c = ops.composite_fwd(raw_c, z_c, rays, None, cfg.white_bkgd)
        elif sc == ops.COARSE_STAGE_SAMPLES and n > 0:
            # the whole coarse stage -- stratified depths, network, compositing -- is one launch
            z_c, pts_c, raw_c, rgb_c, disp_c, acc_c, w_c, depth_c = ops.coarse_stage_fwd(
                rays, host_linspace(sc, dev), _c(t_rand), cfg.lindisp, wf_c, save_c, _c(noise_c), cfg.white_bkgd,
                planes=pl_c, maxima=mx_c, guard=gd_c, lean=lean)
        else:
            z_c, pts_c = ops.coarse_sample(rays, host_linspace(sc, dev), _c(t_rand), cfg.lindisp)
            raw_c = ops.mlp_fwd(pts_c, viewdirs, sc, wf_c, save_c, planes=pl_c, maxima=mx_c, guard=gd_c, lean=lean).view(n, sc, 4)
            rgb_c, disp_c, acc_c, w_c, depth_c = ops.composite_fwd(raw_c, z_c, rays, _c(noise_c), cfg.white_bkgd)

        ctx.cfg, ctx.train, ctx.n = cfg, train, n
        ctx.net_c, ctx.net_f = net_c, net_f
        ctx.n_params_c = len(net_c.ordered_parameters())
        ctx.coarse = (z_c, pts_c, raw_c, _c(noise_c), save_c, mx_c)
        ctx.lean = lean
        # the backward on the live samples alone (ops.live_samples): decided here, per pass, from the arithmetic and the
        # pass's size -- never from whether the rays need a gradient
        ctx.live = {"coarse": ops.live_decision(n * sc, mx_c), "fine": False}
        # (the lean weight-gradient group reads three parameters of the pass's network: a snapshot, as the packed weights
        #  are -- an in-place update between forward and backward must not reach the backward)
        ctx.flat_c = flat_c.detach().clone() if lean else None
        ctx.flat_f = None
        ctx.pl_c = pl_c
        ctx.guards = guards
        ctx.rays = rays
        ctx.wb_c = ops.pack_weights(flat_c, "bwd") if train else None
        ctx.fine = None
        if sf == 0:
            out = (rgb_c, disp_c, acc_c, depth_c, raw_c, None, None, None, None, None, z_c, None)
            ctx.mark_non_differentiable(z_c)
            return out

        fine_net = net_f if net_f is not None else net_c
        u_dev = _c(u) if u is not None else host_linspace(sf, dev)
        tot = sc + sf
        fine_net.require_standard()
        flat_f = fine_net.flat_parameters()
        save_f = ops.save_workspace(n * tot, dev) if train else None
        wf_f, pl_f = (wf_c, pl_c) if fine_net is net_c else ops.network_packs(fine_net, flat_f, train, n)
        mx_f = ops.ChunkMaxima(n * tot, dev) if (train and resident) else None
        gd_f = guards.get("fine")
        if not train and sf > 0 and ops.inference_skip_empty() is not None and n > 0:
            # forward-only with ops.inference_skip_empty(tau): the fine stage on the rays the coarse stage found something on
            out = RenderRaysFunction._fine_stage_on_live_rays(
                ops.inference_skip_empty(), rays, z_c, w_c, u_dev, _c(noise_f), cfg.white_bkgd, wf_f, pl_f, gd_f,
                (rgb_c, disp_c, acc_c, depth_c), sc, sf, grid=grid, stop=stop)
            ctx.mark_non_differentiable(*out[5:])
            return out[:5] + (rgb_c, disp_c, acc_c, depth_c) + out[5:]
        # (with the guard on, and on the one-product arithmetic, the three launches: the same numbers as the fused stage)
        if grid is not None or stop is not None:
            z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, u_dev)
            raw_f = RenderRaysFunction._stage_network(pts_f, viewdirs, tot, wf_f, pl_f, gd_f, grid,
                                                      stop + (z_f, rays) if stop is not None else None).view(n, tot, 4)
            rgb_f, disp_f, acc_f, _, depth_f = ops.composite_fwd(raw_f, z_f, rays, None, cfg.white_bkgd, want_weights=False)
        elif ops.fused_fine_stage() and gd_f is None and not fast and resident and sc == ops.COARSE_STAGE_SAMPLES and sf in ops.FINE_STAGE_IMPORTANCE and n > 0:
            # the whole fine stage -- inverse-cdf sampler, merge, network, compositing -- as one launch (opt-in: measured
            # slower than the three launches below, ops.fused_fine_stage)
            z_f, pts_f, z_s, z_std, _, _, raw_f, rgb_f, disp_f, acc_f, depth_f, _ = ops.fine_stage_fwd(
                rays, z_c, w_c, u_dev, wf_f, save_f, _c(noise_f), cfg.white_bkgd, pl_f, maxima=mx_f, lean=lean)
        else:
            z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays, z_c, w_c, u_dev)
            raw_f = ops.mlp_fwd(pts_f, viewdirs, tot, wf_f, save_f, planes=pl_f, maxima=mx_f, guard=gd_f, lean=lean).view(n, tot, 4)
            rgb_f, disp_f, acc_f, _, depth_f = ops.composite_fwd(raw_f, z_f, rays, _c(noise_f), cfg.white_bkgd,
                                                                 want_weights=False)
        ctx.fine = (z_f, pts_f, raw_f, _c(noise_f), save_f, mx_f)
        ctx.live["fine"] = ops.live_decision(n * tot, mx_f)
        ctx.flat_f = (ctx.flat_c if fine_net is net_c else flat_f.detach().clone()) if lean else None
        ctx.pl_f = pl_f
        ctx.wb_f = (ctx.wb_c if fine_net is net_c else ops.pack_weights(flat_f, "bwd")) if train else None
        ctx.mark_non_differentiable(z_std, z_f, z_s)
        return (rgb_f, disp_f, acc_f, depth_f, raw_f, rgb_c, disp_c, acc_c, depth_c, z_std, z_f, z_s)

    @staticmethod
    def _stage_network(pts, viewdirs, samples_per_ray, wf, pl, gd, grid=None, stop=None):
        """The network of one stage of a forward-only call -> raw [P, 4].
        Neither switch: the dense pass.
        `grid` (ops.inference_occupancy): compaction of the samples the grid does not call dead (one host read: the count
        sizes the launch), the network on that list with one view direction per sample, expansion with zero rows.  All
        samples live goes the same way; none live launches no network.  The guard record stays the dense pass's: the
        compact list has no more blocks.
        `stop` = (eps, K, z, rays) (ops.inference_early_stop, the call's final stage): the same three steps per depth
        segment, front to back, on the samples whose ray is alive (and the grid calls live); behind every segment but the
        last the rays' transmittance decides who goes on.  The first pass without a grid knows its count; every other
        pass reads one.  Every pass takes a guard record of its own, so that none reads block flags another left behind."""
        if stop is None:
            if grid is None:
                return ops.mlp_fwd(pts, viewdirs, samples_per_ray, wf, None, planes=pl, guard=gd)
            _, slot_of, pts_l, vd_l, n_live = ops.occ_compact(pts, viewdirs, samples_per_ray, grid)
            raw_l = ops.mlp_fwd(pts_l, vd_l, 1, wf, None, planes=pl, guard=gd) if n_live > 0 else None
            return ops.occ_expand_raw(raw_l, slot_of, n_live)
        eps, K, z, rays = stop
        S = samples_per_ray
        n = z.shape[0]
        b = ops.segment_bounds(S, K)
        raw = torch.empty((n * S, 4), dtype=torch.float32, device=pts.device)
        state = ops.StopState(n, pts.device)
        ran, n_rays = 0, n
        for k in range(K):
            first, length = b[k], b[k + 1] - b[k]
            opening = k == 0
            _, slot_of, pts_l, vd_l, n_live, n_rays = ops.seg_compact(
                pts, viewdirs, S, first, length, None if opening else state.alive, grid, read=not (opening and grid is None))
            raw_l = None
            if n_live > 0:
                name = "%s/%d" % (gd.name, k) if gd is not None else None
                gd_k = ops.guard_records(pts.device, [(name, n_live)])[name] if gd is not None else None
                raw_l = ops.mlp_fwd(pts_l, vd_l, 1, wf, None, planes=pl, guard=gd_k)
            ops.seg_expand_raw(raw_l, slot_of, raw, S, first, length, n_live)
            ran += n_live
            if k < K - 1:
                ops.seg_transmittance(raw, z, rays, first, length, k, K, eps, state)
        ops.early_stop_count(n, S, ran, n_rays, state.stop_segment)
        return raw

    @staticmethod
    def _fine_stage_on_live_rays(tau, rays, z_c, w_c, u, noise_f, white_bkgd, wf_f, pl_f, gd_f, coarse, sc, sf, grid=None,
                                 stop=None):
        """The fine stage of a forward-only call under ops.inference_skip_empty(tau): compaction of the rays with
        acc0 > tau (one host read: the count sizes the launches), the three launches on that batch, expansion.
        -> (rgb_map, disp_map, acc_map, depth_map, raw, z_std, z_vals, z_samples) for every ray.  All rays live goes the same
        way; none live launches nothing but the expansion.  `grid` / `stop` = (eps, K): the network of the live rays as
        _stage_network runs it under ops.inference_occupancy / ops.inference_early_stop."""
        tot = sc + sf
        live_idx, slot_of, n_live = ops.ray_compact(coarse[2], tau)
        live = None
        if n_live > 0:
            rays_l, z_l, w_l = (ops.ray_rows_gather(t, live_idx, n_live) for t in (rays, z_c, w_c))
            u_l = ops.ray_rows_gather(u, live_idx, n_live) if u.dim() == 2 else u
            noise_l = ops.ray_rows_gather(noise_f, live_idx, n_live) if noise_f is not None else None
            z_f, pts_f, z_s, z_std, _, _ = ops.fine_sample(rays_l, z_l, w_l, u_l)
            raw_f = RenderRaysFunction._stage_network(pts_f, rays_l[:, 8:11], tot, wf_f, pl_f, gd_f, grid,
                                                      stop + (z_f, rays_l) if stop is not None else None)
            raw_f = raw_f.view(n_live, tot, 4)
            rgb_f, disp_f, acc_f, _, depth_f = ops.composite_fwd(raw_f, z_f, rays_l, noise_l, white_bkgd, want_weights=False)
            live = (rgb_f, disp_f, acc_f, depth_f, z_std, raw_f, z_f, z_s)
        rgb, disp, acc, depth, z_std, raw, z_vals, z_samples = ops.ray_expand(slot_of, n_live, live, coarse, tot, sf)
        return rgb, disp, acc, depth, raw, z_std, z_vals, z_samples

    @staticmethod
    def _stage_composite_bwd(stage, rays, white_bkgd, g_rgb, g_disp, g_acc, g_depth, g_raw, want, live):
        """The compositing's gradient of one stage -- it depends on the incoming gradients alone -- and, on the live route
        (ops.live_samples), the compaction of its samples.  Nothing waits here.  -> (d_raw, d_rd, compaction or None)"""
        z, _, raw, noise, _, _ = stage
        d_raw, d_rd = ops.composite_bwd(raw, z, rays, noise, white_bkgd, _c(g_rgb), _c(g_disp), _c(g_acc),
                                        _c(g_depth), _c(g_raw), want_d_rays_d=want)
        return d_raw, d_rd, ops.live_compact(d_raw) if live else None

    @staticmethod
    def _stage_dgrad(stage, first, rays, spr, wbk, d_rays, accumulate, planes=None, guard=None, lean=False, flat_params=None,
                     guard_fwd=None):
        """Data gradients of one stage (network, rays) behind _stage_composite_bwd (`first`); -> what its weight
        gradients need, None when no sample is live.
        d_rays None: the rays need no gradient -- neither the network's input gradient nor the ray reduction runs.
        lean / flat_params: the stage's forward ran lean (ops.lean_workspace) on the network with these parameters.
        With a compaction: the unchanged kernel on the live samples; its input gradient goes back to sample order, zero
        rows for the dead samples, and the dense ray reduction runs.  Under the scale guard (guard_fwd / guard: the
        pass's forward and data-gradient records) a pass whose forward tripped, or whose compact batch trips, takes the
        dense route: the exact-fp32 rerun of a tripped block reads the dense workspace."""
        z, pts, raw, noise, save, maxima = stage
        d_raw, d_rd, L = first
        want = d_rays is not None
        P = z.shape[0] * spr
        if L is not None and L.n > 0 and ops.live_guard_tripped(guard_fwd):
            L = None
        if L is not None and L.n > ops.LIVE_MAX_SHARE * P:
            L = None               # nearly every sample is live: the compaction would cost more than it saves
        if L is not None and L.n > 0:
            masks, pts_l, vd_l = ops.live_gather(L, save, pts, rays[:, 8:11], spr)
            maxima_l = ops.live_maxima(L, maxima)
            guard_l = ops.live_guard_record(guard, L.n) if guard is not None else None
            grads, d_pts, d_views = ops.mlp_bwd_live(L, masks, pts_l, vd_l, wbk, planes, maxima_l, input_grad=want, lean=lean,
                                                     guard=guard_l)
            if guard_l is not None and guard_l.rerun and ops.live_guard_tripped(guard_l):
                L = None
            else:
                if guard_l is not None:
                    ops.live_guard_keep(guard_l)
                maxima = maxima_l
                if want:
                    d_pts, d_views = ops.live_scatter_rows(L, d_pts), ops.live_scatter_rows(L, d_views)
        if L is None:
            grads, d_pts, d_views = ops.mlp_bwd(d_raw, pts, rays[:, 8:11], spr, wbk, save, planes=planes, maxima=maxima,
                                                input_grad=want, guard=guard, lean=lean)
        elif L.n == 0:
            grads = maxima = None
            d_pts, d_views = (torch.zeros((P, 3), dtype=torch.float32, device=rays.device) for _ in range(2)) if want else (None, None)
        if want:
            ops.ray_reduce(d_pts, d_views, z, d_rd, d_rays, accumulate)
        return save, grads, d_raw, P, maxima, lean, flat_params, L

    @staticmethod
    def _stage_wgrad(pending, into=None):
        """`into`: the network's attached flat .grad buffer -- the weight gradients are ADDED to it and
        None is returned (nothing for autograd to accumulate); otherwise a fresh flat gradient."""
        save, grads, d_raw, P, maxima, lean, flat_params, L = pending
        if L is not None:
            if L.n == 0:       # no live sample: the gradient is zero
                return None if into is not None else torch.zeros(ML.N_PARAMS, dtype=torch.float32, device=d_raw.device)
            out = ops.nerf_wgrad_live(L, save, grads, d_raw, maxima, flat_grad=into, accumulate=into is not None, lean=lean,
                                      flat_params=flat_params)
            return None if into is not None else out
        if into is not None:
            ops.nerf_wgrad(save, grads, d_raw, P, flat_grad=into, accumulate=True, maxima=maxima, lean=lean,
                           flat_params=flat_params)
            return None
        return ops.nerf_wgrad(save, grads, d_raw, P, maxima=maxima, lean=lean, flat_params=flat_params)

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_depth, g_raw, g_rgb0, g_disp0, g_acc0, g_depth0, *_unused):
        if not ctx.train:
            raise RuntimeError("render_rays was evaluated without gradient tracking")
        cfg, rays, n = ctx.cfg, ctx.rays, ctx.n
        sc, sf = cfg.n_samples, cfg.n_importance
        # rays that are data (no requires_grad) get no gradient: autograd would drop it
        d_rays = torch.zeros_like(rays) if ctx.needs_input_grad[0] else None
        fg_c = fg_f = None
        wrote = False
        # networks whose .grad tensors are views of one flat buffer take their weight gradients by direct
        # accumulation (what AccumulateGrad would do with 24 returned tensors, in one launch)
        n_pc = ctx.n_params_c
        need = ctx.needs_input_grad[8:]
        into_c = ctx.net_c.attached_flat_grad() if all(need[:n_pc]) else None
        into_f = into_c if ctx.net_f is None else (ctx.net_f.attached_flat_grad() if all(need[n_pc:]) else None)
        # Both stages' data gradients first, then both stages' weight gradients: the 256 x 256 weight-gradient
        # GEMMs run on the bf16 matrix pipe at a lower shader clock, and the kernel that follows them inherits
        # that clock for ~0.3 ms -- adjacent, the two passes cost one such recovery per step instead of two.
        # The live route (ops.live_samples; decided in forward, per pass): the compositing gradients of both stages first
        # -- they depend on the incoming gradients alone --, the compaction of both, ONE host read of both counts, then
        # per stage the data gradients on the live samples.
        pend_f = pend_c = first_f = first_c = None
        want = d_rays is not None
        if sf > 0:
            if any(g is not None for g in (g_rgb, g_disp, g_acc, g_depth, g_raw)):
                first_f = RenderRaysFunction._stage_composite_bwd(ctx.fine, rays, cfg.white_bkgd, g_rgb, g_disp, g_acc, g_depth,
                                                                  g_raw, want, ctx.live["fine"])
            coarse_g = (g_rgb0, g_disp0, g_acc0, g_depth0, None)
        else:
            coarse_g = (g_rgb, g_disp, g_acc, g_depth, g_raw)
        if any(g is not None for g in coarse_g):
            first_c = RenderRaysFunction._stage_composite_bwd(ctx.coarse, rays, cfg.white_bkgd, *coarse_g, want,
                                                              ctx.live["coarse"])
        compactions = [f[2] for f in (first_f, first_c) if f is not None and f[2] is not None]
        if compactions:
            ops.live_counts(*compactions)
        if first_f is not None:
            pend_f = RenderRaysFunction._stage_dgrad(ctx.fine, first_f, rays, sc + sf, ctx.wb_f, d_rays, wrote,
                                                     planes=ctx.pl_f, guard=ctx.guards.get("fine_bwd"), lean=ctx.lean,
                                                     flat_params=ctx.flat_f, guard_fwd=ctx.guards.get("fine"))
            wrote = True
        if first_c is not None:
            pend_c = RenderRaysFunction._stage_dgrad(ctx.coarse, first_c, rays, sc, ctx.wb_c, d_rays, wrote, planes=ctx.pl_c,
                                                     guard=ctx.guards.get("coarse_bwd"), lean=ctx.lean, flat_params=ctx.flat_c,
                                                     guard_fwd=ctx.guards.get("coarse"))
        if pend_f is not None:
            fg_f = RenderRaysFunction._stage_wgrad(pend_f, into=into_f)
        if pend_c is not None:
            fg_c = RenderRaysFunction._stage_wgrad(pend_c, into=into_c)
        if sf > 0 and ctx.net_f is None and fg_f is not None:
            # one network serves both stages (reference :279): its gradient is the sum
            fg_c = fg_f if fg_c is None else fg_c + fg_f
            fg_f = None

        def split(flat):
            return [None] * len(ML.PARAM_SHAPES) if flat is None else ML.layout(3).split(flat)

        grads = split(fg_c)
        if ctx.net_f is not None:
            grads += split(fg_f)
        ctx.coarse = ctx.fine = None       # release the activation workspaces
        return (d_rays, None, None, None, None, None, None, None, *grads)


class RawToOutputsFunction(torch.autograd.Function):
    """apply(raw, z_vals, rays_d, noise, white_bkgd) -> (rgb_map, disp_map, acc_map, weights, depth_map);
    differentiable in raw and rays_d (z_vals carry no gradient: see scnerf_composite_bwd)."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d, noise, white_bkgd):
        raw4 = _c(raw[..., :4])            # a 5th channel, if any, is never read (reference :327,338)
        z = _c(z_vals)
        n = z.shape[0]
        rays = torch.zeros((n, 8), dtype=torch.float32, device=z.device)
        rays[:, 3:6] = rays_d
        noise = _c(noise)
        rgb, disp, acc, w, depth = ops.composite_fwd(raw4, z, rays, noise, white_bkgd)
        ctx.save_for_backward(raw4, z, rays, noise if noise is not None else torch.empty(0, device=z.device))
        ctx.white_bkgd = white_bkgd
        ctx.raw_channels = raw.shape[-1]
        ctx.mark_non_differentiable(w)
        return rgb, disp, acc, w, depth

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, _g_w, g_depth):
        raw4, z, rays, noise = ctx.saved_tensors
        noise = noise if noise.numel() else None
        d_raw, d_rd = ops.composite_bwd(raw4, z, rays, noise, ctx.white_bkgd, _c(g_rgb), _c(g_disp),
                                        _c(g_acc), _c(g_depth), None)
        if ctx.raw_channels > 4:
            pad = torch.zeros(d_raw.shape[:-1] + (ctx.raw_channels - 4,), device=d_raw.device)
            d_raw = torch.cat([d_raw, pad], -1)
        return d_raw, None, d_rd, None, None
