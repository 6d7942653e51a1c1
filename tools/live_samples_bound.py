"""What would the backward pass gain if it ran on the live samples alone?  A bound, measured with the existing exports only.

A sample is dead when its d_raw row is all +-0 (noisy density <= 0: alpha = 0, so weights = 0).  Its dZ rows, its input
gradient and its term in every weight gradient are exact zeros.  This tool takes one training step of the headline
shape, catches what the step hands to ops.mlp_bwd and ops.nerf_wgrad, and times both calls twice: on the step's own
P samples, and on a batch of the P_live live samples built with torch indexing (d_raw rows, points, per-sample view
directions, every workspace section and the lane-native masks regathered into a workspace of P_live samples).  The two
settings alternate; each window is `--iters` back-to-back calls between two device events.

    python tools/live_samples_bound.py [--rays 4096] [--iters 40] [--rounds 3] [--out profiles/r10_live_samples.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scnerf_amd import mlp_layout as ML      # noqa: E402

S_C, S_F = 64, 128


def live_index(d_raw):
    """ascending indices of the samples with a non-zero word in their d_raw row, the sign bit ignored"""
    words = d_raw.reshape(-1, 4).view(torch.int32) & 0x7FFFFFFF
    return torch.nonzero((words != 0).any(dim=1)).reshape(-1)


def _pad_rows(rows, n):
    if rows.shape[0] == n:
        return rows
    pad = torch.zeros((n - rows.shape[0],) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    return torch.cat([rows, pad])


def gather_tiled(block, width, idx, pp_live):
    """tile-native section ([tile][width / 4][32 samples][4], mlp_layout.untile) -> the same layout over samples `idx`"""
    pp = block.numel() // width
    rows = block.view(pp // 32, width // 4, 32, 4).permute(0, 2, 1, 3).reshape(pp, width)[idx]
    rows = _pad_rows(rows, pp_live)
    return rows.view(pp_live // 32, 32, width // 4, 4).permute(0, 2, 1, 3).reshape(-1)


def gather_rows(block, width, idx, pp_live):
    return _pad_rows(block.view(-1, width)[idx], pp_live).reshape(-1)


def gather_masks(masks, idx, pp_live):
    """nine lane-native sections [section][tile][lane = 32 h + m][4 words]: sample 32 tile + m owns lanes m and 32 + m"""
    pp = masks.numel() // ML.MASK_WORDS_PER_SAMPLE
    rows = masks.view(9, pp // 32, 2, 32, 4).permute(0, 1, 3, 2, 4).reshape(9, pp, 8)[:, idx]
    if pp_live > rows.shape[1]:
        rows = torch.cat([rows, torch.zeros((9, pp_live - rows.shape[1], 8), dtype=rows.dtype, device=rows.device)], dim=1)
    return rows.view(9, pp_live // 32, 32, 2, 4).permute(0, 1, 3, 2, 4).reshape(-1)


def gather_save(save, P, idx):
    """the activation workspace of P samples -> one of len(idx) samples holding the rows of `idx`"""
    lay = ML.layout(3)
    off, total = ML.section_offsets(lay.save_sections, P)
    pp, pp_live = ML.padded_samples(P), ML.padded_samples(int(idx.numel()))
    parts = []
    for name, w in lay.save_sections:
        block = save[off[name]: off[name] + w * pp]
        parts.append((gather_tiled if name in ML.TILED_SECTIONS else gather_rows)(block, w, idx, pp_live))
    masks = save[total: total + ML.MASK_WORDS_PER_SAMPLE * pp].view(torch.int32)
    parts.append(gather_masks(masks, idx, pp_live).view(torch.float32))
    return torch.cat(parts)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scnerf_amd import ops, synthetic as synth
    from scnerf_amd.create_nerf import FusedNetworkQuery
    from scnerf_amd.render import render_rays
    from scnerf_amd.run_nerf_helpers import NeRF, get_embedder
    dev = torch.device("cuda:0")
    n = a.rays
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    nets = []
    for seed in (0, 1):
        net = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(synth.network_params(seed=seed))
        nets.append(net.to(dev))
    query = FusedNetworkQuery(get_embedder(10, 0)[0], get_embedder(4, 0)[0])
    rays = synth.ray_batch(n, seed=1).to(dev)
    target = synth.target_rgb(n, seed=2).to(dev)
    rnd = {k: v.to(dev) for k, v in synth.render_randoms(n, S_C, S_F, seed=3).items()}

    # ---- one step of the headline workload (data rays), catching what it hands to the two calls ----
    caught = {"bwd": [], "wgrad": []}
    real_bwd, real_wgrad = ops.mlp_bwd, ops.nerf_wgrad

    def spy_bwd(*args, **kw):
        caught["bwd"].append((args, kw))
        return real_bwd(*args, **kw)

    def spy_wgrad(*args, **kw):
        caught["wgrad"].append((args, kw))
        return real_wgrad(*args, **kw)

    ops.mlp_bwd, ops.nerf_wgrad = spy_bwd, spy_wgrad
    try:
        ret = render_rays(rays, nets[0], query, S_C, retraw=True, perturb=1.0, N_importance=S_F, network_fine=nets[1],
                          raw_noise_std=1.0, _randoms=rnd)
        inv = 1.0 / (3 * n)
        torch.autograd.backward([ret["rgb_map"], ret["rgb0"]], [(ret["rgb_map"].detach() - target) * (2 * inv),
                                                                (ret["rgb0"].detach() - target) * (2 * inv)])
    finally:
        ops.mlp_bwd, ops.nerf_wgrad = real_bwd, real_wgrad
    torch.cuda.synchronize()
    assert len(caught["bwd"]) == 2 and len(caught["wgrad"]) == 2, (len(caught["bwd"]), len(caught["wgrad"]))

    say("live-sample bound: %d rays x (%d + %d), raw_noise_std = 1, the bench's loss, data rays; mlp arithmetic %s, wgrad "
        "arithmetic %s" % (n, S_C, S_F, ops.mlp_arithmetic(), ops.wgrad_arithmetic()))
    say("each window: %d back-to-back calls between two device events; dense and live alternate, %d rounds" % (a.iters, a.rounds))
    total = {"dense": 0.0, "live": 0.0, "prop": 0.0}
    share_of = {}
    for (bargs, bkw), (wargs, wkw) in zip(caught["bwd"], caught["wgrad"]):
        d_raw, pts, viewdirs, spr, wbk, save = bargs
        P = int(wargs[3])
        stage = "fine" if spr == S_C + S_F else "coarse"
        lean, flat_params, mx = bkw["lean"], wkw["flat_params"], bkw["maxima"]
        assert wargs[0] is save and wargs[2] is d_raw and bkw["guard"] is None
        idx = live_index(d_raw)
        p_live = int(idx.numel())
        share_of[stage] = p_live / P
        # no 32-sample wave tile without a live sample?
        tiles_dead = int(((torch.bincount(idx // 32, minlength=(P + 31) // 32)) == 0).sum())
        d_raw_l = d_raw.reshape(P, 4)[idx].contiguous()
        pts_l = pts.reshape(P, 3)[idx].contiguous()
        vd_l = viewdirs[idx // spr].contiguous()
        save_l = gather_save(save, P, idx)
        mx_l = ops.ChunkMaxima(p_live, dev)
        mx_l.x[:] = mx.x.max(dim=1, keepdim=True).values        # an upper bound: all scale_for needs
        say()
        say("%s pass: P = %d, P_live = %d (live share %.4f), wave tiles without a live sample: %d of %d"
            % (stage, P, p_live, p_live / P, tiles_dead, (P + 31) // 32))

        def bwd(dense):
            if dense:
                return real_bwd(d_raw, pts, viewdirs, spr, wbk, save, planes=bkw["planes"], maxima=mx, input_grad=False, lean=lean)
            return real_bwd(d_raw_l, pts_l, vd_l, 1, wbk, save_l, planes=bkw["planes"], maxima=mx_l, input_grad=False, lean=lean)

        g_dense, g_live = bwd(True)[0], bwd(False)[0]

        def wgrad(dense):
            if dense:
                return real_wgrad(save, g_dense, d_raw, P, maxima=mx, lean=lean, flat_params=flat_params)
            return real_wgrad(save_l, g_live, d_raw_l, p_live, maxima=mx_l, lean=lean, flat_params=flat_params)

        # the live batch computes the same gradient (the figure only shows that the batch is a valid one)
        f_dense, f_live = wgrad(True), wgrad(False)
        say("  flat gradient, live batch against dense: max |diff| %.3e over max |dense| %.3e"
            % (float((f_dense - f_live).abs().max()), float(f_dense.abs().max())))
        for name, fn in (("mlp_bwd (data rays)", bwd), ("nerf_wgrad", wgrad)):
            for dense in (True, False):
                timed(lambda: fn(dense), 5)          # warm-up of both shapes
            t = {True: [], False: []}
            for _ in range(a.rounds):
                for dense in (True, False):
                    t[dense].append(timed(lambda: fn(dense), a.iters))
            md, ml = sorted(t[True])[len(t[True]) // 2], sorted(t[False])[len(t[False]) // 2]
            total["dense"] += md
            total["live"] += ml
            prop = md * (1 - p_live / P)
            total["prop"] += prop
            say("  %-20s dense %.3f ms [%s]   live %.3f ms [%s]   saved %.3f ms = %.0f %% of the proportional %.3f ms"
                % (name, md, " ".join("%.3f" % v for v in t[True]), ml, " ".join("%.3f" % v for v in t[False]),
                   md - ml, 100 * (md - ml) / prop, prop))
    say()
    saved = total["dense"] - total["live"]
    say("both passes, both calls: dense %.3f ms, live %.3f ms, saved %.3f ms = %.0f %% of the proportional %.3f ms"
        % (total["dense"], total["live"], saved, 100 * saved / total["prop"], total["prop"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
