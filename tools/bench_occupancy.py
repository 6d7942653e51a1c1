"""What ops.inference_occupancy costs and gains: the procedural scene (three blobs on black, synthetic.procedural_rays) at
image-sized batches through the trained golden networks (tests/golden/trained_nerf.npz), forward only, 64 + 128 samples,
chunks of 32 768 rays, the box [-1.5, 1.5)^3, grids baked at resolution 64 and 128 with probes 2, sigma_min 0, dilate 1.

Arms, each under inference_arithmetic "same" and "fast", run ALTERNATELY round after round (one round = every arm of both
arithmetics once), median and range over the rounds, ms per chunk:
    off                 every switch off
    grid64, grid128     the grid of that resolution
    grid128+skip        the grid and inference_skip_empty(1e-3)
    skip                inference_skip_empty(1e-3) alone
    other               the launches of a chunk that are not the network -- both samplers and both compositing launches on a
                        zero raw, through the stand-alone ops -- the model's t_other
Per grid arm: the share of samples skipped per stage (occupancy_stats; the coarse stage's from a coarse-only call) and the
model t = t_other + (live share) * t_network with t_network = t_off - t_other from the same run; `residual_ms` = measured
minus model is what the compaction, the expansion and the two host reads cost.  A gain counts only when the two arms'
ranges do not overlap (`ranges_apart`).  Also: bake time per grid, and on one view the PSNR of every arm against the off
render and against the scene's own pixel colours (synthetic.procedural_targets), and the same for grids baked at sigma_min
in {0, 0.1, 1} x dilate in {0, 1} (resolution 128).
Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_skip_empty import networks, psnr  # noqa: E402

SC, SF = 64, 128
BOX = ((-1.5,) * 3, (1.5,) * 3)
TAU = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--res", type=int, default=362, help="pixels per image side (362^2 = four chunks of 32 768 rays)")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="off,grid64,grid128,grid128+skip,skip,other")
    ap.add_argument("--arithmetics", default="same,fast")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X"
    from scnerf_amd import create_nerf as cn, ops, render as R, run_nerf_helpers as h, synthetic as synth
    from scnerf_amd.functional import host_linspace
    from scnerf_amd.occupancy import OccupancyGrid

    nets = networks()
    query = cn.FusedNetworkQuery(h.get_embedder(10, 0)[0], h.get_embedder(4, 0)[0])
    rays = synth.procedural_rays(n_views=a.views, res=a.res).cuda()
    n = rays.shape[0]
    chunks = (n + a.chunk - 1) // a.chunk

    def bake(resolution, sigma_min=0.0, dilate=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = OccupancyGrid.bake(nets, BOX[0], BOX[1], resolution=resolution, probes=2, sigma_min=sigma_min, dilate=dilate)
        torch.cuda.synchronize()
        return g, 1e3 * (time.perf_counter() - t0)

    def render(n_importance=SF, batch=rays):
        with torch.no_grad():
            return R.batchify_rays(batch, a.chunk, network_fn=nets[0], network_query_fn=query, N_samples=SC, perturb=0.0,
                                   N_importance=n_importance, network_fine=nets[1], white_bkgd=False, raw_noise_std=0.0)

    def other(batch=rays):
        """the launches of every chunk that are not the network"""
        with torch.no_grad():
            for lo in range(0, batch.shape[0], a.chunk):
                r = batch[lo:lo + a.chunk].contiguous()
                m, dev = r.shape[0], r.device
                z_c, _ = ops.coarse_sample(r, host_linspace(SC, dev), None, False)
                _, _, _, w_c, _ = ops.composite_fwd(torch.zeros((m, SC, 4), device=dev), z_c, r, None, False)
                z_f = ops.fine_sample(r, z_c, w_c, host_linspace(SF, dev))[0]
                ops.composite_fwd(torch.zeros((m, SC + SF, 4), device=dev), z_f, r, None, False, want_weights=False)

    grids, bake_ms = {}, {}
    for res in (64, 128):
        bake(res)                                         # warm-up: the packs, the shapes
        grids[res], bake_ms[res] = bake(res)
    settings = {"off": (None, None), "grid64": (grids[64], None), "grid128": (grids[128], None),
                "grid128+skip": (grids[128], TAU), "skip": (None, TAU), "other": (None, None)}

    def switch(name):
        grid, tau = settings[name]
        ops.inference_occupancy("off" if grid is None else grid)
        ops.inference_skip_empty("off" if tau is None else tau)

    def timed(name):
        switch(name)
        ops.occupancy_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        other() if name == "other" else render()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ops.occupancy_stats(reset=True)
        switch("off")
        return 1e3 * dt / chunks, st

    arithmetics = a.arithmetics.split(",")
    arm_names = a.arms.split(",")
    saved = (ops.inference_arithmetic(), ops.inference_skip_empty(), ops.inference_occupancy())
    result = {"rays": n, "chunk": a.chunk, "chunks": chunks, "samples": [SC, SF], "rounds": a.rounds, "unit": "ms per chunk",
              "scene": "synthetic.procedural_rays(n_views=%d, res=%d), trained golden weights" % (a.views, a.res),
              "box": BOX, "bake": {"probes": 2, "sigma_min": 0.0, "dilate": 1,
                                   "ms": {str(r): bake_ms[r] for r in grids},
                                   "occupied_fraction": {str(r): grids[r].occupied_fraction() for r in grids}},
              "arms": {}}
    try:
        for ar in arithmetics:                            # warm-up: every shape the timed window uses
            ops.inference_arithmetic(ar)
            for name in arm_names:
                timed(name)
        times = {(ar, name): [] for ar in arithmetics for name in arm_names}
        stats = {}
        for _ in range(a.rounds):
            for ar in arithmetics:
                ops.inference_arithmetic(ar)
                for name in arm_names:
                    ms, st = timed(name)
                    times[(ar, name)].append(ms)
                    stats[(ar, name)] = st
        for ar in arithmetics:
            ops.inference_arithmetic(ar)
            out = {}
            for name in arm_names:
                t = times[(ar, name)]
                out[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
                st = stats[(ar, name)]
                if st["samples"]:
                    out[name]["skipped_share"] = st["skipped"] / st["samples"]
                    if settings[name][1] is None:         # per stage: the coarse stage's counts from a coarse-only call
                        switch(name)
                        ops.occupancy_stats(reset=True)
                        render(0)
                        c = ops.occupancy_stats(reset=True)
                        switch("off")
                        out[name]["skipped_share_coarse"] = c["skipped"] / c["samples"]
                        out[name]["skipped_share_fine"] = (st["skipped"] - c["skipped"]) / (st["samples"] - c["samples"])
            if "off" in out and "other" in out:
                t_off, t_other = out["off"]["median_ms"], out["other"]["median_ms"]
                t_net = t_off - t_other
                out["model"] = {"t_other_ms": t_other, "t_network_ms": t_net}
                for name in arm_names:
                    if name in ("off", "other"):
                        continue
                    o = out[name]
                    o["against_off_percent"] = 100.0 * (o["median_ms"] / t_off - 1.0)
                    o["ranges_apart"] = o["max_ms"] < out["off"]["min_ms"] or o["min_ms"] > out["off"]["max_ms"]
                    if "skipped_share" in o and settings[name][1] is None:
                        o["model_ms"] = t_other + (1.0 - o["skipped_share"]) * t_net
                        o["residual_ms"] = o["median_ms"] - o["model_ms"]
            result["arms"][ar] = out
        if not a.no_quality:
            ops.inference_arithmetic("same")
            view = rays[: a.res * a.res]
            target = torch.cat([synth.procedural_targets(view[lo:lo + 4096].cpu()) for lo in range(0, view.shape[0], 4096)])
            switch("off")
            ref = render(batch=view)["rgb_map"].cpu()
            quality = {"rays": int(view.shape[0]), "psnr_off_against_scene": psnr(ref, target), "arms": {}, "bakes": {}}

            def judge():
                ops.occupancy_stats(reset=True)
                got = render(batch=view)["rgb_map"].cpu()
                st = ops.occupancy_stats(reset=True)
                return {"skipped_share": st["skipped"] / st["samples"] if st["samples"] else 0.0,
                        "psnr_against_off": psnr(got, ref) if not torch.equal(got, ref) else None,
                        "psnr_against_scene": psnr(got, target)}
            for name in arm_names:
                if name not in ("off", "other"):
                    switch(name)
                    quality["arms"][name] = judge()
            switch("off")
            for sigma_min in (0.0, 0.1, 1.0):
                for dilate in (0, 1):
                    g, _ = bake(128, sigma_min, dilate)
                    ops.inference_occupancy(g)
                    q = judge()
                    q["occupied_fraction"] = g.occupied_fraction()
                    quality["bakes"]["sigma_min=%g dilate=%d" % (sigma_min, dilate)] = q
            result["quality"] = quality
    finally:
        ops.inference_arithmetic(saved[0])
        ops.inference_skip_empty("off" if saved[1] is None else saved[1])
        ops.inference_occupancy("off" if saved[2] is None else saved[2])
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
