"""What ops.inference_early_stop costs and gains: the procedural scene (three blobs on black, synthetic.procedural_rays) at
image-sized batches through the trained golden networks (tests/golden/trained_nerf.npz), forward only, 64 + 128 samples,
chunks of 32 768 rays -- tools/bench_occupancy.py's scene and chunks.

Arms, run ALTERNATELY round after round (one round = every arm once), median and range over the rounds, ms per chunk:
    off                     every switch off
    eps=E,K=k               inference_early_stop(E, k), E in {1e-3, 1e-4}, k in {2, 4, 8}
    nostop,K=k              inference_early_stop(1e-300, k): the machinery -- K compactions, expansions, K - 1 transmittance
                            launches and host reads, the network in K launches -- where (almost) no ray stops
    grid128                 inference_occupancy with a 128^3 grid baked over [-1.5, 1.5)^3 (probes 2, sigma_min 0, dilate 1)
    grid128+eps=1e-3,K=4    the grid and early stop together
Per arm: the share of the fine stage's samples that did not reach the network and the share of rays stopped
(early_stop_stats), the time against the off arm of the same run, and whether the two arms' ranges are apart -- a gain or a
loss counts only then.  On one view: the PSNR of every arm's rgb_map against the off render, and the largest change of a
channel.  Prints one JSON document and writes it to profiles/early_stop_bench.json (--out: elsewhere)."""
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
NOSTOP = 1e-300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--res", type=int, default=362, help="pixels per image side (362^2 = four chunks of 32 768 rays)")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X"
    from scnerf_amd import create_nerf as cn, ops, render as R, run_nerf_helpers as h, synthetic as synth
    from scnerf_amd.occupancy import OccupancyGrid

    nets = networks()
    query = cn.FusedNetworkQuery(h.get_embedder(10, 0)[0], h.get_embedder(4, 0)[0])
    rays = synth.procedural_rays(n_views=a.views, res=a.res).cuda()
    n = rays.shape[0]
    chunks = (n + a.chunk - 1) // a.chunk
    grid = OccupancyGrid.bake(nets, BOX[0], BOX[1], resolution=128, probes=2, sigma_min=0.0, dilate=1)

    settings = {"off": (None, None)}
    for eps in (1e-3, 1e-4):
        for K in (2, 4, 8):
            settings["eps=%g,K=%d" % (eps, K)] = ((eps, K), None)
    for K in (2, 4, 8):
        settings["nostop,K=%d" % K] = ((NOSTOP, K), None)
    settings["grid128"] = (None, grid)
    settings["grid128+eps=0.001,K=4"] = ((1e-3, 4), grid)
    arm_names = list(settings)

    def switch(name):
        stop, g = settings[name]
        ops.inference_early_stop(*(stop if stop is not None else ("off",)))
        ops.inference_occupancy("off" if g is None else g)

    def render(batch=rays):
        with torch.no_grad():
            return R.batchify_rays(batch, a.chunk, network_fn=nets[0], network_query_fn=query, N_samples=SC, perturb=0.0,
                                   N_importance=SF, network_fine=nets[1], white_bkgd=False, raw_noise_std=0.0)

    def timed(name):
        switch(name)
        ops.early_stop_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ops.early_stop_stats(reset=True)
        switch("off")
        return 1e3 * dt / chunks, st

    saved = (ops.inference_early_stop(), ops.inference_occupancy())
    result = {"rays": n, "chunk": a.chunk, "chunks": chunks, "samples": [SC, SF], "rounds": a.rounds, "unit": "ms per chunk",
              "scene": "synthetic.procedural_rays(n_views=%d, res=%d), trained golden weights" % (a.views, a.res),
              "arithmetic": [ops.mlp_arithmetic(), ops.inference_arithmetic()], "arms": {}}
    try:
        for name in arm_names:                            # warm-up: every shape the timed window uses
            timed(name)
        times = {name: [] for name in arm_names}
        stats = {}
        for _ in range(a.rounds):
            for name in arm_names:
                ms, st = timed(name)
                times[name].append(ms)
                stats[name] = st
        out = result["arms"]
        for name in arm_names:
            t = times[name]
            out[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs_ms": t}
            st = stats[name]
            if st["samples"]:
                out[name]["skipped_share"] = st["skipped"] / st["samples"]
                out[name]["stopped_share"] = st["stopped"] / st["rays"]
        off = out["off"]
        for name in arm_names:
            if name != "off":
                o = out[name]
                o["against_off_percent"] = 100.0 * (o["median_ms"] / off["median_ms"] - 1.0)
                o["ranges_apart"] = o["max_ms"] < off["min_ms"] or o["min_ms"] > off["max_ms"]
        if not a.no_quality:
            view = rays[: a.res * a.res]
            switch("off")
            ref = render(batch=view)["rgb_map"].cpu()
            quality = {"rays": int(view.shape[0]), "arms": {}}
            for name in arm_names:
                if name == "off":
                    continue
                switch(name)
                got = render(batch=view)["rgb_map"].cpu()
                quality["arms"][name] = {"psnr_against_off": psnr(got, ref) if not torch.equal(got, ref) else None,
                                         "max_abs_change": float((got - ref).abs().max())}
            switch("off")
            result["quality"] = quality
    finally:
        ops.inference_early_stop(*(saved[0] if saved[0] is not None else ("off",)))
        ops.inference_occupancy("off" if saved[1] is None else saved[1])
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
