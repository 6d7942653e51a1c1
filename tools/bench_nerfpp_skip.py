"""What ops.inference_skip_background costs and gains: ONE render_single_image chunk of 32 768 synthetic NeRF++ rays
(synthetic.nerfpp_rays) through the two-level cascade at its usual 64 + 128 samples (level 0: 64 foreground + 64 background
samples per ray, level 1: 192 + 192), synthetic weights (synthetic.nerfpp_params), forward only, world_size 1.

Arms, each under inference_arithmetic "same" and "fast", run ALTERNATELY round after round (one round = every arm of both
arithmetics once; a timed window is --repeat renders behind one synchronise; after every change of arithmetic one untimed
render re-packs the weights), median and range over the rounds, profiler off, every shape warmed before the first timed round:
    off                    the switch off
    q0 q25 q50 q75 q100    eps = that quantile of the switch-off call's own bg_lambda over both levels (clamped below 1)
    bg_network             the background network alone: its two launches (n x 64 and n x 192 samples) on the rays' own points
A TIMING MODEL in the skipped share, not a quality claim about any scene: the synthetic weights are untrained.  The skipped
rays of each level are counted from the switch-off bg_lambda (the switch never changes bg_lambda); an arm's `share` is the
fraction of the background SAMPLES it skips, model_ms = t_off - share * t_bg_network, residual_ms = measured - model.
`overhead_q0_ms` = q0 against off: npp_fg_lambda, the compaction, the gathers and the host read with (nearly) nothing skipped.
Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time
import types
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASCADE = [64, 128]
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
QUANTILES = (0, 25, 50, 75, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256, help="height x width = the chunk: 32 768 rays")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeat", type=int, default=8, help="renders per timed window (one window: a few tenths of a second)")
    ap.add_argument("--arithmetics", default="same,fast")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X"
    from scnerf_amd import ops, synthetic as synth
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet

    n = a.height * a.width
    args = types.SimpleNamespace(max_freq_log2=10, max_freq_log2_viewdirs=4, netdepth=8, netwidth=256, use_viewdirs=True)
    nets = []
    for seed in (781, 782):
        net = NerfNet(args)
        net.load_state_dict(synth.nerfpp_params(seed))
        nets.append(net.cuda())
    models = OrderedDict(cascade_level=2, cascade_samples=CASCADE, net_0=nets[0], net_1=nets[1])
    o, d, near = (t.cuda() for t in synth.nerfpp_rays(n, seed=41))

    class Sampler:
        H, W = a.height, a.width

        def get_all(self, camera_model, camera_idx, sampler, rank):
            return OrderedDict(ray_o=o, ray_d=d, depth=None, rgb=None, mask=None, min_depth=near, img_name="x")

    def render():
        return TR.render_single_image(0, 1, models, Sampler(), n, None, camera_idx=None)

    level_samples = [CASCADE[0], CASCADE[0] + CASCADE[1]]
    g = torch.Generator().manual_seed(7)
    bg_pts = []
    for s in level_samples:                                     # unit directions + inverse radii: what the background network sees
        p = torch.nn.functional.normalize(torch.randn(n * s, 3, generator=g), dim=-1)
        bg_pts.append(torch.cat([p, torch.rand(n * s, 1, generator=g)], -1).contiguous().cuda())
    views = torch.nn.functional.normalize(d, dim=-1).contiguous()

    def bg_network():
        with torch.no_grad():
            for net, pts, s in zip(nets, bg_pts, level_samples):
                wf, pl = ops.network_packs(net.bg_net, net.bg_net.flat_parameters(), False, n, 4, remap=net.bg_net.pack_remap())
                ops.mlp_fwd(pts, views, s, wf, None, pd=4, planes=pl)

    def timed(name, eps):
        ops.inference_skip_background("off" if eps is None else eps)
        ops.skip_background_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            bg_network() if name == "bg_network" else render()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ops.skip_background_stats(reset=True)
        ops.inference_skip_background("off")
        return 1e3 * dt / a.repeat, st

    arithmetics = a.arithmetics.split(",")
    arm_names = ["off"] + ["q%d" % q for q in QUANTILES] + ["bg_network"]
    saved = (ops.inference_arithmetic(), ops.inference_skip_background())
    result = {"rays": n, "cascade_samples": CASCADE, "background_samples_per_ray": level_samples, "rounds": a.rounds,
              "renders_per_window": a.repeat, "unit": "ms per chunk (both cascade levels)", "scene": "synthetic.nerfpp_rays, synthetic.nerfpp_params (untrained)",
              "arms": {}}
    try:
        eps_of, share_of = {}, {}
        for ar in arithmetics:
            ops.inference_arithmetic(ar)
            ops.inference_skip_background("off")
            lam = [lvl["bg_lambda"].reshape(-1).float() for lvl in render()]
            both = torch.cat(lam).numpy()
            eps_of[ar] = {"off": None, "bg_network": None}
            share_of[ar] = {"off": 0.0, "bg_network": None}
            for q in QUANTILES:
                eps = min(float(np.float32(np.quantile(both, q / 100.0))), BELOW_ONE)
                eps_of[ar]["q%d" % q] = eps
                skipped = [int((x <= eps).sum()) for x in lam]
                share_of[ar]["q%d" % q] = sum(k * s for k, s in zip(skipped, level_samples)) / float(n * sum(level_samples))
            for name in arm_names:                                  # warm-up: every shape the timed window uses
                timed(name, eps_of[ar][name])
        times = {(ar, name): [] for ar in arithmetics for name in arm_names}
        stats = {}
        for _ in range(a.rounds):
            for ar in arithmetics:
                ops.inference_arithmetic(ar)
                render()                # (untimed: the networks' pack cache holds one arithmetic; the first call re-packs)
                for name in arm_names:
                    ms, st = timed(name, eps_of[ar][name])
                    times[(ar, name)].append(ms)
                    stats[(ar, name)] = st
        for ar in arithmetics:
            out = {}
            for name in arm_names:
                t = times[(ar, name)]
                st = stats[(ar, name)]
                out[name] = {"eps": eps_of[ar][name], "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
                if name.startswith("q"):
                    out[name]["skipped_rays_fraction"] = st["skipped"] / st["rays"] if st["rays"] else 0.0
                    out[name]["skipped_background_samples_share"] = share_of[ar][name]
            t_off, t_bg = out["off"]["median_ms"], out["bg_network"]["median_ms"]
            for q in QUANTILES:
                arm = out["q%d" % q]
                arm["model_ms"] = t_off - arm["skipped_background_samples_share"] * t_bg
                arm["residual_ms"] = arm["median_ms"] - arm["model_ms"]
                arm["against_off_percent"] = 100.0 * (arm["median_ms"] / t_off - 1.0)
            out["overhead_q0_ms"] = out["q0"]["median_ms"] - t_off
            out["overhead_q0_percent"] = 100.0 * (out["q0"]["median_ms"] / t_off - 1.0)
            result["arms"][ar] = out
    finally:
        ops.inference_arithmetic(saved[0])
        ops.inference_skip_background("off" if saved[1] is None else saved[1])
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
