"""What ops.inference_skip_empty costs and gains: the procedural scene (three blobs on black, synthetic.procedural_rays) at
image-sized batches through the trained golden networks (tests/golden/trained_nerf.npz), forward only, 64 + 128 samples,
chunks of 32 768 rays.

Arms, each under inference_arithmetic "same" and "fast", run ALTERNATELY round after round (one round = every arm of both
arithmetics once), median and range over the rounds:
    off            the switch off
    tau=0          the switch on with (nearly) nothing to skip where the scene covers the ray: the machinery's price shows
                   in `machinery_percent` once the skipped fraction is taken out by the model
    q25 q50 q75    tau = that quantile of the batch's own acc0 (of the arithmetic the arm runs in)
    off@live, tau=0@live
                   the same two on a batch of the same size made of the scene's covered rays alone (acc0 > 0.01, repeated):
                   nothing is skipped, so `machinery_percent_direct` = tau=0@live against off@live is the price of the
                   compaction, the gathers, the expansion and the host read
`coarse` (N_importance = 0: the coarse launch alone) gives the model's terms from the same run: t_coarse, and t_fine =
t_off - t_coarse; the model of an arm that skips the fraction f is t_coarse + (1 - f) t_fine, and `residual_ms` is measured
minus model, per chunk.  Quality: the render at tau in {1e-4, 1e-3, 1e-2} -- skipped fraction, PSNR against the switch-off
render and the PSNR of both against the scene's own pixel colours (synthetic.procedural_targets).
Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SC, SF = 64, 128
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def networks():
    from scnerf_amd import run_nerf_helpers as h
    from tests import trained_weights as TW
    nets = []
    for which in ("coarse", "fine"):
        m = h.NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        m.load_state_dict(TW.weights("trained", which=which))
        nets.append(m.cuda())
    return nets


def psnr(a, b):
    return float(-10.0 * torch.log10(torch.mean((a.double() - b.double()) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--res", type=int, default=362, help="pixels per image side (362^2 = four chunks of 32 768 rays)")
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default="off,tau=0,q25,q50,q75,coarse,off@live,tau=0@live")
    ap.add_argument("--arithmetics", default="same,fast")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X"
    from scnerf_amd import create_nerf as cn, ops, render as R, run_nerf_helpers as h, synthetic as synth

    nets = networks()
    query = cn.FusedNetworkQuery(h.get_embedder(10, 0)[0], h.get_embedder(4, 0)[0])
    rays = synth.procedural_rays(n_views=a.views, res=a.res).cuda()
    n = rays.shape[0]
    chunks = (n + a.chunk - 1) // a.chunk

    def render(n_importance=SF, batch=rays):
        with torch.no_grad():
            return R.batchify_rays(batch, a.chunk, network_fn=nets[0], network_query_fn=query, N_samples=SC, perturb=0.0,
                                   N_importance=n_importance, network_fine=nets[1], white_bkgd=False, raw_noise_std=0.0)

    covered = {}

    def timed(tau, name):
        n_importance = 0 if name == "coarse" else SF
        batch = covered["rays"] if name.endswith("@live") else rays
        ops.inference_skip_empty("off" if tau is None else tau)
        ops.skip_empty_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render(n_importance, batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ops.skip_empty_stats(reset=True)
        ops.inference_skip_empty("off")
        return 1e3 * dt / chunks, (st["skipped"] / st["rays"] if st["rays"] else 0.0)

    arithmetics = a.arithmetics.split(",")
    arm_names = a.arms.split(",")
    saved = (ops.inference_arithmetic(), ops.inference_skip_empty())
    result = {"rays": n, "chunk": a.chunk, "chunks": chunks, "samples": [SC, SF], "rounds": a.rounds, "unit": "ms per chunk",
              "scene": "synthetic.procedural_rays(n_views=%d, res=%d), trained golden weights" % (a.views, a.res), "arms": {}}
    try:
        taus = {}
        for ar in arithmetics:
            ops.inference_arithmetic(ar)
            ops.inference_skip_empty("off")
            acc0 = render()["acc0"].float().cpu().numpy()
            taus[ar] = {"off": None, "tau=0": 0.0, "coarse": None, "off@live": None, "tau=0@live": 0.0}
            if not covered:
                idx = torch.nonzero(torch.from_numpy(acc0) > 0.01).flatten()
                covered["rays"] = rays[idx[torch.arange(n) % idx.numel()].cuda()].contiguous()
            for q in (25, 50, 75):
                taus[ar]["q%d" % q] = min(float(np.float32(np.quantile(acc0, q / 100.0))), BELOW_ONE)
            for name in arm_names:                        # warm-up: every shape the timed window uses
                timed(taus[ar][name], name)
        times = {(ar, name): [] for ar in arithmetics for name in arm_names}
        skipped = {}
        for _ in range(a.rounds):
            for ar in arithmetics:
                ops.inference_arithmetic(ar)
                for name in arm_names:
                    ms, f = timed(taus[ar][name], name)
                    times[(ar, name)].append(ms)
                    skipped[(ar, name)] = f
        for ar in arithmetics:
            out = {}
            for name in arm_names:
                t = times[(ar, name)]
                out[name] = {"tau": taus[ar][name], "skipped_fraction": skipped[(ar, name)], "median_ms": statistics.median(t),
                             "min_ms": min(t), "max_ms": max(t)}
            if "off" in out and "coarse" in out:
                t_off, t_c = out["off"]["median_ms"], out["coarse"]["median_ms"]
                t_f = t_off - t_c
                out["model"] = {"t_coarse_ms": t_c, "t_fine_ms": t_f}
                for name in arm_names:
                    if name in ("off", "coarse") or name.endswith("@live"):
                        continue
                    model = t_c + (1.0 - out[name]["skipped_fraction"]) * t_f
                    out[name]["model_ms"] = model
                    out[name]["residual_ms"] = out[name]["median_ms"] - model
                    out[name]["against_off_percent"] = 100.0 * (out[name]["median_ms"] / t_off - 1.0)
                    out[name]["beats_off_by_more_than_both_ranges"] = (
                        t_off - out[name]["median_ms"] > (out["off"]["max_ms"] - out["off"]["min_ms"])
                        + (out[name]["max_ms"] - out[name]["min_ms"]))
                if "tau=0" in out:
                    out["tau=0"]["machinery_percent"] = 100.0 * out["tau=0"]["residual_ms"] / t_off
            if "off@live" in out and "tau=0@live" in out:
                out["tau=0@live"]["machinery_percent_direct"] = 100.0 * (out["tau=0@live"]["median_ms"] / out["off@live"]["median_ms"] - 1.0)
            result["arms"][ar] = out
        if not a.no_quality:
            ops.inference_arithmetic("same")
            view = rays[: a.res * a.res]
            target = torch.cat([synth.procedural_targets(view[lo:lo + 4096].cpu()) for lo in range(0, view.shape[0], 4096)])
            ops.inference_skip_empty("off")
            ref = render(batch=view)["rgb_map"].cpu()
            quality = {"rays": int(view.shape[0]), "psnr_off_against_scene": psnr(ref, target), "thresholds": {}}
            for tau in (1e-4, 1e-3, 1e-2):
                ops.inference_skip_empty(tau)
                ops.skip_empty_stats(reset=True)
                got = render(batch=view)["rgb_map"].cpu()
                st = ops.skip_empty_stats(reset=True)
                quality["thresholds"]["%g" % tau] = {"skipped_fraction": st["skipped"] / st["rays"],
                                                     "psnr_against_off": psnr(got, ref) if not torch.equal(got, ref) else None,
                                                     "psnr_against_scene": psnr(got, target)}
            result["quality"] = quality
    finally:
        ops.inference_arithmetic(saved[0])
        ops.inference_skip_empty("off" if saved[1] is None else saved[1])
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
