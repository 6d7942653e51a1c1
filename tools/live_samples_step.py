"""The training step of the headline workload with the backward on the live samples (ops.live_samples) against the dense
backward, at several batch sizes: where does the compaction -- two small launches, the gathers and ONE host read per
backward -- break even?  Both settings alternate; a window is `--iters` steps between two device events.

    python tools/live_samples_step.py [--rays 256 512 1024 2048 4096] [--iters 30] [--rounds 3] [--out file.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_C, S_F = 64, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[256, 512, 1024, 2048, 4096])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scnerf_amd import ops, synthetic as synth
    from scnerf_amd.create_nerf import FusedNetworkQuery
    from scnerf_amd.render import render_rays
    from scnerf_amd.run_nerf_helpers import NeRF, get_embedder
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    nets = []
    for seed in (0, 1):
        net = NeRF(D=8, W=256, input_ch=63, input_ch_views=27, output_ch=5, skips=[4], use_viewdirs=True)
        net.load_state_dict(synth.network_params(seed=seed))
        net = net.to(dev)
        net.flat_parameters()
        nets.append(net)
    query = FusedNetworkQuery(get_embedder(10, 0)[0], get_embedder(4, 0)[0])
    say("training step (data rays, %d + %d samples, raw_noise_std = 1, the bench's loss): dense backward against the backward on "
        "the live samples; %d steps per window, %d rounds, medians" % (S_C, S_F, a.iters, a.rounds))
    for n in a.rays:
        rays = synth.ray_batch(n, seed=1).to(dev)
        target = synth.target_rgb(n, seed=2).to(dev)
        inv = 1.0 / (3 * n)

        def step():
            for net in nets:
                net.zero_grad(set_to_none=True)
            ret = render_rays(rays, nets[0], query, S_C, retraw=True, perturb=1.0, N_importance=S_F, network_fine=nets[1],
                              raw_noise_std=1.0)
            torch.autograd.backward([ret["rgb_map"], ret["rgb0"]], [(ret["rgb_map"].detach() - target) * (2 * inv),
                                                                    (ret["rgb0"].detach() - target) * (2 * inv)])

        def window(live):
            ops.live_samples(live, min_samples=1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters

        t = {False: [], True: []}
        for live in (False, True):
            window(live)                   # warm-up of both routes
        for _ in range(a.rounds):
            for live in (False, True):
                t[live].append(window(live))
        md, ml = (sorted(t[k])[len(t[k]) // 2] for k in (False, True))
        say("  %5d rays (coarse pass %7d samples, fine pass %7d): dense %.3f ms [%s]   live %.3f ms [%s]   %+.3f ms"
            % (n, n * S_C, n * (S_C + S_F), md, " ".join("%.3f" % v for v in t[False]), ml,
               " ".join("%.3f" % v for v in t[True]), ml - md))
    ops.live_samples(True, min_samples=ops.LIVE_MIN_SAMPLES)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
