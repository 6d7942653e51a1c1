"""What ops.inference_occupancy_nerfpp costs and gains: ONE render_single_image chunk of 32 768 synthetic NeRF++ rays
(synthetic.nerfpp_rays) through the two-level cascade at its usual 64 + 128 samples (level 0: 64 foreground + 64 background
samples per ray, level 1: 192 + 192), synthetic weights (synthetic.nerfpp_params), forward only, world_size 1.

Grids made BY HAND (OccupancyGrid.from_mask, R = 128, bound to no network): a cell is dead with probability 0, 25, 50, 75 or
100 % (a seeded draw per cell; 0: every cell set, 100: no cell set) over the box [-1.01, 1.01]^3, which holds every
foreground sample and every q of a background sample.  A TIMING MODEL in the dead share, not a quality claim about any scene:
the synthetic weights are untrained and the masks follow no density.  The dead SAMPLE shares reported are measured -- the
switch's own counts (ops.occupancy_nerfpp_stats) --, not the cell shares.

Arms, run ALTERNATELY round after round (one round = every arm once; a timed window is --repeat renders behind one
synchronise), median and range over the rounds, profiler off, every shape warmed before the first timed round:
    off                          the switch off
    fg0 .. fg100                 a foreground grid alone at that dead share of cells
    bg0 .. bg100                 a background grid alone
    both0 .. both100             both grids
`price_of_the_switch`: both0 against off -- two compactions, two expansions, two host reads per level, nothing dead.
Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time
import types
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASCADE = [64, 128]
SHARES = (0, 25, 50, 75, 100)
BOX = ((-1.01,) * 3, (1.01,) * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256, help="height x width = the chunk: 32 768 rays")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=4, help="renders per timed window")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--arithmetics", default="same", help="comma-separated: same, fast")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the MI355X"
    from scnerf_amd import ops, synthetic as synth
    from scnerf_amd.nerfplusplus import ddp_train_nerf as TR
    from scnerf_amd.nerfplusplus.ddp_model import NerfNet
    from scnerf_amd.occupancy import OccupancyGrid

    n, R = a.height * a.width, a.resolution
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

    def grid(space, share, seed):
        g = torch.Generator().manual_seed(seed)
        mask = torch.rand((R, R, R), generator=g) >= share / 100.0             # (share 0: every cell set; 100: none)
        return OccupancyGrid.from_mask(mask, BOX[0], BOX[1], space=space).to("cuda")

    arms = OrderedDict(off=None)
    for s in SHARES:
        fg, bg = grid("euclidean", s, 100 + s), grid("inverted_sphere", s, 200 + s)
        arms["fg%d" % s], arms["bg%d" % s], arms["both%d" % s] = (fg, None), (None, bg), (fg, bg)

    def timed(name):
        ops.inference_occupancy_nerfpp("off") if arms[name] is None else ops.inference_occupancy_nerfpp(*arms[name])
        ops.occupancy_nerfpp_stats(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.repeat):
            render()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ops.occupancy_nerfpp_stats(reset=True)
        ops.inference_occupancy_nerfpp("off")
        return 1e3 * dt / a.repeat, st

    arithmetics = a.arithmetics.split(",")
    saved = ops.inference_arithmetic()
    per_ray = [CASCADE[0], CASCADE[0] + CASCADE[1]]
    result = {"rays": n, "cascade_samples": CASCADE, "samples_per_ray_and_network": per_ray, "resolution": R, "box": BOX,
              "rounds": a.rounds, "renders_per_window": a.repeat, "unit": "ms per chunk (both cascade levels)",
              "scene": "synthetic.nerfpp_rays, synthetic.nerfpp_params (untrained); hand-made random-cell grids: a timing model",
              "not_measured": "image quality on real NeRF++ scenes (no dataset here)", "arms": {}}
    try:
        for ar in arithmetics:
            ops.inference_arithmetic(ar)
            for name in arms:                                       # warm-up: every shape the timed windows use
                timed(name)
        times = {(ar, name): [] for ar in arithmetics for name in arms}
        stats = {}
        for _ in range(a.rounds):
            for ar in arithmetics:
                ops.inference_arithmetic(ar)
                render()                # (untimed: the networks' pack cache holds one arithmetic; the first call re-packs)
                for name in arms:
                    ms, st = timed(name)
                    times[(ar, name)].append(ms)
                    stats[(ar, name)] = st
        for ar in arithmetics:
            out = OrderedDict()
            t_off = statistics.median(times[(ar, "off")])
            for name in arms:
                t, st = times[(ar, name)], stats[(ar, name)]
                arm = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                       "against_off_percent": 100.0 * (statistics.median(t) / t_off - 1.0)}
                for which in ("fg", "bg"):
                    if st[which + "_samples"]:
                        arm["dead_%s_sample_share" % which] = st[which + "_skipped"] / float(st[which + "_samples"])
                out[name] = arm
            out["price_of_the_switch_ms"] = out["both0"]["median_ms"] - t_off
            out["price_of_the_switch_percent"] = out["both0"]["against_off_percent"]
            result["arms"][ar] = out
    finally:
        ops.inference_arithmetic(saved)
        ops.inference_occupancy_nerfpp("off")
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
