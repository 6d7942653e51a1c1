"""Training batches on the MI355X: scnerf_amd.batching.RayBatcher.next() (one HIP launch, no host wait) against the host
path of the reference's train() as tests/run_nerf_loop.py::Loop.ray_batch mirrors it, re-stated here as the comparison arm:

  one image   (NeRF/run_nerf.py:409-478)  a device meshgrid of all H W pixels, np.random.choice(H W, [N_rand], replace=False)
                                          on the host, the fancy index with it, .long(), the two gathers of target_s
  all images  (:368-407)                  slices of a host permutation, % and // on the host, np.stack, two
                                          torch.from_numpy(...).cuda() copies, images[index_train, h_list, w_list] with host
                                          index arrays; np.random.shuffle of all n H W indices at each epoch end, timed once and
                                          reported per step as shuffle time / steps per epoch

    python tools/bench_batching.py [--out profiles/batching_bench.json] [--quick]

378 x 504 x 20 (LLFF at factor 8) and 800 x 800 x 100 (Blender), fp32 image stacks on the device, N_rand 1024 and 4096, both
modes.  Per point and arm: wall-clock per step = a host clock around BLOCK steps that end in a device synchronise, REPEATS
blocks per arm, the arms alternating, after warm-up; the median block with its spread.  For the HIP arm also the host time of
the enqueue alone (no synchronise inside the window) and the time between two device events around one next().  Neither arm
includes the ray generation that follows.  One process, needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((378, 504, 20), (800, 800, 100))
N_RANDS = (1024, 4096)
REPEATS, BLOCK, WARMUP = 5, 50, 20


class HostPath:
    """the parent way of making a batch: Loop.ray_batch without the ray generation"""

    def __init__(self, images, i_train, N_rand, mode):
        self.images, self.i_train, self.N_rand, self.mode = images, i_train, N_rand, mode
        self.H, self.W = images.shape[1:3]
        self.device = images.device
        if mode == "all_images":
            self.shuffled_ray_idx = np.arange(len(i_train) * self.H * self.W)
            t0 = time.perf_counter()
            np.random.shuffle(self.shuffled_ray_idx)
            self.shuffle_s = time.perf_counter() - t0
            self.shuffled_image_idx = self.shuffled_ray_idx // (self.H * self.W)
            self.i_batch = 0

    def next(self):
        H, W, N_rand = self.H, self.W, self.N_rand
        if self.mode == "all_images":
            sel = self.shuffled_ray_idx[self.i_batch:self.i_batch + N_rand]
            image_idx = self.shuffled_image_idx[self.i_batch:self.i_batch + N_rand]
            h_list, w_list = sel % (H * W) // W, sel % (H * W) % W
            kps_list = torch.from_numpy(np.stack([w_list, h_list], -1)).to(self.device)
            idx = torch.from_numpy(image_idx).to(self.device)
            index_train = self.i_train[image_idx]
            target_s = self.images[index_train, h_list, w_list]
            np.random.choice(index_train)
            self.i_batch += N_rand
            if self.i_batch >= len(self.shuffled_ray_idx):                 # (not reached in the timed window: see shuffle_s)
                np.random.shuffle(self.shuffled_ray_idx)
                self.shuffled_image_idx = self.shuffled_ray_idx // (H * W)
                self.i_batch = 0
            return kps_list, idx, target_s
        img_i = np.random.choice(self.i_train)
        target = self.images[img_i]
        gx, gy = torch.meshgrid(torch.linspace(0, W - 1, W, device=self.device),      # on the device, as with the
                                torch.linspace(0, H - 1, H, device=self.device), indexing="ij")  # reference's cuda default tensor type
        coords = torch.stack([gx, gy], -1).reshape(-1, 2)
        select_coords = coords[np.random.choice(coords.shape[0], size=[N_rand], replace=False)].long()
        return select_coords, img_i, target[select_coords[:, 1], select_coords[:, 0]]


def block_seconds(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / n, (t1 - t0) / n


def spread(v):
    return {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)}


def bench_point(H, W, n_img, N_rand, mode, repeats, block):
    from scnerf_amd.batching import RayBatcher
    images = torch.rand((n_img, H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(H + n_img))
    i_train = np.arange(n_img)
    np.random.seed(0)
    host = HostPath(images, i_train, N_rand, mode)
    batcher = RayBatcher(images, N_rand, mode=mode, image_ids=i_train, seed=0)
    if mode == "one_image":
        hip = lambda: batcher.next(img_i=np.random.choice(i_train))
    else:
        hip = batcher.next
    for _ in range(WARMUP):
        hip()
        host.next()
    t_hip, t_hip_enqueue, t_host = [], [], []
    for _ in range(repeats):
        a, b = block_seconds(hip, block)
        t_hip.append(a)
        t_hip_enqueue.append(b)
        t_host.append(block_seconds(host.next, block)[0])
    events = []
    for _ in range(block):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip()
        e1.record()
        e1.synchronize()
        events.append(e0.elapsed_time(e1) * 1e-3)
    rec = {"size": [H, W], "images": n_img, "N_rand": N_rand, "mode": mode, "steps_per_arm": repeats * block,
           "hip_step": spread(t_hip), "hip_enqueue_only": spread(t_hip_enqueue), "hip_between_events": spread(events),
           "host_path_step": spread(t_host),
           "host_over_hip": statistics.median(t_host) / statistics.median(t_hip)}
    if mode == "all_images":
        steps_per_epoch = n_img * H * W / N_rand
        rec["host_epoch_shuffle_ms"] = 1e3 * host.shuffle_s
        rec["host_epoch_shuffle_ms_per_step"] = 1e3 * host.shuffle_s / steps_per_epoch
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "batching_bench.json"))
    ap.add_argument("--quick", action="store_true", help="one small point, a few steps: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batching.py measures on the GPU; there is none here")
    sizes, n_rands, repeats, block = (((48, 64, 3),), (256,), 2, 5) if a.quick else (SIZES, N_RANDS, REPEATS, BLOCK)
    out = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "block": block, "warmup": WARMUP, "quick": a.quick,
           "points": [bench_point(H, W, n, N, mode, repeats, block) for (H, W, n) in sizes for N in n_rands
                      for mode in ("one_image", "all_images")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for p in out["points"]:
        print("%4dx%-4d x%-3d N=%-4d %-10s  hip %.3f ms [%.3f, %.3f] (enqueue %.3f, events %.3f)  host path %.3f ms [%.3f, %.3f]  x%.1f%s" % (
            p["size"][0], p["size"][1], p["images"], p["N_rand"], p["mode"], p["hip_step"]["median_ms"], p["hip_step"]["min_ms"],
            p["hip_step"]["max_ms"], p["hip_enqueue_only"]["median_ms"], p["hip_between_events"]["median_ms"],
            p["host_path_step"]["median_ms"], p["host_path_step"]["min_ms"], p["host_path_step"]["max_ms"], p["host_over_hip"],
            "  (+ %.3f ms per step of epoch shuffle)" % p["host_epoch_shuffle_ms_per_step"] if "host_epoch_shuffle_ms" in p else ""))
    print(json.dumps({"metric": "training batch, host path time over RayBatcher.next() time per step (smallest point)",
                      "value": min(p["host_over_hip"] for p in out["points"]), "out": a.out}))


if __name__ == "__main__":
    main()
