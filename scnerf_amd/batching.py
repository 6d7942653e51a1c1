"""Training ray batches drawn on the device: one HIP launch per step (csrc/ray_batch.hip).

The reference's train() makes every batch on the host (NeRF/run_nerf.py): from one image, `np.random.choice(H * W,
size=[N_rand], replace=False)` -- numpy permutes all H W indices to hand back N_rand of them -- a meshgrid and three gathers
(:409-478); from all images with a camera model, `%` and `//` over slices of a host permutation, two host-to-device copies,
a gather with host index arrays and np.random.shuffle over every ray at each epoch end (:368-407).  `RayBatcher` replaces
both: the batch is a pure function of (seed, step, rank), computed by one kernel that the host never waits for.

    batcher = RayBatcher(images, N_rand, mode="one_image", image_ids=i_train)
    b = batcher.next(img_i=img_i, precrop_frac=args.precrop_frac if i < args.precrop_iters else None)
    rays_o, rays_d = get_rays_kps_use_camera(H, W, camera_model, idx_in_camera_param=b.image_idx, kps_list=b.coords)
    target_s = b.target

The sample is *a* uniform sample without replacement, not numpy's sample for the same seed (DESIGN.md section 4.10 has the
construction).  In "all_images" mode every epoch visits every ray of every selected image exactly once, and every batch
has N_rand rays: where the reference's last batch of an epoch is short, ours continues into the next epoch's permutation.
With world_size > 1 the ranks' batches of a step are disjoint slices of one global batch of world_size N_rand rays -- no
communication, no per-rank seeding.  There is no CPU path."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _capi, ops

Batch = namedtuple("Batch", ["coords", "select_inds", "image_idx", "target"])
Batch.__doc__ = """coords int64 [N, 2] as (x, y) (the reference's select_coords.long() / kps_list); select_inds int64 [N] =
y W + x (nerfplusplus's render_ray_from_camera); image_idx int64 [N], the position of each ray's image in the selected
list (idx_in_camera_param); target fp32 [N, 3]."""

MODES = {"one_image": 0, "all_images": 1}
MAX_RAYS = 1 << 40


def precrop_window(H: int, W: int, frac: float):
    """The reference's centre crop (NeRF/run_nerf.py:418-431) as (x0, y0, w, h)"""
    dH, dW = int(H // 2 * frac), int(W // 2 * frac)
    return W // 2 - dW, H // 2 - dH, 2 * dW, 2 * dH


class RayBatcher:
    """images: [n, H, W, 3] fp32, or uint8 [n, H, W, 3 | 4] (a quarter of the memory; converted as the loaders do,
    `(v / 255.).astype(np.float32)`, 4 channels composited over white with `white_bkgd`, alpha dropped without), on the device, read in
    place.  image_ids: the rows of `images` to draw from (the reference's i_train; default all), host integers or a tensor.
    seed: default torch.initial_seed().  rank / world_size: this process's slice of the global batch."""

    def __init__(self, images, N_rand, mode="one_image", image_ids=None, seed=None, rank=0, world_size=1, white_bkgd=False):
        if mode not in MODES:
            raise ValueError("mode must be 'one_image' or 'all_images', got %r" % (mode,))
        if not _capi.on_device(images):
            raise RuntimeError("images must live on the GPU (scnerf_amd has no CPU path)")
        if images.dtype not in (torch.float32, torch.uint8):
            raise TypeError("images must be torch.float32 or torch.uint8, got %s" % images.dtype)
        if images.dim() != 4 or images.shape[3] not in ((3, 4) if images.dtype == torch.uint8 else (3,)):
            raise ValueError("images must be [n, H, W, 3] (fp32) or [n, H, W, 3 | 4] (uint8), got %s %s" % (
                images.dtype, tuple(images.shape)))
        if not images.is_contiguous():
            raise ValueError("images must be contiguous")
        n, self.H, self.W = (int(v) for v in images.shape[:3])
        if image_ids is None:
            ids = list(range(n))
            self._ids = None
        else:
            # once, at construction: the host copy answers next(img_i=...) without touching the device
            ids = [int(v) for v in (image_ids.tolist() if hasattr(image_ids, "tolist") else image_ids)]
            if not ids or min(ids) < 0 or max(ids) >= n:
                raise ValueError("image_ids must name rows of images (0 .. %d), got %s" % (n - 1, ids))
            self._ids = torch.tensor(ids, dtype=torch.int64).to(images.device)
        self._where = {row: pos for pos, row in reversed(list(enumerate(ids)))}
        self.n_sel = len(ids)
        self.images, self.mode, self.N_rand = images, mode, int(N_rand)
        self.rank, self.world_size, self.white_bkgd = int(rank), int(world_size), bool(white_bkgd)
        if self.N_rand < 0 or self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError("need N_rand >= 0 and 0 <= rank < world_size, got %d, %d, %d" % (self.N_rand, self.rank, self.world_size))
        if self.n_sel * self.H * self.W >= MAX_RAYS:
            raise ValueError("%d rays: the permutation covers fewer than 2^40" % (self.n_sel * self.H * self.W))
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.step = 0

    def next(self, img_i=None, precrop_frac=None) -> Batch:
        """The batch of the current step, and the step moves on.  one_image: `img_i` is the row of `images` the batch
        comes from (a member of image_ids, as the reference's np.random.choice(i_train)); `precrop_frac` restricts it to
        the centre crop.  all_images: neither is accepted.  The host does not wait for the device."""
        H, W = self.H, self.W
        window, pos = (0, 0, W, H), 0
        if self.mode == "one_image":
            if img_i is None:
                raise ValueError("one_image mode needs img_i, the row of `images` to draw from")
            pos = self._where.get(int(img_i))
            if pos is None:
                raise ValueError("img_i = %d is not among image_ids" % int(img_i))
            if precrop_frac is not None:
                window = precrop_window(H, W, precrop_frac)
                if window[2] < 1 or window[3] < 1 or window[2] > W or window[3] > H:
                    raise ValueError("precrop_frac = %r leaves no window inside %d x %d" % (precrop_frac, H, W))
            if self.world_size * self.N_rand > window[2] * window[3]:
                raise ValueError("cannot take %d x %d rays without replacement from a window of %d pixels" % (
                    self.world_size, self.N_rand, window[2] * window[3]))
        elif img_i is not None or precrop_frac is not None:
            raise ValueError("img_i and precrop_frac belong to one_image mode")
        out = ops.ray_batch(MODES[self.mode], self.seed, self.step, self.images, self._ids, self.n_sel, pos, H, W, window,
                            self.N_rand, self.rank, self.world_size, self.white_bkgd)
        self.step += 1
        return Batch(*out)

    def state_dict(self):
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state):
        self.seed, self.step = int(state["seed"]) & 0xFFFFFFFFFFFFFFFF, int(state["step"])
