"""TEST INFRASTRUCTURE for the image-metric tests (test_metrics_oracle.py, test_emu_metrics.py, test_gpu_metrics.py).

* `oracle()`: SSIM / MSE in torch fp64, written from the definition in INTEGRATION.md ("Image-quality metrics"): shifted
  weighted sums, no convolution routine.  It uses the kernel's fp32 taps widened to fp64, so the taps are no source of
  difference.
* `fp32_formulation()`: the same definition evaluated op by op in fp32 with torch's conv2d on the CPU -- how piqa evaluates it.
  Its error against the oracle, measured on a test's own images, is the yardstick the kernel is held to (`yardstick`, `bound`).
* `images()`: the three image classes, from seeded torch generators.
* `CASES`: the size / window / clip grid the interpreter and GPU tests share.

Sizes.  The kernel tiles the map in 32 x 32 blocks of window origins (csrc/image_metrics.hip, kTile), so for a window of `win`
taps the map extents 1, 31, 32, 33 and 65 -- H, W in {win, win + 30, win + 31, win + 32, win + 64} -- are the smallest at which
tiling can go wrong: one origin, one short of a tile, exactly a tile, one origin in a second tile, one in a third."""
import functools

import numpy as np
import torch

TILE = 32
CLASSES = ("noise", "smooth", "bright")
WINDOWS = (11, 7)
K1, K2, VALUE_RANGE = 0.01, 0.03, 1.0
C1, C2 = (K1 * VALUE_RANGE) ** 2, (K2 * VALUE_RANGE) ** 2


def sizes(win):
    """(H, W) pairs: for win = 11 these are 11x11, 11x43, 43x11, 42x42, 43x75, 75x43"""
    one, full, over, three = win, win + TILE - 1, win + TILE, win + 2 * TILE
    return ((one, one), (one, over), (over, one), (full, full), (over, three), (three, over))


# (win, H, W, clip_x): every size at both windows, clamping on and off
CASES = tuple((win, h, w, clip) for win in WINDOWS for (h, w) in sizes(win) for clip in (False, True))
LAYOUTS = (("nchw", "nchw"), ("nhwc", "nhwc"), ("nchw", "nhwc"), ("nhwc", "nchw"))


def taps(win, sigma=1.5):
    """the window as the product computes it: fp64, rounded to fp32"""
    d = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def images(cls, n, c, h, w, seed=0, overshoot=False):
    """(x, y) float32 [n, c, h, w], contiguous.  `overshoot`: x + 0.02 Gaussian noise on top, so that some of x lies outside
    [0, 1] and clamping it matters."""
    gen = torch.Generator().manual_seed(1000 * seed + 17 * h + w + 7 * CLASSES.index(cls))
    rand = lambda: torch.rand((n, c, h, w), generator=gen, dtype=torch.float64)
    randn = lambda: torch.randn((n, c, h, w), generator=gen, dtype=torch.float64)
    if cls == "noise":
        x, y = rand(), rand()
    elif cls == "smooth":
        yy = torch.arange(h, dtype=torch.float64)[:, None] / 16.0
        xx = torch.arange(w, dtype=torch.float64)[None, :] / 16.0
        x = torch.stack([torch.stack([0.5 + 0.4 * torch.sin((1.0 + 0.3 * ch) * xx + (0.7 + 0.2 * ch) * yy + 0.9 * i + ch)
                                      for ch in range(c)]) for i in range(n)])
        y = (x + 0.05 * randn()).clamp(0.0, 1.0)
    elif cls == "bright":
        x = 0.97 + 0.03 * rand()
        y = x + 0.002 * randn()
    else:
        raise ValueError(cls)
    if overshoot:
        x = x + 0.02 * randn()
    return x.float().contiguous(), y.float().contiguous()


def channel_last(t):
    """the same values in [N, H, W, C] memory, viewed as [N, C, H, W] (what .permute(2, 0, 1)[None] of an image gives)"""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def in_layout(t, layout):
    return channel_last(t) if layout == "nhwc" else t.contiguous()


def _filter64(v, g):
    """separable, channel-wise, no padding: [..., H, W] -> [..., H - win + 1, W - win + 1]"""
    win = g.shape[0]
    oh, ow = v.shape[-2] - win + 1, v.shape[-1] - win + 1
    rows = sum(g[t] * v[..., :, t:t + ow] for t in range(win))
    return sum(g[t] * rows[..., t:t + oh, :] for t in range(win))


def oracle(x, y, g32, clip=False, c1=C1, c2=C2, value_range=VALUE_RANGE):
    """-> (per_channel [N, C] fp64: mean of ss over the map, ss map [N, C, OH, OW] fp64, squared error sums [N, C] fp64).
    The per-image SSIM of the first c channels is per_channel[:, :c].mean(1); the MSE is sums[:, :c].sum(1) / (c H W)."""
    g = torch.from_numpy(np.asarray(g32, np.float32)).double()
    x64, y64 = x.double(), y.double()
    sse = ((x64 - y64) ** 2).sum((2, 3))
    if clip:
        x64 = x64.clamp(0.0, value_range)
    mu_x, mu_y = _filter64(x64, g), _filter64(y64, g)
    s_xx = _filter64(x64 * x64, g) - mu_x * mu_x
    s_yy = _filter64(y64 * y64, g) - mu_y * mu_y
    s_xy = _filter64(x64 * y64, g) - mu_x * mu_y
    cs = (2 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1) * cs
    return ss.mean((2, 3)), ss, sse


def fp32_formulation(x, y, g32, clip=False, c1=C1, c2=C2, value_range=VALUE_RANGE):
    """The definition op by op in fp32 with conv2d (groups = channels, one pass per axis) -> (per_channel [N, C], map), fp32.
    ATen's own convolution, not oneDNN's: the same arithmetic on every host (oneDNN picks a kernel per instruction set), and
    no primitive is compiled per shape (a second per class on an idle machine, many under four test workers)."""
    import torch.nn.functional as F
    saved = torch.backends.mkldnn.enabled
    torch.backends.mkldnn.enabled = False
    try:
        return _fp32_formulation(x, y, g32, clip, c1, c2, value_range, F)
    finally:
        torch.backends.mkldnn.enabled = saved


def _fp32_formulation(x, y, g32, clip, c1, c2, value_range, F):
    c = x.shape[1]
    g = torch.from_numpy(np.asarray(g32, np.float32))
    kv = g.view(1, 1, -1, 1).repeat(c, 1, 1, 1)
    kh = g.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    conv = lambda v: F.conv2d(F.conv2d(v, kv, groups=c), kh, groups=c)
    x = x.float().contiguous()
    y = y.float().contiguous()
    if clip:
        x = x.clamp(0.0, value_range)
    mu_x, mu_y = conv(x), conv(y)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_xx = conv(x ** 2) - mu_xx
    s_yy = conv(y ** 2) - mu_yy
    s_xy = conv(x * y) - mu_xy
    cs = (2 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return ss.mean((2, 3)), ss


@functools.lru_cache(maxsize=None)
def case_data(cls, win, h, w, clip):
    """One case's images (N = 2, C = 3; the tests take subsets) with its oracle and fp32-formulation results; computed once
    and shared -- callers must not modify it."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)        # small tensors: four test workers' thread pools only wait for each other
    try:
        x, y = images(cls, 2, 3, h, w, seed=win, overshoot=clip)
        g = taps(win)
        per_channel, ss, sse = oracle(x, y, g, clip)
        ref_pc, ref_ss = fp32_formulation(x, y, g, clip)
    finally:
        torch.set_num_threads(threads)
    return {"x": x, "y": y, "taps": g, "per_channel": per_channel, "map": ss, "sse": sse,
            "ref_per_channel": ref_pc, "ref_map": ref_ss}


def ssim_of(per_channel, n, c):
    """per-image value of the first n images' first c channels from the per-channel means (fp64)"""
    return per_channel[:n, :c].double().mean(1)


@functools.lru_cache(maxsize=None)
def yardstick(cls, extra=()):
    """E32 of a class: the largest error of the fp32 formulation against the oracle over all of CASES (plus `extra`,
    further (win, h, w, clip) tuples a test adds), -> (per-image E32 over C in {1, 3}, per-element E32 of the map)."""
    e_value, e_map = 0.0, 0.0
    for case in CASES + tuple(extra):
        d = case_data(cls, *case)
        for c in (1, 3):
            e_value = max(e_value, float((ssim_of(d["ref_per_channel"], 2, c) - ssim_of(d["per_channel"], 2, c)).abs().max()))
        e_map = max(e_map, float((d["ref_map"].double() - d["map"]).abs().max()))
    return e_value, e_map


def bound(e32):
    """what the kernel's error against fp64 may be: 4 x the fp32 formulation's own (another summation order, and a class
    maximum over a dozen sizes is still a sample), floored at a handful of fp32 roundings of a value below 1"""
    return max(4.0 * e32, 2.0 ** -22)


MSE_RTOL = 2.0 ** -21        # each squared term carries at most three fp32 roundings; the sums are fp64
