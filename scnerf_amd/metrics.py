"""Image-quality metrics on the device: SSIM, MSE and PSNR from one fused HIP kernel (csrc/image_metrics.hip).

The reference scores every test and train image with `img2mse`, `mse2psnr` and `piqa.ssim.SSIM`
(NeRF/run_nerf.py:748-795, :987-1040; nerfplusplus/ddp_test_nerf.py:122-196).  `SSIM` below takes piqa's constructor
arguments and is called the same way; `scnerf_amd.dropin.install_metrics()` registers it under piqa's module names when
piqa itself is not installed.

Definition (Wang et al. 2004 with the defaults piqa documents; INTEGRATION.md, "Image-quality metrics"): a normalised
1-D Gaussian of `window_size` taps applied separably, channel by channel, without padding;
    ss = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 s_xy + c2) / (s_xx + s_yy + c2),
c1 = (k1 L)^2, c2 = (k2 L)^2; the per-image value is the mean of ss over the map and the channels.  The definition is
transcribed, not pinned against piqa: tests/test_metrics_oracle.py compares the two wherever piqa is installed.

The metrics are forward-only (the reference evaluates under no_grad) and there is no CPU path."""
from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from . import ops


def gaussian_taps(window_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """The normalised 1-D Gaussian window: computed in fp64, rounded to fp32 (the values the kernel multiplies by)."""
    window_size = int(window_size)
    if window_size % 2 == 0 or not 3 <= window_size <= 11:
        raise ValueError("window_size must be odd and between 3 and 11, got %d" % window_size)
    d = np.arange(window_size, dtype=np.float64) - (window_size - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * float(sigma) ** 2))
    return (g / g.sum()).astype(np.float32)


_taps_cache = {}


def _device_taps(window_size, sigma, device):
    key = (int(window_size), float(sigma), str(device))
    t = _taps_cache.get(key)
    if t is None:
        t = _taps_cache[key] = torch.from_numpy(gaussian_taps(window_size, sigma)).to(device)
    return t


def _ln10(device):
    """log(10) as a device tensor, the divisor of mse2psnr (run_nerf_helpers.py:11), made once per device"""
    key = ("ln10", str(device))
    t = _taps_cache.get(key)
    if t is None:
        t = _taps_cache[key] = torch.log(torch.tensor(10., device=device))
    return t


def _forward_only(*tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise NotImplementedError("scnerf_amd.metrics is forward-only (the reference evaluates under torch.no_grad()): "
                                  "detach the inputs or call it under no_grad")


def _reduce(v, reduction):
    if reduction == "none":
        return v
    if reduction == "mean":
        return v.mean()
    if reduction == "sum":
        return v.sum()
    raise ValueError("reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))


def _run(x, y, taps, value_range, k1, k2, clip_x, want_map):
    _forward_only(x, y)
    L = float(value_range)
    return ops.image_metrics(x.detach(), y.detach(), taps, (k1 * L) ** 2, (k2 * L) ** 2, L, clip_x, want_map)


def ssim(x, y, window_size=11, sigma=1.5, value_range=1., k1=0.01, k2=0.03, return_map=False):
    """SSIM of x against y, both [N, C, H, W] fp32 on the device with any strides -> [N] (and the map
    [N, C, H - window_size + 1, W - window_size + 1] with `return_map`)."""
    s, _, m = _run(x, y, _device_taps(window_size, sigma, x.device), value_range, k1, k2, False, return_map)
    return (s, m) if return_map else s


class SSIM(torch.nn.Module):
    """piqa.ssim.SSIM's interface on the fused kernel: `SSIM().cuda()(x, y)` with x, y [N, C, H, W] in [0, value_range].
    `n_channels` is accepted for compatibility (the window is the same for every channel)."""

    def __init__(self, window_size=11, sigma=1.5, n_channels=3, reduction="mean", value_range=1., k1=0.01, k2=0.03):
        super().__init__()
        _reduce(torch.zeros(1), reduction)           # an unknown reduction fails here, not at the first image
        self.register_buffer("taps", torch.from_numpy(gaussian_taps(window_size, sigma)))
        self.n_channels = int(n_channels)
        self.reduction = reduction
        self.value_range = float(value_range)
        self.k1, self.k2 = float(k1), float(k2)

    def forward(self, x, y):
        taps = self.taps
        if taps.device != x.device or taps.dtype != torch.float32:      # a module never moved, or moved with .double()
            taps = taps.to(device=x.device, dtype=torch.float32)
        s, _, _ = _run(x, y, taps, self.value_range, self.k1, self.k2, False, False)
        return _reduce(s, self.reduction)


def image_metrics(rgb, gt, clip=True, window_size=11, sigma=1.5, value_range=1., k1=0.01, k2=0.03):
    """What the reference's evaluation loop computes per image (NeRF/run_nerf.py:757-772), from ONE kernel call and without
    a host synchronisation: rgb, gt [H, W, 3] or [N, H, W, 3] (channel-last, as render_path produces them; read in place)
    -> {"mse", "psnr", "ssim"}, device tensors of shape [] or [N].  `clip` clamps rgb to [0, value_range] for SSIM only;
    the squared error is taken on the unclipped image, as the loop does.  psnr = -10 ln(mse) / ln(10) as mse2psnr."""
    if rgb.dim() not in (3, 4) or rgb.shape != gt.shape:
        raise ValueError("rgb and gt must both be [H, W, C] or [N, H, W, C], got %s and %s" % (tuple(rgb.shape), tuple(gt.shape)))
    single = rgb.dim() == 3
    x = (rgb[None] if single else rgb).permute(0, 3, 1, 2)
    y = (gt[None] if single else gt).permute(0, 3, 1, 2)
    s, mse, _ = _run(x, y, _device_taps(window_size, sigma, x.device), value_range, k1, k2, bool(clip), False)
    psnr = -10. * torch.log(mse) / _ln10(mse.device)
    out = {"mse": mse, "psnr": psnr, "ssim": s}
    return {k: v[0] for k, v in out.items()} if single else out


class LPIPSUnavailable(torch.nn.Module):
    """Stand-in for piqa.lpips.LPIPS where piqa is not installed: LPIPS needs pretrained network weights that this
    package does not ship.  It can be constructed and moved like the real one and returns NaN -- never a number that
    could pass for a measurement -- with one warning per instance."""

    def __init__(self, network="alex", scales=True, dropout=False, pretrained=True, eval=True, reduction="mean"):
        super().__init__()
        self.network = network
        self.reduction = reduction
        self._warned = False

    def forward(self, x, y):
        if not self._warned:
            self._warned = True
            warnings.warn("LPIPS is not available (piqa is not installed and scnerf_amd ships no %s weights): "
                          "the value returned is NaN" % self.network, UserWarning, stacklevel=2)
        v = torch.full((x.shape[0],) if x.dim() == 4 else (), math.nan, dtype=torch.float32, device=x.device)
        return v if self.reduction == "none" or v.dim() == 0 else v.sum() if self.reduction == "sum" else v.mean()
