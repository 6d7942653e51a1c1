"""Image metrics on the MI355X: scnerf_amd.metrics.image_metrics (one fused HIP pass: MSE, PSNR, SSIM) against the same
quantities from torch operators in fp32 on the same device -- what a user with piqa runs per evaluated image
(NeRF/run_nerf.py:757-772): img2mse, mse2psnr, clip, five Gaussian-filtered maps through conv2d.

    python tools/bench_metrics.py [--accuracy] [--out profiles/metrics_bench.json]

Sizes 378x504 (LLFF at factor 8), 800x800 (Blender) and 1080x1920, C = 3, one image, in both memory layouts (contiguous
[1, 3, H, W]; the channel-last [H, W, 3] that render_path produces).  Per point: median / min / max of 20 event-timed repeats
after warm-up, the two paths alternating; bytes/s = the two images' bytes over the time (each is read once by the fused pass).
Clocks and power are whatever the socket gives while it runs; the spread is part of the record.  One process, needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((378, 504), (800, 800), (1080, 1920))
REPEATS, WARMUP = 20, 5


def torch_formulation(x, y, kv, kh, c1, c2):
    """x, y [N, C, H, W] (any strides) -> mse, psnr, ssim [N] with torch operators in fp32 (piqa's sequence of operations)"""
    mse = ((x - y) ** 2).mean((1, 2, 3))
    psnr = -10. * torch.log(mse) / torch.log(torch.tensor([10.], device=x.device))
    x = torch.clip(x, 0, 1)
    c = x.shape[1]
    conv = lambda v: F.conv2d(F.conv2d(v, kv, groups=c), kh, groups=c)
    mu_x, mu_y = conv(x), conv(y)
    mu_xx, mu_yy, mu_xy = mu_x ** 2, mu_y ** 2, mu_x * mu_y
    s_xx, s_yy, s_xy = conv(x ** 2) - mu_xx, conv(y ** 2) - mu_yy, conv(x * y) - mu_xy
    cs = (2 * s_xy + c2) / (s_xx + s_yy + c2)
    ss = (2 * mu_xy + c1) / (mu_xx + mu_yy + c1) * cs
    return mse, psnr, ss.flatten(1).mean(-1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def bench_point(h, w, layout, metrics):
    gen = torch.Generator().manual_seed(h * 7 + w)
    gt = torch.rand((1, h, w, 3), generator=gen)
    rgb = (gt + 0.05 * torch.randn((1, h, w, 3), generator=gen))           # overshoots [0, 1] here and there, as a render does
    if layout == "nchw":
        x, y = rgb.permute(0, 3, 1, 2).contiguous().cuda(), gt.permute(0, 3, 1, 2).contiguous().cuda()
    else:
        x, y = rgb.cuda().permute(0, 3, 1, 2), gt.cuda().permute(0, 3, 1, 2)
    taps = torch.from_numpy(metrics.gaussian_taps(11, 1.5)).cuda()
    kv, kh = taps.view(1, 1, -1, 1).repeat(3, 1, 1, 1), taps.view(1, 1, 1, -1).repeat(3, 1, 1, 1)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    hip = lambda: metrics.image_metrics(x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1), clip=True)
    ref = lambda: torch_formulation(x, y, kv, kh, c1, c2)
    for _ in range(WARMUP):
        hip()
        ref()
    torch.cuda.synchronize()
    t_hip, t_ref = [], []
    for _ in range(REPEATS):
        t_hip.append(timed(hip))
        t_ref.append(timed(ref))
    a, b = hip(), ref()
    nbytes = 2 * x.numel() * 4
    rec = {"size": [h, w], "channels": 3, "layout": layout, "hip": spread(t_hip), "torch_fp32": spread(t_ref),
           "bytes": nbytes, "hip_bytes_per_s": nbytes / (statistics.median(t_hip) * 1e-3),
           "torch_over_hip": statistics.median(t_ref) / statistics.median(t_hip),
           "hip_not_slower": statistics.median(t_hip) <= statistics.median(t_ref),
           "values": {"hip": {k: float(v[0]) for k, v in a.items()},
                      "torch_fp32": {"mse": float(b[0][0]), "psnr": float(b[1][0]), "ssim": float(b[2][0])}}}
    return rec


def accuracy(metrics):
    """E32 (the fp32 conv2d formulation's error against the fp64 oracle, on the CPU) and the kernel's error, per image class
    and size: the table the tests' bound max(4 E32, 2^-22) is read against."""
    from tests import metrics_reference as R
    rows = []
    for cls in R.CLASSES:
        for (h, w) in ((11, 11), (43, 75), (75, 43)) + SIZES[:1]:
            x, y = R.images(cls, 1, 3, h, w)
            g = R.taps(11)
            per_channel, ss, sse = R.oracle(x, y, g)
            ref_pc, ref_ss = R.fp32_formulation(x, y, g)
            want = R.ssim_of(per_channel, 1, 3)
            s, m = metrics.ssim(R.channel_last(x.cuda()), y.cuda(), return_map=True)
            rows.append({"class": cls, "size": [h, w],
                         "E32": float((R.ssim_of(ref_pc, 1, 3) - want).abs().max()),
                         "E32_map": float((ref_ss.double() - ss).abs().max()),
                         "kernel": float((s.cpu().double() - want).abs().max()),
                         "kernel_map": float((m.cpu().double() - ss).abs().max())})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU; there is none here")
    from scnerf_amd import metrics
    out = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "warmup": WARMUP,
           "points": [bench_point(h, w, layout, metrics) for (h, w) in SIZES for layout in ("nchw", "nhwc")]}
    out["hip_not_slower_everywhere"] = all(p["hip_not_slower"] for p in out["points"])
    if a.accuracy:
        out["accuracy"] = accuracy(metrics)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for p in out["points"]:
        print("%4dx%-4d %s  hip %.3f ms [%.3f, %.3f]  torch %.3f ms [%.3f, %.3f]  x%.1f  %.0f GB/s" % (
            p["size"][0], p["size"][1], p["layout"], p["hip"]["median_ms"], p["hip"]["min_ms"], p["hip"]["max_ms"],
            p["torch_fp32"]["median_ms"], p["torch_fp32"]["min_ms"], p["torch_fp32"]["max_ms"], p["torch_over_hip"],
            p["hip_bytes_per_s"] / 1e9))
    print(json.dumps({"metric": "image metrics, torch fp32 formulation time over fused HIP time (smallest of six points)",
                      "value": min(p["torch_over_hip"] for p in out["points"]), "out": a.out}))


if __name__ == "__main__":
    main()
