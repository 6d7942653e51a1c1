"""scnerf_amd.metrics on the MI355X against the fp64 oracle: the grid of tests/metrics_reference.py (sizes at the tile
edges, both windows, both layouts and mixed, C in {1, 3}, N in {1, 2}, clamping on and off), one LLFF-sized image,
image_metrics, the error paths and a non-default stream.

Bounds as in test_emu_metrics.py: max(4 E32, 2^-22) against fp64, E32 the error of the fp32 conv2d formulation on the same
images (here including the 378 x 504 case); MSE to 2^-21 relative."""
import pytest
import torch

from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

LLFF = (11, 378, 504, False)         # an LLFF image at factor 8


def on_gpu(t, layout):
    return R.in_layout(t, layout).cuda() if layout == "nchw" else R.channel_last(t.cuda())


def check(d, ssim, mse, ss, n, c, e_value, e_map, what):
    h, w = d["x"].shape[-2:]
    ssim, mse = ssim.cpu().double(), mse.cpu().double()
    assert torch.isfinite(ssim).all() and torch.isfinite(mse).all(), what
    err = float((ssim - R.ssim_of(d["per_channel"], n, c)).abs().max())
    print("%s: ssim err %.3g (bound %.3g)" % (what, err, R.bound(e_value)))
    assert err <= R.bound(e_value), (what, err, R.bound(e_value))
    if ss is not None:
        err_map = float((ss.cpu().double() - d["map"][:n, :c]).abs().max())
        assert err_map <= R.bound(e_map), (what, "map", err_map, R.bound(e_map))
    want_mse = d["sse"][:n, :c].sum(1) / (c * h * w)
    rel = float(((mse - want_mse).abs() / want_mse).max())
    assert rel <= R.MSE_RTOL, (what, "mse", rel)


@pytest.mark.parametrize("case", R.CASES, ids=lambda k: "win%d-%dx%d-clip%d" % k)
@pytest.mark.parametrize("cls", R.CLASSES)
def test_grid_against_oracle(cls, case):
    from scnerf_amd import metrics, ops
    win, h, w, clip = case
    d = R.case_data(cls, *case)
    e_value, e_map = R.yardstick(cls, (LLFF,))
    taps = torch.from_numpy(d["taps"]).cuda()
    for lx, ly in R.LAYOUTS:
        x, y = on_gpu(d["x"], lx), on_gpu(d["y"], ly)
        for c in (1, 3):
            for n in (1, 2):
                xs, ys = x[:n, :c], y[:n, :c]
                what = "%s %s x=%s y=%s C=%d N=%d" % (cls, case, lx, ly, c, n)
                # the kernel's three outputs, clamping as the case says
                s, m, ss = ops.image_metrics(xs, ys, taps, R.C1, R.C2, R.VALUE_RANGE, clip, want_map=True)
                check(d, s, m, ss, n, c, e_value, e_map, what)
                # the public forms give the same bits
                out = metrics.image_metrics(xs.permute(0, 2, 3, 1), ys.permute(0, 2, 3, 1), clip=clip, window_size=win)
                assert torch.equal(out["ssim"], s) and torch.equal(out["mse"], m)
                if not clip:
                    s2, ss2 = metrics.ssim(xs, ys, window_size=win, return_map=True)
                    assert torch.equal(s2, s) and torch.equal(ss2, ss)


@pytest.mark.parametrize("cls", R.CLASSES)
def test_llff_sized_image(cls):
    from scnerf_amd import metrics
    d = R.case_data(cls, *LLFF)
    e_value, e_map = R.yardstick(cls, (LLFF,))
    x, y = on_gpu(d["x"], "nhwc"), on_gpu(d["y"], "nchw")
    s, ss = metrics.ssim(x, y, return_map=True)
    out = metrics.image_metrics(x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1), clip=False)
    check(d, s, out["mse"], ss, 2, 3, e_value, e_map, "%s 378x504" % cls)
    assert torch.equal(out["ssim"], s)
    single = metrics.ssim(x[1:], y[1:])
    assert torch.equal(single, s[1:])                                 # an image's bits do not depend on its batch


def test_identical_images_give_one():
    from scnerf_amd import metrics
    for cls in R.CLASSES:
        x, _ = R.images(cls, 2, 3, 43, 75)
        s, ss = metrics.ssim(on_gpu(x, "nchw"), on_gpu(x, "nhwc"), return_map=True)
        assert float((s - 1).abs().max()) <= 2.0 ** -23 and float((ss - 1).abs().max()) <= 2.0 ** -23


def test_image_metrics_against_oracle_and_module_interface():
    from scnerf_amd import metrics
    from scnerf_amd.run_nerf_helpers import img2mse, mse2psnr
    d = R.case_data("noise", 11, 43, 75, True)             # x overshoots [0, 1]: clamping matters
    e_value, _ = R.yardstick("noise", (LLFF,))
    rgb = d["x"].permute(0, 2, 3, 1).contiguous().cuda()     # [N, H, W, 3] as render_path produces it
    gt = d["y"].permute(0, 2, 3, 1).contiguous().cuda()
    out = metrics.image_metrics(rgb, gt)
    assert sorted(out) == ["mse", "psnr", "ssim"]
    assert all(v.is_cuda and v.shape == (2,) and v.dtype == torch.float32 for v in out.values())      # results stay on the device
    check(d, out["ssim"], out["mse"], None, 2, 3, e_value, 0.0, "image_metrics")
    assert torch.equal(out["psnr"], mse2psnr(out["mse"]))
    one = metrics.image_metrics(rgb[0], gt[0])
    assert all(one[k].shape == () and torch.equal(one[k], out[k][0]) for k in out)
    # against the reference loop's own expressions (NeRF/run_nerf.py:757-772) on the device
    # (img2mse is an fp32 reduction of 9675 terms: some log2(n) roundings of 2^-24 each)
    assert abs(float(one["mse"]) - float(img2mse(rgb[0], gt[0]))) <= 1e-5 * float(one["mse"])
    model = metrics.SSIM().cuda()
    assert model.taps.is_cuda
    v = model(torch.clip(rgb[0].permute(2, 0, 1)[None], 0, 1), gt[0].permute(2, 0, 1)[None])
    assert v.shape == () and torch.equal(v, one["ssim"])
    per_image = metrics.SSIM(reduction="none").to("cuda")(rgb.permute(0, 3, 1, 2).clamp(0, 1), gt.permute(0, 3, 1, 2))
    assert torch.equal(per_image, out["ssim"])
    assert torch.equal(metrics.SSIM(reduction="sum").cuda()(rgb.permute(0, 3, 1, 2).clamp(0, 1), gt.permute(0, 3, 1, 2)), per_image.sum())


def test_error_paths():
    from scnerf_amd import metrics
    x, y = R.images("noise", 1, 3, 16, 16)
    with pytest.raises(RuntimeError):
        metrics.SSIM()(x, y)                                  # CPU tensors
    with pytest.raises(RuntimeError):
        metrics.image_metrics(x[0].permute(1, 2, 0), y[0].permute(1, 2, 0))
    xg, yg = x.cuda(), y.cuda()
    with pytest.raises(NotImplementedError, match="forward-only"):
        metrics.SSIM().cuda()(xg.clone().requires_grad_(True), yg)
    with pytest.raises(NotImplementedError, match="forward-only"):
        metrics.ssim(xg, yg.clone().requires_grad_(True))
    with torch.no_grad():
        assert metrics.ssim(xg.clone().requires_grad_(True), yg).shape == (1,)
    with pytest.raises(ValueError):
        metrics.ssim(xg[..., :10], yg[..., :10])
    with pytest.raises(ValueError):
        metrics.ssim(xg, yg, window_size=8)
    with pytest.raises(TypeError):
        metrics.ssim(xg.double(), yg.double())
    assert metrics.ssim(xg[:0], yg[:0]).shape == (0,)


def test_non_default_stream_gives_the_same_bits():
    from scnerf_amd import metrics
    d = R.case_data("noise", 11, 43, 75, False)
    x, y = on_gpu(d["x"], "nhwc"), on_gpu(d["y"], "nchw")
    s0, m0 = metrics.ssim(x, y, return_map=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s1, m1 = metrics.ssim(x, y, return_map=True)
        out = metrics.image_metrics(x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1), clip=False)
    side.synchronize()
    assert torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(out["ssim"], s0)
