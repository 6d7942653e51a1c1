"""scnerf_image_metrics (csrc/image_metrics.hip under the CPU SIMT interpreter) on numpy buffers against the fp64 oracle:
the size / layout / C / N / window grid with clamping on and off, unwritten outputs, bit-reproducibility, the border
pixels of the squared error, the argument errors, and the Python layer (scnerf_amd.metrics) on top of the same library.

Bounds (tests/metrics_reference.py): the kernel's error against fp64 may be max(4 E32, 2^-22), E32 the error of the
definition evaluated op by op in fp32 with conv2d, measured here on the same images, per class; MSE to 2^-21 relative."""
import numpy as np
import pytest
import torch

from tests import metrics_reference as R
from tests.emu import harness as H

pytestmark = pytest.mark.emu
EINVAL = -22


def memory(t, layout):
    """-> (the numpy buffer holding t in `layout`, the element strides of its [N, C, H, W] view)"""
    if layout == "nhwc":
        base = t.permute(0, 2, 3, 1).contiguous()
        return base.numpy(), base.permute(0, 3, 1, 2).stride()
    base = t.contiguous()
    return base.numpy(), base.stride()


def run(xm, xs, ym, ys, n, c, h, w, g, clip, want_map=True, status=False):
    win = len(g)
    oh, ow = max(h - win + 1, 1), max(w - win + 1, 1)
    ssim = np.full(max(n, 1), np.nan, np.float32)
    mse = np.full(max(n, 1), np.nan, np.float32)
    ss = np.full((max(n, 1), max(c, 1), oh, ow), np.nan, np.float32) if want_map else None
    floats = H.lib().scnerf_image_metrics_workspace_floats(n, c, h, w, win)
    ws = np.full(max(int(floats), 2), np.nan, np.float32)
    args = (xm, *xs, ym, *ys, n, c, h, w, g, win, R.C1, R.C2, R.VALUE_RANGE, int(clip), ssim, mse, ss, ws, None)
    if status:
        return H.lib_call_status("scnerf_image_metrics", *args)
    H.call("scnerf_image_metrics", *args)
    return ssim[:n], mse[:n], ss


def check_against_oracle(d, got, n, c, e_value, e_map, what):
    ssim, mse, ss = got
    h, w = d["x"].shape[-2:]
    assert np.isfinite(ssim).all() and np.isfinite(mse).all() and np.isfinite(ss).all(), what + ": an output was not written"
    want = R.ssim_of(d["per_channel"], n, c).numpy()
    err = float(np.abs(ssim.astype(np.float64) - want).max())
    print("%s: ssim err %.3g (bound %.3g)" % (what, err, R.bound(e_value)))
    assert err <= R.bound(e_value), (what, err, R.bound(e_value))
    err_map = float(np.abs(ss.astype(np.float64) - d["map"][:n, :c].numpy()).max())
    assert err_map <= R.bound(e_map), (what, "map", err_map, R.bound(e_map))
    want_mse = (d["sse"][:n, :c].sum(1) / (c * h * w)).numpy()
    rel = float((np.abs(mse.astype(np.float64) - want_mse) / want_mse).max())
    assert rel <= R.MSE_RTOL, (what, "mse", rel)


@pytest.mark.parametrize("case", R.CASES, ids=lambda k: "win%d-%dx%d-clip%d" % k)
@pytest.mark.parametrize("cls", R.CLASSES)
def test_grid_against_oracle(cls, case):
    win, h, w, clip = case
    d = R.case_data(cls, *case)
    e_value, e_map = R.yardstick(cls)
    for lx, ly in R.LAYOUTS:
        xm, xs = memory(d["x"], lx)
        ym, ys = memory(d["y"], ly)
        for c in (1, 3):
            for n in (1, 2):
                got = run(xm, xs, ym, ys, n, c, h, w, d["taps"], clip)
                check_against_oracle(d, got, n, c, e_value, e_map, "%s %s x=%s y=%s C=%d N=%d" % (cls, case, lx, ly, c, n))


def test_identical_images_give_one():
    for cls in R.CLASSES:
        x, _ = R.images(cls, 2, 3, 43, 75)
        xm, xs = memory(x, "nchw")
        ym, ys = memory(x, "nhwc")
        ssim, mse, ss = run(xm, xs, ym, ys, 2, 3, 43, 75, R.taps(11), False)
        assert np.abs(ssim - 1.0).max() <= 2.0 ** -23 and np.abs(ss - 1.0).max() <= 2.0 ** -23
        assert (mse == 0).all()


def test_two_calls_and_batch_against_singles_are_bit_identical():
    d = R.case_data("noise", 11, 43, 75, False)
    for layout in ("nchw", "nhwc"):
        xm, xs = memory(d["x"], layout)
        ym, ys = memory(d["y"], "nhwc")
        a = run(xm, xs, ym, ys, 2, 3, 43, 75, d["taps"], False)
        b = run(xm, xs, ym, ys, 2, 3, 43, 75, d["taps"], False)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
        for i in range(2):
            xi, xis = memory(d["x"][i:i + 1], layout)
            yi, yis = memory(d["y"][i:i + 1], "nhwc")
            s, m, ss = run(xi, xis, yi, yis, 1, 3, 43, 75, d["taps"], False)
            assert s.tobytes() == a[0][i:i + 1].tobytes() and m.tobytes() == a[1][i:i + 1].tobytes()
            assert ss.tobytes() == a[2][i:i + 1].tobytes()


@pytest.mark.parametrize("h,w", [(43, 75), (42, 42), (11, 11)])
def test_squared_error_counts_the_border(h, w):
    """x and y differ ONLY in the last win - 1 rows and columns, which start no window"""
    x, _ = R.images("noise", 2, 3, h, w)
    y = x.clone()
    delta = torch.rand((2, 3, h, w), generator=torch.Generator().manual_seed(5)) * 0.5 + 0.1
    border = torch.zeros(h, w, dtype=torch.bool)
    border[h - 10:, :] = True
    border[:, w - 10:] = True
    y[..., border] -= delta[..., border]
    want = ((x.double() - y.double()) ** 2).sum((1, 2, 3)) / (3 * h * w)
    assert float(want.min()) > 0
    for layout in ("nchw", "nhwc"):
        xm, xs = memory(x, layout)
        ym, ys = memory(y, layout)
        _, mse, _ = run(xm, xs, ym, ys, 2, 3, h, w, R.taps(11), False, want_map=False)
        assert float((np.abs(mse - want.numpy()) / want.numpy()).max()) <= R.MSE_RTOL


def test_map_is_optional_and_other_windows_run():
    x, y = R.images("smooth", 1, 3, 40, 37)
    xm, xs = memory(x, "nhwc")
    ym, ys = memory(y, "nchw")
    for win in (3, 5, 9):
        g = R.taps(win)
        with_map = run(xm, xs, ym, ys, 1, 3, 40, 37, g, False)
        without = run(xm, xs, ym, ys, 1, 3, 40, 37, g, False, want_map=False)
        assert without[2] is None and with_map[0].tobytes() == without[0].tobytes()
        per_channel, ss, _ = R.oracle(x, y, g)
        e = float((R.fp32_formulation(x, y, g)[1].double() - ss).abs().max())
        assert float(np.abs(with_map[2] - ss.numpy()).max()) <= R.bound(e)


def test_argument_errors_and_empty_batch():
    x, y = R.images("noise", 1, 3, 16, 16)
    xm, xs = memory(x, "nchw")
    ym, ys = memory(y, "nchw")
    g = R.taps(11)
    ok = lambda **k: dict(dict(xm=xm, xs=xs, ym=ym, ys=ys, n=1, c=3, h=16, w=16, g=g, clip=False), **k)
    assert run(status=True, **ok()) == 0
    assert run(status=True, want_map=False, **ok()) == 0
    for bad in (dict(h=10), dict(w=10), dict(n=-1), dict(c=-1), dict(c=0), dict(g=np.ones(10, np.float32)),
                dict(g=np.ones(13, np.float32)), dict(g=np.ones(1, np.float32)), dict(g=np.ones(2, np.float32))):
        assert run(status=True, **ok(**bad)) == EINVAL, bad
    # null pointers, one at a time (positions in the argument list: x, y, taps, ssim, mse, workspace)
    ssim, mse, ws = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(64, np.float32)
    base = [xm, *xs, ym, *ys, 1, 3, 16, 16, g, 11, R.C1, R.C2, 1.0, 0, ssim, mse, None, ws, None]
    assert H.lib_call_status("scnerf_image_metrics", *base) == 0
    for pos in (0, 5, 14, 20, 21, 23):
        args = list(base)
        args[pos] = None
        assert H.lib_call_status("scnerf_image_metrics", *args) == EINVAL, pos
    # n == 0: a successful no-op that writes nothing
    ssim, mse, ss = run(**ok(n=0))
    assert ssim.size == 0 and np.isnan(ss).all()
    assert H.lib().scnerf_image_metrics_workspace_floats(0, 3, 16, 16, 11) == 0
    assert H.lib().scnerf_image_metrics_workspace_floats(2, 3, 43, 75, 11) == 2 * 3 * 2 * 3 * 4


def test_python_layer_on_the_interpreter():
    """scnerf_amd.metrics (module, functional form, image_metrics) over the same library on CPU tensors"""
    from scnerf_amd import metrics
    from tests.emu.host_on_emu import emulated_device
    d = R.case_data("noise", 11, 43, 75, True)
    x, y = d["x"], d["y"]
    want = R.ssim_of(R.oracle(x, y, d["taps"])[0], 2, 3)
    e_value, e_map = R.yardstick("noise")
    with emulated_device():
        per_image = metrics.SSIM(reduction="none")(x, y)
        assert float((per_image.double() - want).abs().max()) <= R.bound(e_value)
        assert torch.equal(metrics.SSIM()(x, y), per_image.mean()) and torch.equal(metrics.SSIM(reduction="sum")(x, y), per_image.sum())
        s, m = metrics.ssim(R.channel_last(x), y, return_map=True)
        assert torch.equal(s, per_image) and m.shape == (2, 3, 33, 65)
        s7 = metrics.ssim(x, y, window_size=7)
        assert float((s7.double() - R.ssim_of(R.oracle(x, y, R.taps(7))[0], 2, 3)).abs().max()) <= R.bound(e_value)
        rgb, gt = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
        out = metrics.image_metrics(rgb, gt)
        assert sorted(out) == ["mse", "psnr", "ssim"] and all(v.shape == (2,) for v in out.values())
        clipped = R.ssim_of(d["per_channel"], 2, 3)
        assert float((out["ssim"].double() - clipped).abs().max()) <= R.bound(e_value)
        want_mse = d["sse"].sum(1) / (3 * 43 * 75)
        assert float(((out["mse"].double() - want_mse) / want_mse).abs().max()) <= R.MSE_RTOL
        from scnerf_amd.run_nerf_helpers import mse2psnr
        assert torch.equal(out["psnr"], mse2psnr(out["mse"]))
        one = metrics.image_metrics(rgb[1], gt[1])
        assert all(one[k].shape == () and torch.equal(one[k], out[k][1]) for k in out)
        unclipped = metrics.image_metrics(rgb, gt, clip=False)
        assert torch.equal(unclipped["mse"], out["mse"]) and not torch.equal(unclipped["ssim"], out["ssim"])
        with pytest.raises(NotImplementedError, match="forward-only"):
            metrics.SSIM()(x.clone().requires_grad_(True), y)
        with torch.no_grad():
            metrics.SSIM()(x.clone().requires_grad_(True), y)
        with pytest.raises(ValueError):
            metrics.ssim(x[:, :, :8], y[:, :, :8])
        with pytest.raises(TypeError):
            metrics.ssim(x.double(), y.double())
    with pytest.raises(RuntimeError):
        metrics.SSIM()(x, y)                       # outside the context these are CPU tensors
