"""The fp64 SSIM oracle of tests/metrics_reference.py against closed forms, and against piqa where piqa is installed.
These tests check the ORACLE (and the window the product computes); the kernel is held to the oracle in
test_emu_metrics.py and test_gpu_metrics.py."""
import numpy as np
import pytest
import torch

from scnerf_amd import metrics
from tests import metrics_reference as R


@pytest.mark.parametrize("win", [3, 5, 7, 9, 11])
def test_product_window_is_the_oracles(win):
    g = metrics.gaussian_taps(win, 1.5)
    assert g.dtype == np.float32 and g.shape == (win,)
    assert np.array_equal(g, R.taps(win))
    assert abs(float(g.astype(np.float64).sum()) - 1.0) < win * 2.0 ** -24      # each tap rounded once
    assert np.array_equal(g, g[::-1]) and g.argmax() == win // 2


@pytest.mark.parametrize("bad", [2, 4, 1, 13, 0])
def test_product_window_rejects_other_sizes(bad):
    with pytest.raises(ValueError):
        metrics.gaussian_taps(bad)


@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.25, 0.75), (1.0, 0.5), (0.9, 0.9)])
@pytest.mark.parametrize("win", R.WINDOWS)
def test_constant_images_closed_form(a, b, win):
    x = torch.full((1, 2, 20, 17), a)
    y = torch.full((1, 2, 20, 17), b)
    g = R.taps(win)
    s = float(g.astype(np.float64).sum()) ** 2     # the rounded taps sum to 1 only to fp32 accuracy: the 2-D window sums to s, mu = s a
    per_channel, ss, sse = R.oracle(x, y, g)
    a, b = float(x[0, 0, 0, 0]), float(y[0, 0, 0, 0])
    mu_a, mu_b = s * a, s * b
    # variances of a constant: s a^2 - (s a)^2 = s (1 - s) a^2, below 1e-7: the closed form keeps them
    cs = (2 * s * (1 - s) * a * b + R.C2) / (s * (1 - s) * (a * a + b * b) + R.C2)
    want = (2 * mu_a * mu_b + R.C1) / (mu_a ** 2 + mu_b ** 2 + R.C1) * cs
    assert float((ss - want).abs().max()) <= 1e-12
    assert float((per_channel - want).abs().max()) <= 1e-12
    # and the textbook value (taps summing to exactly 1) to the accuracy of that sum
    textbook = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert float((per_channel - textbook).abs().max()) <= 1e-5
    assert float((sse - 20 * 17 * (a - b) ** 2).abs().max()) <= 1e-9


def test_constant_images_with_exact_window():
    """x = a, y = b under a window that sums to exactly 1 (three taps 1/4, 1/2, 1/4): (2ab + c1) / (a^2 + b^2 + c1) to 1e-12"""
    g = np.array([0.25, 0.5, 0.25], np.float32)
    for a, b in ((0.25, 0.75), (1.0, 0.5), (0.0, 1.0), (0.5, 0.5)):
        per_channel, ss, _ = R.oracle(torch.full((2, 3, 9, 12), a), torch.full((2, 3, 9, 12), b), g)
        want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
        assert float((ss - want).abs().max()) <= 1e-12 and float((per_channel - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("cls", R.CLASSES)
def test_symmetry_and_identity(cls):
    x, y = R.images(cls, 2, 3, 25, 31)
    g = R.taps(11)
    a, ma, _ = R.oracle(x, y, g)
    b, mb, _ = R.oracle(y, x, g)
    assert torch.equal(a, b) and torch.equal(ma, mb)
    one, m1, sse = R.oracle(x, x, g)
    assert torch.equal(m1, torch.ones_like(m1)) and torch.equal(one, torch.ones_like(one))
    assert float(sse.abs().max()) == 0.0


@pytest.mark.parametrize("cls", R.CLASSES)
def test_single_window_against_a_double_loop(cls):
    x, y = R.images(cls, 1, 1, 11, 11, seed=3)
    g = R.taps(11).astype(np.float64)
    xa, ya = x[0, 0].double().numpy(), y[0, 0].double().numpy()
    mu_x = mu_y = e_xx = e_yy = e_xy = 0.0
    for i in range(11):
        for j in range(11):
            wgt = g[i] * g[j]
            mu_x += wgt * xa[i, j]
            mu_y += wgt * ya[i, j]
            e_xx += wgt * xa[i, j] ** 2
            e_yy += wgt * ya[i, j] ** 2
            e_xy += wgt * xa[i, j] * ya[i, j]
    s_xx, s_yy, s_xy = e_xx - mu_x ** 2, e_yy - mu_y ** 2, e_xy - mu_x * mu_y
    want = (2 * mu_x * mu_y + R.C1) / (mu_x ** 2 + mu_y ** 2 + R.C1) * (2 * s_xy + R.C2) / (s_xx + s_yy + R.C2)
    per_channel, ss, _ = R.oracle(x, y, R.taps(11))
    assert ss.shape == (1, 1, 1, 1)
    # fp64 sums of 121 terms in another order; the variances cancel up to 1e4-fold in the bright class
    assert abs(float(ss) - want) <= 1e-10 and abs(float(per_channel) - want) <= 1e-10


def test_clip_applies_to_ssim_only():
    x, y = R.images("noise", 1, 3, 20, 20, overshoot=True)
    assert float(x.max()) > 1.0 and float(x.min()) < 0.0
    g = R.taps(11)
    a, _, sse_a = R.oracle(x, y, g, clip=True)
    b, _, sse_b = R.oracle(x.clamp(0, 1), y, g, clip=False)
    assert torch.equal(a, b)
    assert torch.equal(sse_a, ((x.double() - y.double()) ** 2).sum((2, 3))) and not torch.equal(sse_a, sse_b)


@pytest.mark.parametrize("cls", R.CLASSES)
def test_fp32_formulation_tracks_the_oracle(cls):
    """the yardstick is the same definition: its error is rounding-sized"""
    e_value, e_map = R.yardstick(cls)
    assert 0.0 < e_value < 1e-3 and 0.0 < e_map < 1e-2


def test_against_piqa():
    """The definition is transcribed from piqa's documentation; wherever piqa is installed this pins it.  piqa evaluated in
    fp64 differs from the oracle only through its window, computed in fp32 (each tap within a few 2^-24 of ours): on the noise
    class (variances around 0.08) that moves ss by about 11 x 1e-7 / 0.16 < 1e-5.
    Only the REAL piqa counts: stand-ins that other tests of the same process left in sys.modules (tests/dropin_support.py's
    zero metric, dropin.install_metrics()'s modules; neither has a file) are set aside for the import and put back."""
    import sys
    aside = {k: m for k, m in sys.modules.items()
             if k.split(".")[0] == "piqa" and not getattr(m, "__file__", None)}
    for k in aside:
        del sys.modules[k]
    try:
        piqa_ssim = pytest.importorskip("piqa.ssim")
        x, y = R.images("noise", 2, 3, 43, 75)
        want = R.ssim_of(R.oracle(x, y, R.taps(11))[0], 2, 3)
        got = piqa_ssim.SSIM(reduction="none").double()(x.double(), y.double())
        assert float((got - want).abs().max()) <= 1e-5
    finally:
        sys.modules.update(aside)
