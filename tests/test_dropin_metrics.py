"""scnerf_amd.dropin.install_metrics(): piqa's module names resolve to the package's SSIM and to an LPIPS stand-in that
returns NaN -- when, and only when, no piqa is importable."""
import importlib.util
import sys
import types
import warnings

import pytest
import torch

from scnerf_amd import dropin, metrics

NAMES = ("piqa", "piqa.ssim", "piqa.lpips")


@pytest.fixture
def clean_modules():
    saved = {k: sys.modules.get(k) for k in NAMES}
    for k in NAMES:
        sys.modules.pop(k, None)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _real_piqa():
    return importlib.util.find_spec("piqa") is not None


def test_registers_the_three_names_when_piqa_is_absent(clean_modules):
    if _real_piqa():
        assert dropin.install_metrics() == [] and "piqa" not in sys.modules      # a real piqa is never shadowed
        return
    assert dropin.install_metrics() == ["piqa", "piqa.lpips", "piqa.ssim"]
    from piqa.ssim import SSIM
    from piqa.lpips import LPIPS
    import piqa
    assert SSIM is metrics.SSIM and LPIPS is metrics.LPIPSUnavailable and piqa.ssim.SSIM is SSIM
    model = SSIM()                                     # NeRF/run_nerf.py:79 `SSIM_model = SSIM().cuda()`
    assert isinstance(model, torch.nn.Module) and model.taps.shape == (11,) and model.reduction == "mean"
    assert dropin.install_metrics() == []              # a second call finds the names taken and leaves them


def test_a_module_already_registered_is_left_alone(clean_modules):
    theirs = types.ModuleType("piqa")
    sys.modules["piqa"] = theirs
    assert dropin.install_metrics() == []
    assert sys.modules["piqa"] is theirs and "piqa.ssim" not in sys.modules and "piqa.lpips" not in sys.modules


def test_lpips_stand_in_returns_nan_with_one_warning(clean_modules):
    model = metrics.LPIPSUnavailable(network="vgg")    # NeRF/run_nerf.py:80 `LPIPS(network="vgg").cuda()`
    assert isinstance(model, torch.nn.Module) and model.to("cpu") is model
    x = torch.rand(2, 3, 16, 16)
    with pytest.warns(UserWarning, match="LPIPS is not available"):
        v = model(x, x)
    assert v.shape == () and torch.isnan(v)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.isnan(model(x, x))                # the warning is given once
    per_image = metrics.LPIPSUnavailable(reduction="none")
    with pytest.warns(UserWarning):
        assert torch.isnan(per_image(x, x)).all() and per_image(x, x).shape == (2,)


def test_install_is_unchanged_and_does_not_register_the_metrics(clean_modules):
    from scnerf_amd import camera_model
    aliases = list(dropin._MAP) + ["model"]
    saved = {k: sys.modules.get(k) for k in aliases}
    saved_path, saved_flag = list(sys.meta_path), camera_model._PinholeRotNoise.share_matrix_node
    try:
        names = dropin.install()
        assert names == sorted(dropin._MAP) and not any(n.startswith("piqa") for n in names)
        assert not any(k.split(".")[0] == "piqa" for k in sys.modules)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        sys.meta_path[:] = saved_path
        camera_model._PinholeRotNoise.share_matrix_node = saved_flag


def test_sys_modules_is_restored_afterwards():
    """(runs after the tests above in this file: none of them leaves a piqa entry behind that it did not find)"""
    left = [k for k in NAMES if k in sys.modules and getattr(sys.modules[k], "__doc__", "") and "stand-in" in sys.modules[k].__doc__]
    assert left == []
