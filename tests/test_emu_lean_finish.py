"""The lean weight-gradient group's finishing kernel (csrc/wgrad.hip wgrad_lean_finish_kernel, HIP source under the CPU
SIMT interpreter) against the numpy fp64 products: from M = sum_p dZv_p act7_p^T and s = sum_p dZv_p it forms
d views_linears.0.weight[:, :256] = M W_f^T + s b_f^T, d feature_linear.weight = W_vf^T M, d feature_linear.bias =
W_vf^T s and d views_linears.0.bias = s, written or added into the flat gradient; nothing else is touched."""
import numpy as np
import pytest

from scnerf_amd import mlp_layout as ML
from tests.emu import harness as H

pytestmark = pytest.mark.emu

OFF = ML.PARAM_OFFSETS
N = ML.layout(3).n_params


def _case(seed):
    rng = np.random.default_rng(seed)
    params = (rng.standard_normal(N) * 0.1).astype(np.float32)
    M = rng.standard_normal((128, 256)).astype(np.float32) * 30.0
    s = rng.standard_normal(128).astype(np.float32) * 5.0
    W_f = params[OFF["feature_linear.weight"]:][:256 * 256].reshape(256, 256).astype(np.float64)
    b_f = params[OFF["feature_linear.bias"]:][:256].astype(np.float64)
    W_v = params[OFF["views_linears.0.weight"]:][:128 * 283].reshape(128, 283).astype(np.float64)
    W_vf = W_v[:, :256]
    M64, s64 = M.astype(np.float64), s.astype(np.float64)
    ref = {"wv": M64 @ W_f.T + np.outer(s64, b_f), "wf": W_vf.T @ M64, "bf": W_vf.T @ s64, "bv": s64}
    return params, M, s, ref


def _targets(g):
    wv = g[OFF["views_linears.0.weight"]:][:128 * 283].reshape(128, 283)
    return {"wv": wv[:, :256], "wf": g[OFF["feature_linear.weight"]:][:256 * 256].reshape(256, 256),
            "bf": g[OFF["feature_linear.bias"]:][:256], "bv": g[OFF["views_linears.0.bias"]:][:128]}


def _touched():
    m = np.zeros(N, bool)
    wv = m[OFF["views_linears.0.weight"]:][:128 * 283].reshape(128, 283)
    wv[:, :256] = True
    for name, n in (("feature_linear.weight", 256 * 256), ("feature_linear.bias", 256), ("views_linears.0.bias", 128)):
        m[OFF[name]:OFF[name] + n] = True
    return m


@pytest.mark.parametrize("accumulate", [0, 1])
def test_finishing_kernel_matches_fp64_products(accumulate):
    params, M, s, ref = _case(11 + accumulate)
    before = np.random.default_rng(5).standard_normal(N).astype(np.float32)
    g = before.copy()
    H.call("scnerf_wgrad_lean_finish", M, s, params, g, accumulate, None)
    touched = _touched()
    np.testing.assert_array_equal(g[~touched], before[~touched])          # (the encoded-direction columns among them)
    got, was = _targets(g), _targets(before)
    for k in ("wv", "wf", "bf", "bv"):
        # one rounding of the fp64 product to fp32, and with `accumulate` one fp32 addition to what was there; numpy sums
        # its fp64 products in another order, so a value on a rounding boundary may land one fp32 step away
        r32 = ref[k].astype(np.float32)
        want = was[k] + r32 if accumulate else r32
        err = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
        assert (err <= 2.0 ** -23 * (np.abs(r32) + np.abs(want))).all(), (k, float(err.max()))
