"""TEST INFRASTRUCTURE: the yardstick of the one-product arithmetic (ops.inference_arithmetic("fast"); csrc/mlp_fwd_h3_kernel.h,
PRODUCTS == 1) -- the network (NeRF/run_nerf_helpers.py:105-128 behind run_network, NeRF/create_nerf.py:18-32) evaluated in
double precision twice:

  plain    every product exact
  model    every operand of a matrix product first rounded to fp16 after scaling by a power of two -- per SAMPLE for the
           activations (the one that puts the sample's largest input entry in [2^11, 2^12)), per LAYER for the weights (the
           same rule on the layer's largest weight) -- and the accumulation exact

The model states "one fp16 product per product" without copying the kernel's scale rule (a bound-derived power of two,
csrc/mlp_h3.h:18-26): fp16 rounding is relative, so the choice of the power of two matters only for entries more than 2^-11
below the sample's maximum.  Errors are taken per `raw` column, as maximum and as rms over the samples, normalised by the
column's largest plain magnitude."""
import numpy as np
import torch

from oracle import scnerf_oracle as O


def _pow2_scale(amax):
    """the power of two s with amax * s in [2^11, 2^12) (1 where amax == 0)"""
    amax = np.asarray(amax, np.float64)
    e = np.floor(np.log2(np.where(amax > 0, amax, 1.0)))
    return np.where(amax > 0, np.exp2(11.0 - e), 1.0)


def _round_f16(x, s):
    return (x * s).astype(np.float16).astype(np.float64) / s


def _linear(x, w, b, rounded):
    """x [P, K] @ w [N, K]^T + b in fp64; `rounded`: both operands through fp16 first (per-sample / per-layer scale)"""
    if rounded:
        x = _round_f16(x, _pow2_scale(np.abs(x).max(1, keepdims=True)))
        w = _round_f16(w, _pow2_scale(np.abs(w).max()))
    return x @ w.T + b


def network_fp64(p, pts, viewdirs, samples_per_ray, rounded):
    """raw [P, 4] (rgb logits, sigma) in fp64.  p: name -> tensor (the NeRF names), pts [P, pd], viewdirs [n_rays, 3]."""
    P = pts.shape[0]
    W = lambda name: p[name].detach().cpu().double().numpy()
    e = O.positional_encoding(torch.as_tensor(pts).double(), 10).numpy()
    vd = torch.as_tensor(viewdirs).double()
    vd = vd[:, None, :].expand(vd.shape[0], samples_per_ray, 3).reshape(P, 3)
    ev = O.positional_encoding(vd, 4).numpy()
    h = e
    for i in range(8):
        h = np.maximum(_linear(h, W("pts_linears.%d.weight" % i), W("pts_linears.%d.bias" % i), rounded), 0.0)
        if i == 4:
            h = np.concatenate([e, h], -1)
    sigma = _linear(h, W("alpha_linear.weight"), W("alpha_linear.bias"), rounded)
    feat = _linear(h, W("feature_linear.weight"), W("feature_linear.bias"), rounded)
    hv = np.maximum(_linear(np.concatenate([feat, ev], -1), W("views_linears.0.weight"), W("views_linears.0.bias"), rounded), 0.0)
    rgb = _linear(hv, W("rgb_linear.weight"), W("rgb_linear.bias"), rounded)
    return np.concatenate([rgb, sigma], -1)


class Yardstick:
    """plain and model chains of one (network, inputs) case, computed once; errors(raw) -> {"max": [4], "rms": [4]}"""

    def __init__(self, p, pts, viewdirs, samples_per_ray):
        self.plain = network_fp64(p, pts, viewdirs, samples_per_ray, False)
        self.model = network_fp64(p, pts, viewdirs, samples_per_ray, True)
        self.size = np.abs(self.plain).max(0)
        self.err_model = self.errors(self.model)

    def errors(self, raw):
        d = np.asarray(raw, np.float64).reshape(self.plain.shape) - self.plain
        return {"max": np.abs(d).max(0) / self.size, "rms": np.sqrt((d * d).mean(0)) / self.size}


# err_fast <= MARGIN x err_model, per column, maximum and rms.  The largest ratio measured on the CPU SIMT interpreter over
# the cases of tests/test_emu_mlp_fast.py is recorded in DESIGN.md ("One-product inference"); the margin is the next power
# of two above it.  It covers the maximum norm over a few hundred outputs and the kernel's fp32 accumulation, which the
# model's exact sums do not have.  A ratio above 4 would be a bug in the kernel, not a reason for a larger margin.
MARGIN = 2.0
# err_fast >= this x err_resident (rms): the proof that the call ran ONE product -- far below the 2^11 that separates the
# two arithmetics, far above noise
SEPARATION = 10.0


def check(y, raw_fast, raw_resident, what=""):
    """the two network-level assertions; -> the figures (printed by the callers before they assert)"""
    ef, er = y.errors(raw_fast), y.errors(raw_resident)
    ratio = {k: ef[k] / y.err_model[k] for k in ("max", "rms")}
    sep = ef["rms"] / er["rms"]
    print("%s err_model max %s rms %s | err_fast max %s rms %s | err_resident rms %s | fast/model max %s rms %s | fast/resident rms %s"
          % (what, y.err_model["max"], y.err_model["rms"], ef["max"], ef["rms"], er["rms"], ratio["max"], ratio["rms"], sep))
    assert np.all(ef["max"] <= MARGIN * y.err_model["max"]), (what, "max", ratio["max"])
    assert np.all(ef["rms"] <= MARGIN * y.err_model["rms"]), (what, "rms", ratio["rms"])
    assert np.all(sep >= SEPARATION), (what, sep)
    return {"ratio_max": float(ratio["max"].max()), "ratio_rms": float(ratio["rms"].max()), "separation": float(sep.min())}
