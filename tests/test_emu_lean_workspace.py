"""The lean workspace end to end under the CPU SIMT interpreter (the kernels' own sources): the resident forward and data
gradients with the lean flag leave everything but the feature / d feature sections as the full pass does, and the lean
weight-gradient group (seven big jobs, the views layer's narrow GEMM on act7, the finishing kernel) reproduces the full
group's gradients -- bit for bit outside the three derived tensors, to fp32 rounding inside them.  (The accuracy statement
proper is the GPU test's, tests/test_gpu_lean_workspace.py: the interpreter is sequentially consistent and has no matrix pipe.)"""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests.emu import harness as H
from tests.emu_mlp_util import flat_params, grad_views, network_params, pack_backward, pack_forward, pack_h3, save_views

pytestmark = pytest.mark.emu

OFF = ML.PARAM_OFFSETS
NO_GUARD = (None, None, None)


def _run(lean, P, spr, chunks, pts, vd, d_raw, p):
    lay = ML.layout(3)
    lib = H.lib()
    wpk, wbk = pack_forward(p, 3), pack_backward(p, 3)
    fwd, bwd, sc = pack_h3(p, 3)
    nb = lib.scnerf_wgrad256_chunks(chunks)
    cs = lib.scnerf_wgrad_chunk_samples(P, nb)
    mx, mz = np.zeros((12, nb), np.float32), np.zeros((12, nb), np.float32)
    raw = np.zeros((P, 4), np.float32)
    save = np.full(lay.save_floats(P), np.nan, np.float32)
    H.call("scnerf_mlp_fwd_h3_lean", 3, pts, vd, 3, spr, wpk, fwd, sc, raw, save, P, mx, nb, cs, *NO_GUARD, lean, None)
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    d_pts, d_views = np.full((P, 3), np.nan, np.float32), np.full((P, 3), np.nan, np.float32)
    H.call("scnerf_mlp_bwd_h3_lean", 3, d_raw, pts, vd, 3, spr, wbk, bwd, sc, save, grads, d_pts, d_views, P, mz, nb, cs,
           *NO_GUARD, lean, None)
    ws = np.full(lib.scnerf_nerf_wgrad_workspace_floats(chunks), np.nan, np.float32)
    g = np.full(lay.n_params, np.nan, np.float32)
    if lean:
        H.call("scnerf_nerf_wgrad_h3_lean", 3, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, flat_params(p, 3), None, None, None)
    else:
        H.call("scnerf_nerf_wgrad_h3", 3, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, None, None, None)
    return dict(raw=raw, save=save, grads=grads, d_pts=d_pts, d_views=d_views, mx=mx, mz=mz, g=g)


def test_lean_pass_and_lean_group_against_the_full_ones():
    lay = ML.layout(3)
    n_rays, spr, chunks = 5, 34, 2                 # 170 samples: a partial 128-block; two chunks per job
    P = n_rays * spr
    p = network_params(3, 3)
    gen = torch.Generator().manual_seed(17)
    pts = (torch.rand(P, 3, generator=gen) * 2.4 - 1.2).numpy()
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).numpy()
    d_raw = torch.randn(P, 4, generator=gen).numpy()
    full = _run(0, P, spr, chunks, pts, vd, d_raw, p)
    lean = _run(1, P, spr, chunks, pts, vd, d_raw, p)
    Pp = ML.padded_samples(P)
    for k in ("raw", "d_pts", "d_views", "mx", "mz"):
        np.testing.assert_array_equal(full[k].view(np.int32), lean[k].view(np.int32), err_msg=k)
    so, total = ML.section_offsets(lay.save_sections, P)
    for name, w in lay.save_sections:
        a, b = full["save"][so[name]:so[name] + w * Pp], lean["save"][so[name]:so[name] + w * Pp]
        if name == "feat":
            assert np.isnan(b).all() and not np.isnan(a).any()
        else:
            np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=name)
    np.testing.assert_array_equal(full["save"][total:].view(np.int32), lean["save"][total:].view(np.int32))
    go, _ = ML.section_offsets(ML.GRAD_SECTIONS, P)
    for name, w in ML.GRAD_SECTIONS:
        a, b = full["grads"][go[name]:go[name] + w * Pp], lean["grads"][go[name]:go[name] + w * Pp]
        if name == "dfeat":
            assert np.isnan(b).all() and not np.isnan(a).any()
        else:
            np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=name)
    # the weight gradients
    derived = np.zeros(lay.n_params, bool)
    derived[OFF["feature_linear.weight"]:OFF["feature_linear.weight"] + 256 * 256] = True
    derived[OFF["feature_linear.bias"]:OFF["feature_linear.bias"] + 256] = True
    derived[OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)[:, :256] = True
    assert np.isfinite(full["g"]).all() and np.isfinite(lean["g"]).all()
    np.testing.assert_array_equal(full["g"].view(np.int32)[~derived], lean["g"].view(np.int32)[~derived])
    sv, gv = save_views(full["save"], P), grad_views(full["grads"], P)
    act7, feat = sv["act7"].astype(np.float64), sv["feat"].astype(np.float64)
    dzv, dfeat = gv["dzv"].astype(np.float64), gv["dfeat"].astype(np.float64)
    ref = {"feature_linear.weight": dfeat.T @ act7, "feature_linear.bias": dfeat.sum(0), "views": dzv.T @ feat}
    wv = lean["g"][OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)
    got = {"feature_linear.weight": lean["g"][OFF["feature_linear.weight"]:][:256 * 256].reshape(256, 256),
           "feature_linear.bias": lean["g"][OFF["feature_linear.bias"]:][:256], "views": wv[:, :256]}
    for k in ref:
        # fp32 sums over 170 samples and fp32 `feature` / `d feature` on the full side: a few 1e-7 of the largest entry
        assert np.abs(got[k] - ref[k]).max() <= 2e-6 * np.abs(ref[k]).max(), (k, np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())
