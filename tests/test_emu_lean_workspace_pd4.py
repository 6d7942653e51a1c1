"""The lean workspace for 4-D points (the NeRF++ background network) under the CPU SIMT interpreter -- the pt_dims = 4 twin
of test_emu_lean_workspace.py and test_emu_lean_finish.py: the resident forward and data gradients with the lean flag
leave everything but the feature / d feature sections as the full pass does, the lean weight-gradient group reproduces the
full group's gradients (bit for bit outside the three derived tensors, to fp32 rounding inside them), and the finishing
kernel reads and writes its tensors at the 4-D layout's offsets (scnerf_wgrad_lean_finish_pd), the legacy symbol staying
its pt_dims = 3 case."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests.emu import harness as H
from tests.emu_mlp_util import flat_params, grad_views, network_params, pack_backward, pack_forward, pack_h3, save_views

pytestmark = pytest.mark.emu

PD = 4
LAY = ML.layout(PD)
OFF = LAY.param_offsets
N = LAY.n_params
NO_GUARD = (None, None, None)


def _run(lean, P, spr, chunks, pts, vd, d_raw, p):
    lib = H.lib()
    wpk, wbk = pack_forward(p, PD), pack_backward(p, PD)
    fwd, bwd, sc = pack_h3(p, PD)
    nb = lib.scnerf_wgrad256_chunks(chunks)
    cs = lib.scnerf_wgrad_chunk_samples(P, nb)
    mx, mz = np.zeros((12, nb), np.float32), np.zeros((12, nb), np.float32)
    raw = np.zeros((P, 4), np.float32)
    save = np.full(LAY.save_floats(P), np.nan, np.float32)
    H.call("scnerf_mlp_fwd_h3_lean", PD, pts, vd, 3, spr, wpk, fwd, sc, raw, save, P, mx, nb, cs, *NO_GUARD, lean, None)
    grads = np.full(ML.grad_floats(P), np.nan, np.float32)
    d_pts, d_views = np.full((P, PD), np.nan, np.float32), np.full((P, 3), np.nan, np.float32)
    H.call("scnerf_mlp_bwd_h3_lean", PD, d_raw, pts, vd, 3, spr, wbk, bwd, sc, save, grads, d_pts, d_views, P, mz, nb, cs,
           *NO_GUARD, lean, None)
    ws = np.full(lib.scnerf_nerf_wgrad_workspace_floats(chunks), np.nan, np.float32)
    g = np.full(N, np.nan, np.float32)
    if lean:
        H.call("scnerf_nerf_wgrad_h3_lean", PD, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, flat_params(p, PD), None, None, None)
    else:
        H.call("scnerf_nerf_wgrad_h3", PD, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, None, None, None)
    return dict(raw=raw, save=save, grads=grads, d_pts=d_pts, d_views=d_views, mx=mx, mz=mz, g=g)


def test_lean_pass_and_lean_group_against_the_full_ones_pd4():
    n_rays, spr, chunks = 5, 34, 2                 # 170 samples: a partial 128-block; two chunks per job
    P = n_rays * spr
    p = network_params(3, PD)
    gen = torch.Generator().manual_seed(17)
    unit = torch.nn.functional.normalize(torch.randn(P, 3, generator=gen), dim=-1)
    inv_r = 1.0 - torch.rand(P, 1, generator=gen)                    # (0, 1]
    pts = torch.cat([unit, inv_r], -1).contiguous().numpy()
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).numpy()
    d_raw = torch.randn(P, 4, generator=gen).numpy()
    full = _run(0, P, spr, chunks, pts, vd, d_raw, p)
    lean = _run(1, P, spr, chunks, pts, vd, d_raw, p)
    Pp = ML.padded_samples(P)
    for k in ("raw", "d_pts", "d_views", "mx", "mz"):
        assert not np.isnan(full[k]).any(), k
        np.testing.assert_array_equal(full[k].view(np.int32), lean[k].view(np.int32), err_msg=k)
    so, total = ML.section_offsets(LAY.save_sections, P)
    for name, w in LAY.save_sections:
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
    derived = np.zeros(N, bool)
    derived[OFF["feature_linear.weight"]:OFF["feature_linear.weight"] + 256 * 256] = True
    derived[OFF["feature_linear.bias"]:OFF["feature_linear.bias"] + 256] = True
    derived[OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)[:, :256] = True
    assert np.isfinite(full["g"]).all() and np.isfinite(lean["g"]).all()
    np.testing.assert_array_equal(full["g"].view(np.int32)[~derived], lean["g"].view(np.int32)[~derived])
    sv, gv = save_views(full["save"], P, PD), grad_views(full["grads"], P)
    act7, feat = sv["act7"].astype(np.float64), sv["feat"].astype(np.float64)
    dzv, dfeat = gv["dzv"].astype(np.float64), gv["dfeat"].astype(np.float64)
    ref = {"feature_linear.weight": dfeat.T @ act7, "feature_linear.bias": dfeat.sum(0), "views": dzv.T @ feat}
    wv = lean["g"][OFF["views_linears.0.weight"]:OFF["views_linears.0.weight"] + 128 * 283].reshape(128, 283)
    got = {"feature_linear.weight": lean["g"][OFF["feature_linear.weight"]:][:256 * 256].reshape(256, 256),
           "feature_linear.bias": lean["g"][OFF["feature_linear.bias"]:][:256], "views": wv[:, :256]}
    for k in ref:
        # (test_emu_lean_workspace.py's rule -- fp32 sums over 170 samples and fp32 `feature` / `d feature` on the full side:
        # a few 1e-7 of the largest entry)
        assert np.abs(got[k] - ref[k]).max() <= 2e-6 * np.abs(ref[k]).max(), (k, np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max())


# ---- the finishing kernel at the 4-D layout's offsets ---------------------------------------------------------------------
def _case(seed, off, n):
    rng = np.random.default_rng(seed)
    params = (rng.standard_normal(n) * 0.1).astype(np.float32)
    M = rng.standard_normal((128, 256)).astype(np.float32) * 30.0
    s = rng.standard_normal(128).astype(np.float32) * 5.0
    W_f = params[off["feature_linear.weight"]:][:256 * 256].reshape(256, 256).astype(np.float64)
    b_f = params[off["feature_linear.bias"]:][:256].astype(np.float64)
    W_v = params[off["views_linears.0.weight"]:][:128 * 283].reshape(128, 283).astype(np.float64)
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
def test_finishing_kernel_matches_fp64_products_pd4(accumulate):
    assert OFF["feature_linear.weight"] != ML.PARAM_OFFSETS["feature_linear.weight"]       # (the offsets under test differ)
    params, M, s, ref = _case(11 + accumulate, OFF, N)
    before = np.random.default_rng(5).standard_normal(N).astype(np.float32)
    g = before.copy()
    H.call("scnerf_wgrad_lean_finish_pd", PD, M, s, params, g, accumulate, None)
    touched = _touched()
    np.testing.assert_array_equal(g[~touched], before[~touched])          # (the encoded-direction columns among them)
    got, was = _targets(g), _targets(before)
    for k in ("wv", "wf", "bf", "bv"):
        # test_emu_lean_finish.py's bound: one rounding of the fp64 product to fp32, and with `accumulate` one fp32 addition to
        # what was there; numpy sums its fp64 products in another order, so a value on a rounding boundary may land one fp32
        # step away
        r32 = ref[k].astype(np.float32)
        want = was[k] + r32 if accumulate else r32
        err = np.abs(got[k].astype(np.float64) - want.astype(np.float64))
        assert (err <= 2.0 ** -23 * (np.abs(r32) + np.abs(want))).all(), (k, float(err.max()))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_legacy_symbol_is_the_pd3_case(accumulate):
    n3 = ML.layout(3).n_params
    params, M, s, _ = _case(23 + accumulate, ML.PARAM_OFFSETS, n3)
    before = np.random.default_rng(6).standard_normal(n3).astype(np.float32)
    a, b = before.copy(), before.copy()
    H.call("scnerf_wgrad_lean_finish", M, s, params, a, accumulate, None)
    H.call("scnerf_wgrad_lean_finish_pd", 3, M, s, params, b, accumulate, None)
    assert not np.array_equal(a, before)
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_the_pd_entry_point_refuses_other_point_dimensions():
    params, M, s, _ = _case(31, OFF, N)
    g = np.zeros(N, np.float32)
    assert H.lib_call_status("scnerf_wgrad_lean_finish_pd", 5, M, s, params, g, 0, None) != 0
    assert not g.any()
