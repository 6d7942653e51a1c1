"""csrc/live_compact.hip under the CPU SIMT interpreter, through the C ABI on numpy buffers, against the numpy restatement
of tests/live_samples_ref.py (the GPU twin is tests/test_gpu_live_samples.py): the compaction -- index list, offset table,
count, gathered d_raw -- the gathered masks, points and view directions, the scatter back to sample order and the remap of
the X chunk maxima.  Then one small pass end to end: the unchanged data-gradient kernel on the compact batch writes the
dense launch's dZ rows of the live samples bit for bit, and the weight-gradient group over compact dZ and gathered X
reproduces the dense group (alpha_linear / rgb_linear bit for bit, the GEMMs to fp32 rounding of a differently cut sum)."""
import numpy as np
import pytest
import torch

from scnerf_amd import mlp_layout as ML
from tests import live_samples_ref as R
from tests.emu import harness as H
from tests.emu_mlp_util import flat_params, grad_views, network_params, pack_backward, pack_forward, pack_h3

pytestmark = pytest.mark.emu
EINVAL = -22
NO_GUARD = (None, None, None)


def _compact(d_raw):
    P = d_raw.shape[0]
    Pp = ML.padded_samples(P)
    lib = H.lib()
    ws = np.full(lib.scnerf_live_compact_workspace_ints(P), -1, np.int32)
    idx, xoff = np.full(Pp, -7, np.int32), np.full(Pp, 0xFFFFFFFF, np.uint32)
    live = np.full((P, 4), np.nan, np.float32)
    n_dev, n_host = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    H.call("scnerf_live_compact", d_raw, P, ws, idx, xoff, live, n_dev, n_host, None)
    assert n_dev[0] == n_host[0]
    return idx, xoff, live, int(n_dev[0])


@pytest.mark.parametrize("P", [300, 2500])
def test_compaction_and_gather_equal_the_numpy_restatement(P):
    lay = ML.layout(3)
    Pp = ML.padded_samples(P)
    rng = np.random.default_rng(P)
    spr = 25
    pts = rng.standard_normal((P, 3)).astype(np.float32)
    rays = rng.standard_normal((P // spr, 11)).astype(np.float32)               # the directions are columns 8 .. 10: row stride 11
    vd = rays[:, 8:11]
    masks = rng.integers(0, 2 ** 32, ML.MASK_WORDS_PER_SAMPLE * Pp, dtype=np.uint32)
    for name, live in R.patterns(P).items():
        d_raw = R.d_raw_with(live)
        want = R.live_index(d_raw)
        assert np.array_equal(want, np.flatnonzero(live)), name
        idx, xoff, d_live, n = _compact(d_raw)
        Pl = ML.padded_samples(n)
        assert n == len(want), name
        np.testing.assert_array_equal(idx[:Pl], R.padded_index(want, P), err_msg=name)
        np.testing.assert_array_equal(xoff[:Pl], R.xoff_table(want), err_msg=name)
        assert (idx[Pl:] == -7).all() and (xoff[Pl:] == 0xFFFFFFFF).all(), name        # nothing behind the padded count
        np.testing.assert_array_equal(d_live[:n].view(np.uint32), d_raw[want].view(np.uint32), err_msg=name)
        assert np.isnan(d_live[n:]).all(), name
        if n == 0:
            continue
        m_l = np.full(ML.MASK_WORDS_PER_SAMPLE * Pl, 0xDEADBEEF, np.uint32)
        p_l, v_l = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
        H.call("scnerf_live_gather", idx, n, P, masks, pts, 3, rays.reshape(-1)[8:], 11, spr, m_l, p_l, v_l, None)
        np.testing.assert_array_equal(m_l, R.gather_masks(masks, P, want), err_msg=name)
        np.testing.assert_array_equal(p_l, pts[want], err_msg=name)
        np.testing.assert_array_equal(v_l, vd[want // spr], err_msg=name)
        back = np.full((P, 3), np.nan, np.float32)
        H.call("scnerf_live_scatter_rows", p_l, idx, back, n, 3, P, None)
        ref = np.zeros((P, 3), np.float32)
        ref[want] = pts[want]
        np.testing.assert_array_equal(back, ref, err_msg=name)


def test_remapped_maxima_bound_every_compact_chunk():
    P, n_src, chunk_src, n_dst, chunk_dst = 2500, 5, 512, 4, 480
    live = R.patterns(P)["random"]
    idx = R.padded_index(np.flatnonzero(live).astype(np.int32), P)
    n = int(live.sum())
    rng = np.random.default_rng(3)
    per_sample = rng.random((8, P)).astype(np.float32)
    src = np.stack([[per_sample[r, c * chunk_src:(c + 1) * chunk_src].max() for c in range(n_src)] for r in range(8)]).astype(np.float32)
    dst = np.full((8, n_dst), np.nan, np.float32)
    H.call("scnerf_live_remap_maxima", idx, n, src, n_src, chunk_src, dst, n_dst, chunk_dst, 8, None)
    for c in range(n_dst):
        rows = idx[c * chunk_dst:min((c + 1) * chunk_dst, n)]
        for r in range(8):
            assert dst[r, c] >= (per_sample[r, rows].max() if len(rows) else 0.0)
            assert dst[r, c] <= src[r].max()


def test_argument_errors():
    st = H.lib_call_status
    d = np.zeros((64, 4), np.float32)
    i32, u32, one = np.zeros(128, np.int32), np.zeros(128, np.uint32), np.zeros(1, np.int32)
    assert st("scnerf_live_compact", d, 0, i32, i32, u32, d.copy(), one, one.copy(), None) == EINVAL
    assert st("scnerf_live_compact", d, 64, i32, None, u32, d.copy(), one, one.copy(), None) == EINVAL
    assert st("scnerf_live_compact", d, 1 << 22, i32, i32, u32, d.copy(), one, one.copy(), None) != 0
    assert st("scnerf_live_compact", d, 64, i32, i32.copy(), u32, d.copy(), one, None, None) == 0       # the pinned word is optional
    assert st("scnerf_live_scatter_rows", d, i32, d.copy(), 65, 4, 64, None) == EINVAL


def _pass(P, spr, chunks, pts, vd, d_raw, p, lean):
    """forward, dense data gradients and the dense group; then the same on the live samples"""
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
    fp = flat_params(p, 3)
    if lean:
        H.call("scnerf_nerf_wgrad_h3_lean", 3, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, fp, None, None, None)
    else:
        H.call("scnerf_nerf_wgrad_h3", 3, save, grads, d_raw, P, chunks, ws, g, 0, mx, mz, sc, None, None, None)
    dense = dict(grads=grads, d_pts=d_pts, d_views=d_views, g=g)

    idx, xoff, d_live, n = _compact(d_raw)
    Pp, Pl = ML.padded_samples(P), ML.padded_samples(n)
    masks = save[lay.save_floats_per_sample * Pp:].view(np.uint32)
    m_l = np.zeros(ML.MASK_WORDS_PER_SAMPLE * Pl, np.uint32)
    p_l, v_l = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    H.call("scnerf_live_gather", idx, n, P, masks, pts, 3, vd, 3, spr, m_l, p_l, v_l, None)
    chunks_l = max(1, min(chunks, n // 64))
    nb_l = lib.scnerf_wgrad256_chunks(chunks_l)
    cs_l = lib.scnerf_wgrad_chunk_samples(n, nb_l)
    mx_l, mz_l = np.zeros((12, nb_l), np.float32), np.zeros((12, nb_l), np.float32)
    H.call("scnerf_live_remap_maxima", idx, n, mx, nb, cs, mx_l, nb_l, cs_l, 8, None)
    grads_l = np.full(ML.grad_floats(n), np.nan, np.float32)
    dp_l, dv_l = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
    H.call("scnerf_mlp_bwd_h3_masks", 3, d_live, p_l, v_l, 3, 1, wbk, bwd, sc, m_l, grads_l, dp_l, dv_l, n, mz_l, nb_l, cs_l,
           *NO_GUARD, lean, None)
    ws = np.full(lib.scnerf_nerf_wgrad_workspace_floats(chunks), np.nan, np.float32)
    g_l = np.full(lay.n_params, np.nan, np.float32)
    H.call("scnerf_nerf_wgrad_h3_live", 3, save, P, chunks, grads_l, d_raw, idx, xoff, n, chunks_l, ws, g_l, 0, mx_l, mz_l, sc,
           fp if lean else None, None, None, None)
    return dense, dict(grads=grads_l, d_pts=dp_l, d_views=dv_l, g=g_l, idx=idx[:n], n=n)


@pytest.mark.parametrize("lean", [0, 1])
def test_pass_on_the_live_samples_against_the_dense_pass(lean):
    n_rays, spr, chunks = 9, 34, 2                 # 306 samples: a partial 128-block, two chunks per job
    P = n_rays * spr
    p = network_params(3, 3)
    gen = torch.Generator().manual_seed(23)
    pts = (torch.rand(P, 3, generator=gen) * 2.4 - 1.2).numpy()
    vd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).numpy()
    live = R.patterns(P, seed=4)["random"]
    live[40:75] = False                            # a whole wave tile dead
    d_raw = R.d_raw_with(live, seed=5)
    dense, got = _pass(P, spr, chunks, pts, vd, d_raw, p, lean)
    idx, n = got["idx"], got["n"]
    assert n == int(live.sum())
    gd, gl = grad_views(dense["grads"], P), grad_views(got["grads"], n)
    for name in gd:
        if lean and name == "dfeat":
            continue
        np.testing.assert_array_equal(gl[name].view(np.uint32), gd[name][idx].view(np.uint32), err_msg=name)
        assert not gd[name][~live].any(), name                  # the dead rows of the dense launch are all +-0
    for k in ("d_pts", "d_views"):
        np.testing.assert_array_equal(got[k].view(np.uint32), dense[k][idx].view(np.uint32), err_msg=k)
        assert not dense[k][~live].any(), k
    OFF = ML.PARAM_OFFSETS
    a, b = dense["g"], got["g"]
    assert np.isfinite(a).all() and np.isfinite(b).all()
    for name, size in (("alpha_linear.weight", 256), ("alpha_linear.bias", 1), ("rgb_linear.weight", 384), ("rgb_linear.bias", 3)):
        np.testing.assert_array_equal(a[OFF[name]:OFF[name] + size].view(np.uint32), b[OFF[name]:OFF[name] + size].view(np.uint32), err_msg=name)
    for name, shape in ML.PARAM_SHAPES:
        x, y = a[OFF[name]:OFF[name] + int(np.prod(shape))], b[OFF[name]:OFF[name] + int(np.prod(shape))]
        # the same fp32-grade sums over differently cut chunks with other power-of-two scales: a few 1e-7 of the largest entry
        assert np.abs(x - y).max() <= 4e-6 * np.abs(x).max(), (name, np.abs(x - y).max() / np.abs(x).max())
